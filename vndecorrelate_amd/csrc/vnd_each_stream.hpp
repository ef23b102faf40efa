// vnd_each_stream.hpp - a pool streamed block by block through one filter PER STREAM (include/vnd_each_stream.h): the
// streaming side of vnd_each.hpp, which applies the batched optimisers' one kappa per signal to whole signals only.  (The
// HaasEffect entries of that header, one delay per stream, are in vnd_haas_stream.hpp beside the one-delay form.)
//
// each_stream_kernel relates to conv_stream_kernel (vnd_stream.hpp) the way each_kernel relates to conv_ordered_kernel.  A
// workgroup owns one tile of 2 * 256 * R output frames of one stream b and the candidate tables[b] of a bank (candidate t
// owns channels 2t, 2t + 1).  The pool advances in lockstep at ONE latency H, the bank's largest tap index: a call at
// position pos that pushes n_in frames writes the outputs [E, E') of vnd_stream.hpp with that H, whatever the stream's own
// filter reaches.  The workgroup stages the window [E + t0, E + t0 + tile + halo_of(H)) in CX LDS planes with
// stream_stage - the ring below pos, the caller's chunk up to pos + n_in, zeros past it - and runs each_tile
// (vnd_each.hpp: conv_ordered_kernel<MODE 0>'s bits; a tap that reaches past the end of the signal adds +-0 and drops
// out), storing through store_result and a raw buffer descriptor over the rest of the stream's row of THIS CALL's output:
// nothing at or past n_out is written.  The ring is vnd_stream.hpp's (RingArgs: its contract with reach = the bank's H);
// the same launch writes it (ring_write), and a call that only fills the ring launches one workgroup per stream.
//
// R is chosen per call, by make_stream_plan's rule (the largest tile that still leaves every CU six workgroups, else the
// smallest) among the tiles the call fills past half: live blocks are short, and each_kernel's fixed 2048-frame tile
// would leave three quarters of the lanes of a 480-frame block without frames.  Per output the operation sequence does not
// depend on R (vp_channel walks the taps in table order for every frame pair it holds), so the concatenated outputs are
// bit-identical to the one-shot call for every schedule - the argument vnd_stream.hpp makes for its exact and fma modes.
// The window always fits: a bank whose largest tap index is above VND_VELVET_PAIRS_MAX_TAP_INDEX is refused, so there is
// no direct fallback to carry.
#pragma once
#include "vnd_each.hpp"
#include "vnd_stream.hpp"
#include "../../include/vnd_each_stream.h"

namespace vnd {

struct EachStreamArgs {
    StreamArgs s;                                       // s.k: the bank's tables, k.y, k.n (= n_out), k.Cx, k.W, k.epi_*; s.r: the ring
    const int32_t *__restrict__ tables;                 // [batch]
    int32_t T;                                          // candidates in the bank
};

// grid = (max(1, ceil(n_out / tile)), batch); dynamic LDS = CX planes of k.W floats
template <int CX, int MODE, int R, bool EPI>
__global__ __launch_bounds__(kVpThreads) void each_stream_kernel(const EachStreamArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float es_lds[];
    constexpr int NT = kVpThreads, TILE = 2 * NT * R;
    const StreamArgs &sa = a.s;
    const KArgs &k = sa.k;
    const int64_t b = blockIdx.y;
    ring_write<NT>(sa.r, b, blockIdx.x, gridDim.x, (int)threadIdx.x);
    if (k.n == 0) return;                                          // (a call that only fills the ring)
    const int64_t t0 = (int64_t)blockIdx.x * TILE;
    float *dst = k.y + (b * k.n + t0) * 2;
    const v4i rdst = make_rsrc(dst, (k.n - t0) * 2 * 4);           // the rest of this stream's row of this call
    const int shape = access_shape<2>(dst, 2);                     // workgroup-uniform
    each_tile<CX, MODE, R, EPI>(
        k, es_lds, __builtin_amdgcn_readfirstlane(a.tables[b]), a.T,
        [&] { stream_stage<NT, CX>(sa.r, es_lds, b, sa.first_out + t0, 0, k.W, (int)threadIdx.x); },
        [&](int q, const float (&v)[4]) { store_result<2>(rdst, shape, k.stream_out, q, 1, 2, v); });
}

}  // namespace vnd

// ------------------------------------------------------------------------------
// C ABI (include/vnd_each_stream.h)
// ------------------------------------------------------------------------------
struct EachStreamPlan {
    int r = 1;                      // frame pairs per lane (tile = 2 * 256 * r frames)
    int W = 0;
    size_t lds_bytes = 0;
    int tiles = 1;
    uint32_t nblocks = 0;
    bool fma = false, epi = false;
};

typedef void (*each_stream_kern_t)(const EachStreamArgs);

template <int CX, int MODE, bool EPI>
static each_stream_kern_t each_stream_by_r(int r)
{
    switch (r) {
    case 1: return each_stream_kernel<CX, MODE, 1, EPI>;
    case 2: return each_stream_kernel<CX, MODE, 2, EPI>;
    case 4: return each_stream_kernel<CX, MODE, 4, EPI>;
    default: return nullptr;
    }
}

template <int CX>
static each_stream_kern_t each_stream_by_mode(const EachStreamPlan &p)
{
    if (p.epi) return p.fma ? each_stream_by_r<CX, 1, true>(p.r) : each_stream_by_r<CX, 0, true>(p.r);
    return p.fma ? each_stream_by_r<CX, 1, false>(p.r) : each_stream_by_r<CX, 0, false>(p.r);
}

static size_t each_stream_lds_need(int Cx, int r, int max_index)
{
    return (size_t)Cx * ((size_t)2 * kVpThreads * r + halo_of(max_index)) * sizeof(float);
}

// make_stream_plan's choice of the tile for a workgroup that owns both channels of a stream; the window always fits.
// One refinement: a tile that the call's frames do not fill past half is passed over.  A pool of 2048 streams makes six
// workgroups per CU at any tile, and the plain rule then gives a 480-frame block the 2048-frame tile - three quarters of the
// lanes without frames and four times the window staged (measured: DESIGN.md 3.15).
static EachStreamPlan make_each_stream_plan(const vnd_ctx *ctx, const vnd_taps *t, int64_t batch, int64_t n_out, int Cx, bool epi)
{
    EachStreamPlan p;
    const int cus = ctx->prop.multiProcessorCount > 0 ? ctx->prop.multiProcessorCount : 256;
    const size_t limit = (size_t)ctx->lds_limit - 1024;
    int r = 1;
    for (int cand : {4, 2}) {
        const int64_t T = (int64_t)2 * kVpThreads * cand;
        const int64_t tiles = (n_out + T - 1) / T;
        if (tiles == (n_out + T / 2 - 1) / (T / 2)) continue;          // half the tile covers the call with as few workgroups
        if (batch * tiles >= (int64_t)cus * 6 && each_stream_lds_need(Cx, cand, t->max_index) <= limit / 4) { r = cand; break; }
    }
    const int64_t T = (int64_t)2 * kVpThreads * r;
    p.r = r;
    p.W = (int)T + halo_of(t->max_index);
    p.lds_bytes = each_stream_lds_need(Cx, r, t->max_index);
    p.tiles = (int)std::max<int64_t>(1, (n_out + T - 1) / T);          // (a call that only fills the ring: one tile)
    p.nblocks = (uint32_t)(batch * p.tiles);
    p.fma = arithmetic_of(t, VND_MODE_EXACT) != VND_MODE_EXACT;        // +-1 weights: the same bits
    p.epi = epi;
    return p;
}

extern "C" {

static_assert(2 * (2 * vnd::kVpThreads * 4 + vnd::kVpMaxHalo) * sizeof(float) + 1024 <= 65536, "the r = 4 window fits the default LDS limit");

vnd_status vnd_each_stream_state_bytes(const vnd_taps *t, int64_t batch, int32_t in_channels, int64_t max_frames_per_call,
                                       int64_t *bytes)
{
    if (!t || !bytes) return fail(VND_ERR_INVALID, "null tap table or bytes");
    *bytes = 0;
    if (batch < 0) return fail(VND_ERR_INVALID, "negative batch");
    if (in_channels != 1 && in_channels != 2)
        return fail(VND_ERR_INVALID, "a pool of mono or stereo streams is taken, got %d channels", in_channels);
    if (max_frames_per_call < 0 || max_frames_per_call > ((int64_t)1 << 40))
        return fail(VND_ERR_INVALID, "max_frames_per_call %lld out of range", (long long)max_frames_per_call);
    if (batch > VND_MAX_STREAMS) return fail(VND_ERR_UNSUPPORTED, "more than %d streams per call: split the pool", VND_MAX_STREAMS);
    *bytes = batch * stream_capacity(t, max_frames_per_call) * in_channels * (int64_t)sizeof(float);
    return VND_OK;
}

// The scalar checks - the union of stream_check's and each_check's; *n_out from position, n_in, H and final alone.
// (Its position and frame-count lines stay here, not in block_stream_check: this entry reports the range of
// max_frames_per_call between them, and the bank's limits before the size of the state.)
static vnd_status each_stream_scalars(const vnd_ctx *ctx, const vnd_taps *t, int64_t max_frames_per_call, int64_t batch,
                                      int64_t pos, int64_t n_in, int32_t Cx, int32_t final_, int32_t mode, int64_t *n_out)
{
    if (!ctx || !t) return fail(VND_ERR_INVALID, "null context or tap table");
    if (!n_out) return fail(VND_ERR_INVALID, "null n_out");
    *n_out = 0;
    if (batch < 0 || n_in < 0) return fail(VND_ERR_INVALID, "negative batch or frame count");
    if (Cx != 1 && Cx != 2) return fail(VND_ERR_INVALID, "a pool of mono or stereo streams is taken, got %d channels", Cx);
    vnd_status st = each_bank_pairs(ctx, t);
    if (st != VND_OK) return st;
    if (pos < 0 || pos > ((int64_t)1 << 60)) return fail(VND_ERR_INVALID, "position %lld out of range", (long long)pos);
    if (max_frames_per_call < 0 || max_frames_per_call > ((int64_t)1 << 40))
        return fail(VND_ERR_INVALID, "max_frames_per_call %lld out of range", (long long)max_frames_per_call);
    if (n_in > max_frames_per_call)
        return fail(VND_ERR_INVALID, "%lld frames in one call, above max_frames_per_call %lld", (long long)n_in,
                    (long long)max_frames_per_call);
    if ((st = each_bank_limits(t, batch, mode, "stream", "streams", "stream it filter by filter")) != VND_OK) return st;
    const int64_t H = t->max_index;
    const int64_t e0 = std::max<int64_t>(0, pos - H);
    const int64_t e1 = final_ ? pos + n_in : std::max<int64_t>(0, pos + n_in - H);
    if (batch * (e1 - e0) * 2 > ((int64_t)1 << 40)) return fail(VND_ERR_UNSUPPORTED, "problem too large");
    *n_out = e1 - e0;
    return VND_OK;
}

// Every argument check, before anything is enqueued and with nothing written but *n_out.
static vnd_status each_stream_check(const vnd_ctx *ctx, const vnd_taps *t, const int32_t *tables, const void *state,
                                    int64_t state_bytes, int64_t max_frames_per_call, const float *x, const float *y,
                                    int64_t batch, int64_t pos, int64_t n_in, int32_t Cx, int32_t final_, int32_t mode,
                                    int64_t *n_out)
{
    vnd_status st = each_stream_scalars(ctx, t, max_frames_per_call, batch, pos, n_in, Cx, final_, mode, n_out);
    if (st != VND_OK) return st;
    const int64_t nout = *n_out;
    *n_out = 0;
    int64_t need = 0;
    if ((st = vnd_each_stream_state_bytes(t, batch, Cx, max_frames_per_call, &need)) != VND_OK) return st;
    if ((st = block_stream_check(pos, n_in, max_frames_per_call, state_bytes, need)) != VND_OK) return st;   // (the state: the rest has passed)
    if (batch > 0 && ((need > 0 && !state) || (n_in > 0 && !x) || (nout > 0 && !y) || ((n_in > 0 || nout > 0) && !tables)))
        return fail(VND_ERR_INVALID, "null state, chunk, output or table index pointer");
    *n_out = nout;
    return VND_OK;
}

vnd_status vnd_each_stream_f32_dev(vnd_ctx *ctx, const vnd_taps *t, const int32_t *tables, void *state, int64_t state_bytes,
                                   int64_t max_frames_per_call, const float *x, float *y, int64_t batch, int64_t pos,
                                   int64_t n_in, int32_t Cx, int32_t final_, int32_t mode, int32_t ms_encode,
                                   int32_t use_width, double width, int64_t *n_out, void *stream_)
{
    vnd_status st = each_stream_check(ctx, t, tables, state, state_bytes, max_frames_per_call, x, y, batch, pos, n_in, Cx,
                                      final_, mode, n_out);
    if (st != VND_OK) return st;
    const int64_t H = t->max_index, nout = *n_out;
    EachStreamArgs a{};
    StreamArgs &sa = a.s;
    sa.r = ring_plan(pos, n_in, H, final_, stream_capacity(t, max_frames_per_call));
    sa.r.chunk = x; sa.r.ring = (float *)state; sa.r.Cx = Cx;
    sa.first_out = std::max<int64_t>(0, pos - H);
    if (ring_idle(sa.r, batch, nout)) return VND_OK;
    const bool epi = ms_encode || use_width;
    const EachStreamPlan p = make_each_stream_plan(ctx, t, batch, nout, Cx, epi);
    KArgs &k = sa.k;
    table_args(k, t);
    k.y = y; k.n = nout; k.C = t->C; k.Cx = Cx; k.W = p.W;
    k.epi_ms_encode = ms_encode ? 1 : 0; k.epi_use_width = use_width ? 1 : 0;
    k.epi_w_mid = (float)(1.0 - width); k.epi_w_side = (float)width;       // as the decorrelate stage passes the width
    a.tables = tables; a.T = t->C / 2;
    DeviceScope on(ctx->device);
    if (!on.ok) return fail(VND_ERR_HIP, "cannot select device %d", ctx->device);
    each_stream_kern_t kern = Cx == 2 ? each_stream_by_mode<2>(p) : each_stream_by_mode<1>(p);
    if (!kern) return fail(VND_ERR_UNSUPPORTED, "no stream kernel for this tile shape");
    hipLaunchKernelGGL(kern, dim3((unsigned)p.tiles, (unsigned)batch), dim3(kVpThreads), p.lds_bytes, (hipStream_t)stream_, a);
    HIP_TRY(hipGetLastError());
    return VND_OK;
}

vnd_status vnd_each_stream_f32_host(vnd_ctx *ctx, const vnd_taps *t, const int32_t *tables, void *state, int64_t state_bytes,
                                    int64_t max_frames_per_call, const float *x, float *y, int64_t batch, int64_t pos,
                                    int64_t n_in, int32_t Cx, int32_t final_, int32_t mode, int32_t ms_encode,
                                    int32_t use_width, double width, int64_t *n_out)
{
    vnd_status st = each_stream_check(ctx, t, tables, state, state_bytes, max_frames_per_call, x, y, batch, pos, n_in, Cx,
                                      final_, mode, n_out);
    if (st != VND_OK) return st;
    const int64_t nout = *n_out;
    if (batch == 0 || (n_in == 0 && nout == 0)) return VND_OK;
    const HostIndex ix{tables, t->C / 2, false, "table", "tables", "stream"};
    HostCall call(ctx);
    call.staged(x, (size_t)(batch * n_in * Cx) * sizeof(float), "the chunk", y, (size_t)(batch * nout * 2) * sizeof(float), &ix,
                batch, 0, n_out, [&](void *x_dev, void *y_dev, int32_t *t_dev, void *, hipStream_t s) {
        int64_t got = 0;
        return vnd_each_stream_f32_dev(ctx, t, t_dev, state, state_bytes, max_frames_per_call, (const float *)x_dev, (float *)y_dev,
                                       batch, pos, n_in, Cx, final_, mode, ms_encode, use_width, width, &got, s);
    });
    return call.finish("vnd_each_stream_f32_host");
}

}  // extern "C"

// vnd_each_stream.hpp - a pool streamed block by block through one filter or one delay PER STREAM
// (include/vnd_each_stream.h): the streaming side of vnd_each.hpp, which applies the batched optimisers' one kappa or one
// delay per signal to whole signals only.
//
// Velvet noise: each_stream_kernel relates to conv_stream_kernel (vnd_stream.hpp) the way each_kernel relates to
// conv_ordered_kernel.  A workgroup owns one tile of 2 * 256 * R output frames of one stream b and the candidate
// tables[b] of a bank (candidate t owns channels 2t, 2t + 1).  The pool advances in lockstep at ONE latency H, the bank's
// largest tap index: a call at position pos that pushes n_in frames writes the outputs [E, E') of vnd_stream.hpp with that
// H, whatever the stream's own filter reaches.  The workgroup stages the window [E + t0, E + t0 + tile + halo_of(H)) in
// CX LDS planes with stream_stage - the ring below pos, the caller's chunk up to pos + n_in, zeros past it - forms its
// frames with vp_channel<MODE, R> (conv_ordered_kernel<MODE 0>'s bits: the same helpers in the same order; a tap that
// reaches past the end of the signal adds +-0 and drops out), applies epi_pointwise on the input frames still staged and
// stores through store_result and a raw buffer descriptor over the rest of the stream's row of THIS CALL's output:
// nothing at or past n_out is written.  The same launch copies the chunk's last min(n_in, H) frames into the ring
// (stream_ring_write); a call that only fills the ring launches one workgroup per stream.
//
// Capacity (vnd_stream.hpp's argument with the bank's H): the ring holds H + max_frames_per_call frames, slot = absolute
// frame mod capacity.  A frame f read from the ring and a frame g written in the same call have
// 0 < g - f <= H + n_in - 1 < capacity, so no slot is both read and written in one call, and every frame is written once.
//
// R is chosen per call, by make_stream_plan's rule (the largest tile that still leaves every CU six workgroups, else the
// smallest) among the tiles the call fills past half: live blocks are short, and each_kernel's fixed 2048-frame tile
// would leave three quarters of the lanes of a 480-frame block without frames.  Per output the operation sequence does not depend on R (vp_channel walks the taps in
// table order for every frame pair it holds), so the concatenated outputs are bit-identical to the one-shot call for
// every schedule - the argument vnd_stream.hpp makes for its exact and fma modes.  The window always fits: a bank whose
// largest tap index is above VND_VELVET_PAIRS_MAX_TAP_INDEX is refused, so there is no direct fallback to carry.
//
// HaasEffect: haas_each_stream_kernel is haas_stream_kernel (vnd_haas_stream.hpp) with the delay read per stream.  The
// ring holds max_delay + max_frames_per_call frames and every call writes the chunk's last min(n_in, max_delay) frames,
// so the frames [pos - max_delay, pos) are there for every stream's d_b <= max_delay.  The final call returns
// n_in + max_delay frames per stream; those at or past the stream's own n + d_b are written as +0.0.
#pragma once
#include "vnd_each.hpp"
#include "vnd_haas_stream.hpp"
#include "vnd_stream.hpp"
#include "../../include/vnd_each_stream.h"

namespace vnd {

struct EachStreamArgs {
    StreamArgs s;                                       // s.k: the bank's tables, k.y, k.n (= n_out), k.Cx, k.W, k.epi_*
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
    const int tid = threadIdx.x;
    const int W = k.W;
    const int64_t b = blockIdx.y;
    stream_ring_write<NT>(sa, b, blockIdx.x, gridDim.x, tid);
    if (k.n == 0) return;                                          // (a call that only fills the ring)
    const int64_t t0 = (int64_t)blockIdx.x * TILE;
    float *dst = k.y + (b * k.n + t0) * 2;
    const v4i rdst = make_rsrc(dst, (k.n - t0) * 2 * 4);           // the rest of this stream's row of this call
    const int shape = access_shape<2>(dst, 2);                     // workgroup-uniform
    const int32_t cand = __builtin_amdgcn_readfirstlane(a.tables[b]);
    if (cand < 0 || cand >= a.T) {                                 // outside the contract: the stream's row is NaN
        const float nan = __builtin_nanf("");
        const float v[4] = {nan, nan, nan, nan};
#pragma unroll
        for (int j = 0; j < R; ++j) store_result<2>(rdst, shape, k.stream_out, tid + NT * j, 1, 2, v);
        return;
    }
    stream_stage<NT, CX>(sa, es_lds, b, sa.first_out + t0, 0, W, tid);
    __syncthreads();
    const float *right = es_lds + (CX == 2 ? W : 0);
    v2f out[2][R];
    vp_channel<MODE, R>(k, 2 * cand, es_lds + 2 * tid, out[0]);
    vp_channel<MODE, R>(k, 2 * cand + 1, right + 2 * tid, out[1]);
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const int q = tid + NT * j;
        float v[4] = {out[0][j].x, out[1][j].x, out[0][j].y, out[1][j].y};
        if constexpr (EPI) {
            const float2 x0 = *(const float2 *)(es_lds + 2 * q), x1 = *(const float2 *)(right + 2 * q);
            const float xin[4] = {x0.x, x1.x, x0.y, x1.y};
            epi_pointwise(k, v, xin);
        }
        store_result<2>(rdst, shape, k.stream_out, q, 1, 2, v);
    }
}

struct HesArgs {
    HArgs h;                           // Cx, delayed_channel, ms, use_width, w_mid, w_side (h.x, h.y, h.n, h.delay unused)
    const float *__restrict__ chunk;   // [batch][n_in][Cx]
    float *__restrict__ ring;          // [batch][cap][Cx]
    double *__restrict__ y;            // [batch][n_out][2]
    const int32_t *__restrict__ delays;    // [batch]
    int64_t pos, n_in, n_out;
    int64_t cap;                       // ring capacity, frames: max_delay + max_frames_per_call
    int64_t ring_first, ring_slot0;    // pos - max_delay (may be below 0) and its slot, ring_first mod cap in [0, cap)
    int64_t wr_first, wr_count, wr_slot0;   // chunk frames [wr_first, wr_first + wr_count) (absolute) go to the ring
    int32_t max_delay;
};

// Input frame f >= pos - d of stream s, d <= max_delay, as float32 samples widened to double: (l, r), r = 0 for mono.
// false: frame f reads as zeros, and nothing is loaded.  A frame in [0, pos) comes from the ring at
// ring_slot0 + (f - ring_first), less cap if that is past the end: 0 <= f - ring_first < max_delay <= cap and
// 0 <= ring_slot0 < cap, so the slot is in [0, cap); it is f mod cap because ring_slot0 = ring_first mod cap.
__device__ __forceinline__ bool haas_each_stream_frame(const HesArgs &a, int64_t s, int64_t f, double &l, double &r)
{
    const int Cx = a.h.Cx;
    if (f < 0 || f >= a.pos + a.n_in) return false;
    const float *__restrict__ p;
    if (f >= a.pos) {
        p = a.chunk + (s * a.n_in + (f - a.pos)) * Cx;
    } else {
        int64_t slot = a.ring_slot0 + (f - a.ring_first);
        if (slot >= a.cap) slot -= a.cap;
        p = a.ring + (s * a.cap + slot) * Cx;
    }
    if (Cx == 1) {
        l = (double)p[0]; r = 0.0;
    } else {
        const float2 v = *(const float2 *)p;
        l = (double)v.x; r = (double)v.y;
    }
    return true;
}

// grid = (max(1, ceil(n_out / kHaasStreamThreads)), batch): one lane per output frame
__global__ __launch_bounds__(kHaasStreamThreads) void haas_each_stream_kernel(const HesArgs a)
{
    const int64_t s = blockIdx.y;
    const int tid = threadIdx.x;
    // the chunk frames later calls read, into the ring: the stream's workgroups share them in grid-stride order
    if (a.wr_count > 0) {
        const int Cx = a.h.Cx;
        const int64_t total = a.wr_count * Cx, capf = a.cap * Cx;
        const float *__restrict__ src = a.chunk + (s * a.n_in + (a.wr_first - a.pos)) * Cx;
        float *__restrict__ dst = a.ring + s * capf;
        const int64_t s0 = a.wr_slot0 * Cx;
        for (int64_t e = (int64_t)blockIdx.x * kHaasStreamThreads + tid; e < total;
             e += (int64_t)gridDim.x * kHaasStreamThreads) {
            int64_t slot = s0 + e;
            if (slot >= capf) slot -= capf;
            dst[slot] = src[e];
        }
    }
    const int64_t k = (int64_t)blockIdx.x * kHaasStreamThreads + tid;
    if (k >= a.n_out) return;
    const int64_t t = a.pos + k;
    const int32_t d = a.delays[s];
    double v[2];
    if (d < 0 || d > a.max_delay) {                     // outside the contract: the stream's rows are NaN
        v[0] = v[1] = __builtin_nan("");
    } else if (t >= a.pos + a.n_in + d) {               // past this stream's own n + d frames (final call): padding
        v[0] = v[1] = 0.0;
    } else {
        double c[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            double l = 0.0, r = 0.0;
            const bool in = haas_each_stream_frame(a, s, j == a.h.delayed_channel ? t - d : t, l, r);
            c[j] = in ? haas_column_of(a.h, j, l, r) : 0.0;                               // np.roll: zeros wrap in
        }
        haas_frame(a.h, c[0], c[1], v);
    }
    *(double2 *)(a.y + (s * a.n_out + k) * 2) = make_double2(v[0], v[1]);
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
static vnd_status each_stream_scalars(const vnd_ctx *ctx, const vnd_taps *t, int64_t max_frames_per_call, int64_t batch,
                                      int64_t pos, int64_t n_in, int32_t Cx, int32_t final_, int32_t mode, int64_t *n_out)
{
    if (!ctx || !t) return fail(VND_ERR_INVALID, "null context or tap table");
    if (!n_out) return fail(VND_ERR_INVALID, "null n_out");
    *n_out = 0;
    if (batch < 0 || n_in < 0) return fail(VND_ERR_INVALID, "negative batch or frame count");
    if (Cx != 1 && Cx != 2) return fail(VND_ERR_INVALID, "a pool of mono or stereo streams is taken, got %d channels", Cx);
    if (t->C % 2 != 0) return fail(VND_ERR_INVALID, "a bank holds stereo pairs: this one has %d channels", t->C);
    if (t->ctx != ctx && t->ctx->device != ctx->device)
        return fail(VND_ERR_INVALID, "the tap table lives on device %d, the context on device %d", t->ctx->device, ctx->device);
    if (pos < 0 || pos > ((int64_t)1 << 60)) return fail(VND_ERR_INVALID, "position %lld out of range", (long long)pos);
    if (max_frames_per_call < 0 || max_frames_per_call > ((int64_t)1 << 40))
        return fail(VND_ERR_INVALID, "max_frames_per_call %lld out of range", (long long)max_frames_per_call);
    if (n_in > max_frames_per_call)
        return fail(VND_ERR_INVALID, "%lld frames in one call, above max_frames_per_call %lld", (long long)n_in,
                    (long long)max_frames_per_call);
    if (mode != VND_MODE_EXACT) return fail(VND_ERR_UNSUPPORTED, "a filter per stream runs in VND_MODE_EXACT only, got mode %d", mode);
    if (batch > VND_MAX_STREAMS) return fail(VND_ERR_UNSUPPORTED, "more than %d streams per call: split the pool", VND_MAX_STREAMS);
    if (t->max_index > VND_VELVET_PAIRS_MAX_TAP_INDEX || !t->lds_images)
        return fail(VND_ERR_UNSUPPORTED, "the bank's largest tap index %d is above %d: stream it filter by filter", t->max_index,
                    VND_VELVET_PAIRS_MAX_TAP_INDEX);
    if (t->nonfinite) return fail(VND_ERR_UNSUPPORTED, "the bank has a weight that is not finite: stream it filter by filter");
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
    if (state_bytes < need)
        return fail(VND_ERR_INVALID, "state of %lld bytes, the stream needs %lld", (long long)state_bytes, (long long)need);
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
    sa.chunk = x; sa.ring = (float *)state;
    sa.pos = pos; sa.n_in = n_in; sa.first_out = std::max<int64_t>(0, pos - H);
    sa.cap = stream_capacity(t, max_frames_per_call);
    // the last H frames of the chunk are what later calls read (none after the final call)
    sa.wr_first = final_ ? pos + n_in : std::max<int64_t>(pos, pos + n_in - H);
    sa.wr_count = pos + n_in - sa.wr_first;
    if (batch == 0 || (nout == 0 && sa.wr_count == 0)) return VND_OK;
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
    for (int64_t b = 0; b < batch; ++b)
        if (tables[b] < 0 || tables[b] >= t->C / 2) {
            *n_out = 0;
            return fail(VND_ERR_INVALID, "table %d of stream %lld is outside [0, %d)", tables[b], (long long)b, t->C / 2);
        }
    HostCall call(ctx);
    const size_t x_bytes = (size_t)(batch * n_in * Cx) * sizeof(float);
    const size_t y_bytes = (size_t)(batch * nout * 2) * sizeof(float);
    const size_t i_bytes = (size_t)batch * sizeof(int32_t);
    call.carve({x_bytes, y_bytes, i_bytes});
    float *x_dev = call.piece<float>(0), *y_dev = call.piece<float>(1);
    int32_t *t_dev = call.piece<int32_t>(2);
    call.up(x_dev, x, x_bytes, "the chunk");
    call.up(t_dev, tables, i_bytes, "tables");
    int64_t got = 0;
    call.run([&] { return vnd_each_stream_f32_dev(ctx, t, t_dev, state, state_bytes, max_frames_per_call, x_dev, y_dev, batch, pos,
                                                  n_in, Cx, final_, mode, ms_encode, use_width, width, &got, call.stream()); });
    call.down(y, y_dev, y_bytes, "y");
    return call.finish("vnd_each_stream_f32_host");
}

// ---- HaasEffect with a delay per stream -------------------------------------------------------------------------------
vnd_status vnd_haas_each_stream_state_bytes(int64_t batch, int32_t in_channels, int32_t max_delay, int64_t max_frames_per_call,
                                            int64_t *bytes)
{
    if (!bytes) return fail(VND_ERR_INVALID, "null bytes");
    *bytes = 0;
    if (batch < 0) return fail(VND_ERR_INVALID, "negative batch");
    if (in_channels != 1 && in_channels != 2)
        return fail(VND_ERR_INVALID, "HaasEffect takes a mono or stereo signal, got %d channels", in_channels);
    if (max_delay < 0) return fail(VND_ERR_INVALID, "negative max_delay %d", max_delay);
    if (max_frames_per_call < 0 || max_frames_per_call > ((int64_t)1 << 40))
        return fail(VND_ERR_INVALID, "max_frames_per_call %lld out of range", (long long)max_frames_per_call);
    if (batch > VND_MAX_STREAMS) return fail(VND_ERR_UNSUPPORTED, "more than %d streams per call: split the pool", VND_MAX_STREAMS);
    if (max_delay == 0) return VND_OK;                   // no frame is ever read back: no state
    *bytes = batch * haas_stream_capacity(max_delay, max_frames_per_call) * in_channels * (int64_t)sizeof(float);
    return VND_OK;
}

// Every argument check, before anything is enqueued; *n_out from n_in, max_delay and final alone.
static vnd_status haas_each_stream_check(const vnd_ctx *ctx, const void *state, int64_t state_bytes, int64_t max_frames_per_call,
                                         const float *x, const double *y, int64_t batch, int64_t pos, int64_t n_in,
                                         int32_t Cx, int32_t final_, const int32_t *delays, int32_t max_delay,
                                         int32_t delayed_channel, int64_t *n_out)
{
    if (!ctx) return fail(VND_ERR_INVALID, "null context");
    if (!n_out) return fail(VND_ERR_INVALID, "null n_out");
    *n_out = 0;
    int64_t need = 0;
    vnd_status st = vnd_haas_each_stream_state_bytes(batch, Cx, max_delay, max_frames_per_call, &need);
    if (st != VND_OK) return st;
    if (delayed_channel != 0 && delayed_channel != 1)
        return fail(VND_ERR_INVALID, "delayed_channel must be 0 or 1, got %d", delayed_channel);
    if (pos < 0 || pos > ((int64_t)1 << 60)) return fail(VND_ERR_INVALID, "position %lld out of range", (long long)pos);
    if (n_in < 0) return fail(VND_ERR_INVALID, "negative frame count");
    if (n_in > max_frames_per_call)
        return fail(VND_ERR_INVALID, "%lld frames in one call, above max_frames_per_call %lld", (long long)n_in,
                    (long long)max_frames_per_call);
    if (state_bytes < need)
        return fail(VND_ERR_INVALID, "state of %lld bytes, the stream needs %lld", (long long)state_bytes, (long long)need);
    const int64_t total = n_in + (final_ ? max_delay : 0);
    if (batch > 0 && ((need > 0 && !state) || (n_in > 0 && !x) || (total > 0 && (!y || !delays))))
        return fail(VND_ERR_INVALID, "null state, chunk, output or delay pointer");
    if (batch * total * 2 > ((int64_t)1 << 40)) return fail(VND_ERR_UNSUPPORTED, "problem too large");
    *n_out = total;
    return VND_OK;
}

vnd_status vnd_haas_each_stream_f64_dev(vnd_ctx *ctx, void *state, int64_t state_bytes, int64_t max_frames_per_call,
                                        const float *x, double *y, int64_t batch, int64_t pos, int64_t n_in, int32_t Cx,
                                        int32_t final_, const int32_t *delays, int32_t max_delay, int32_t delayed_channel,
                                        int32_t ms_mode, int32_t use_width, double width, int64_t *n_out, void *stream)
{
    vnd_status st = haas_each_stream_check(ctx, state, state_bytes, max_frames_per_call, x, y, batch, pos, n_in, Cx, final_,
                                           delays, max_delay, delayed_channel, n_out);
    if (st != VND_OK) return st;
    using namespace vnd;
    HesArgs a{};
    a.h.Cx = Cx; a.h.delayed_channel = delayed_channel;
    a.h.ms = ms_mode ? 1 : 0; a.h.use_width = use_width ? 1 : 0; a.h.w_mid = 1.0 - width; a.h.w_side = width;
    a.chunk = x; a.ring = (float *)state; a.y = y; a.delays = delays; a.max_delay = max_delay;
    a.pos = pos; a.n_in = n_in; a.n_out = *n_out;
    a.cap = haas_stream_capacity(max_delay, max_frames_per_call);
    a.ring_first = pos - max_delay;
    a.ring_slot0 = a.cap > 0 ? ((a.ring_first % a.cap) + a.cap) % a.cap : 0;
    // the last max_delay frames of the chunk are what later calls read (none after the final call, none without a delay)
    a.wr_first = (final_ || max_delay == 0) ? pos + n_in : std::max<int64_t>(pos, pos + n_in - max_delay);
    a.wr_count = pos + n_in - a.wr_first;
    a.wr_slot0 = a.cap > 0 ? a.wr_first % a.cap : 0;
    if (batch == 0 || (a.n_out == 0 && a.wr_count == 0)) return VND_OK;
    const int64_t blocks = std::max<int64_t>(1, (a.n_out + kHaasStreamThreads - 1) / kHaasStreamThreads);
    if (blocks > 0x7fffffffLL) return fail(VND_ERR_UNSUPPORTED, "too many frames in one call");
    DeviceScope on(ctx->device);
    if (!on.ok) return fail(VND_ERR_HIP, "cannot select device %d", ctx->device);
    hipLaunchKernelGGL(haas_each_stream_kernel, dim3((unsigned)blocks, (unsigned)batch), dim3(kHaasStreamThreads), 0,
                       (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return VND_OK;
}

vnd_status vnd_haas_each_stream_f64_host(vnd_ctx *ctx, void *state, int64_t state_bytes, int64_t max_frames_per_call,
                                         const float *x, double *y, int64_t batch, int64_t pos, int64_t n_in, int32_t Cx,
                                         int32_t final_, const int32_t *delays, int32_t max_delay, int32_t delayed_channel,
                                         int32_t ms_mode, int32_t use_width, double width, int64_t *n_out)
{
    vnd_status st = haas_each_stream_check(ctx, state, state_bytes, max_frames_per_call, x, y, batch, pos, n_in, Cx, final_,
                                           delays, max_delay, delayed_channel, n_out);
    if (st != VND_OK) return st;
    const int64_t nout = *n_out;
    if (batch == 0 || (n_in == 0 && nout == 0)) return VND_OK;
    for (int64_t b = 0; b < batch; ++b)
        if (delays[b] < 0 || delays[b] > max_delay) {
            *n_out = 0;
            return fail(VND_ERR_INVALID, "delay %d of stream %lld is outside [0, %d]", delays[b], (long long)b, max_delay);
        }
    HostCall call(ctx);
    const size_t x_bytes = (size_t)(batch * n_in * Cx) * sizeof(float);
    const size_t y_bytes = (size_t)(batch * nout * 2) * sizeof(double);
    const size_t d_bytes = (size_t)batch * sizeof(int32_t);
    call.carve({y_bytes, x_bytes, d_bytes});
    double *y_dev = call.piece<double>(0);
    float *x_dev = call.piece<float>(1);
    int32_t *d_dev = call.piece<int32_t>(2);
    call.up(x_dev, x, x_bytes, "the chunk");
    call.up(d_dev, delays, d_bytes, "delays");
    int64_t got = 0;
    call.run([&] { return vnd_haas_each_stream_f64_dev(ctx, state, state_bytes, max_frames_per_call, x_dev, y_dev, batch, pos, n_in,
                                                       Cx, final_, d_dev, max_delay, delayed_channel, ms_mode, use_width, width,
                                                       &got, call.stream()); });
    call.down(y, y_dev, y_bytes, "y");
    return call.finish("vnd_haas_each_stream_f64_host");
}

}  // extern "C"

// vnd_voice_stream.hpp - a voice pool (include/vnd_voice_stream.h): the block stream of vnd_each_stream.hpp with the
// stream position moved from the caller into the device state, one per slot, and a frame count and start / end flags per
// slot and call.  A slot is a voice with a life of its own, and a call is a pure function of device memory: it can be
// captured in a graph and replayed.
//
// voice_stream_kernel is the sibling of each_stream_kernel.  Its grid is fixed by the pool - (slots, ceil((M + H) / tile)),
// the longest row a call can write - and not by the call.  The SLOT is the fast dimension: workgroups are dealt round-robin
// over the 8 XCDs by their linear index, and in steady state only the first tiles of a row have frames - with the tile as
// the fast dimension and 4 tiles per row every working workgroup landed on two XCDs, and the kernel took 2.6 times the
// lockstep kernel's time.  A workgroup reads pos[b], counts[b], flags[b] and tables[b] of
// its slot once, workgroup-uniform, and derives from them what the host derives for the lockstep streams: the span
// (voice_span) and the ring side of the call (ring_plan, the host's own function).  It then builds a RingArgs whose chunk
// and ring pointers are offset to slot b, so ring_write, stream_stage, each_tile and store_result are called unchanged
// with stream 0.  Per output the operation sequence is each_stream_kernel's, which depends neither on the tile nor on
// the call, so a voice's concatenated outputs are the one-shot call's bit for bit, whatever its neighbours do.
//
// Every index that is built from device data:
//   - counts[b] outside [0, M]: the workgroup leaves before anything is addressed with it;
//   - pos[b] outside [0, 2^60] (a state that was never reset) without START: the same - so p >= 0 below;
//   - chunk frames: ring_write reads [wr_first - p, n) of the slot's row of x, stream_stage [0, n): both inside [0, M);
//   - ring slots: wr_slot0 = wr_first % cap and base % cap lie in [0, cap), each walked forward with one wrap; a read
//     slot belongs to a frame in [p - H, p), a written one to [p, p + n): less than cap = H + M apart (vnd_stream.hpp);
//   - y: the descriptor covers (n_out - t0) frames of row b from t0 on, n_out <= M + H = the row; t0 < n_out;
//   - tables[b]: each_tile's bounds check (NaN rows), nothing is indexed with a bad one.
//
// voice_advance_kernel<VoiceStreamArgs>, one lane per slot, follows on the same stream and writes pos[b] and out_counts[b]
// (vnd_voice_core.hpp: the slot rule, and why a kernel boundary orders the reads of pos[b] before its update).
#pragma once
#include "vnd_each_stream.hpp"
#include "vnd_voice_core.hpp"

namespace vnd {

constexpr int64_t kVoiceMaxFrames = (int64_t)1 << 24;     // tiles of a row <= 65535 at the smallest tile; counts are int32

// One slot's side of a call, from the stored position, counts[b] and flags[b] alone (include/vnd_voice_stream.h).
// The slot rule is written out here, not taken from voice_head (vnd_voice_core.hpp, which the two meters use): with the
// head in between the compiler orders the scalar preamble of voice_stream_kernel and haas_voice_stream_kernel differently,
// and these two are the kernels a decorrelating server runs per block.  What holds this text and voice_head to one rule
// is the pools' GPU tests, which compare every pool's out_counts and positions with the NumPy mirrors call by call, bad
// and idle slots planted; tests/test_voice_spans_cpu.py holds those mirrors, not this text, to the headers' formulas.
struct VoiceSpan {
    int64_t p, n;                  // position the call starts at, frames pushed
    int64_t first_out, n_out;      // E, E' - E
    int64_t next;                  // the position after the call
    bool end, ok;                  // !ok: a bad count or position - the slot is left alone, out_counts = -1
};

__host__ __device__ inline VoiceSpan voice_span(int64_t stored, int32_t count, int32_t flags, int64_t M, int64_t H)
{
    VoiceSpan v{};
    v.end = (flags & VND_VOICE_END) != 0;
    v.p = (flags & VND_VOICE_START) ? 0 : stored;
    v.ok = count >= 0 && count <= M && v.p >= 0 && v.p <= kVoiceMaxPosition;
    if (!v.ok) { v.p = 0; v.next = stored; v.n_out = -1; return v; }
    v.n = count;
    const int64_t held = v.p - H, ready = v.p + v.n - H;
    v.first_out = held > 0 ? held : 0;
    const int64_t e1 = v.end ? v.p + v.n : (ready > 0 ? ready : 0);
    v.n_out = e1 - v.first_out;
    v.next = v.end ? 0 : v.p + v.n;
    return v;
}

struct VoiceStreamArgs {
    KArgs k;                                            // the bank's tables, k.C, k.Cx, k.W, k.epi_*; k.y and k.n are not read
    const float *__restrict__ x;                        // [slots][M][Cx]
    float *__restrict__ y;                              // [slots][M + H][2]
    float *__restrict__ ring;                           // [slots][cap][Cx]
    int64_t *__restrict__ pos;                          // [slots]
    const int32_t *__restrict__ counts;                 // [slots]
    const int32_t *__restrict__ flags;                  // [slots]
    const int32_t *__restrict__ tables;                 // [slots]
    int32_t *__restrict__ out_counts;                   // [slots]
    int64_t M, H, cap;                                  // max_frames_per_call, the bank's largest tap index, H + M
    int32_t T, slots;                                   // candidates in the bank
    __device__ VoiceAnswer advance(int64_t b) const
    {
        const VoiceSpan v = voice_span(pos[b], counts[b], flags[b], M, H);
        return {(int32_t)v.n_out, v.ok, v.next};
    }
};

// grid = (slots, max(1, ceil((M + H) / tile))); dynamic LDS = CX planes of k.W floats
template <int CX, int MODE, int R, bool EPI>
__global__ __launch_bounds__(kVpThreads) void voice_stream_kernel(const VoiceStreamArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float vs_lds[];
    constexpr int NT = kVpThreads, TILE = 2 * NT * R;
    const KArgs &k = a.k;
    const int64_t b = blockIdx.x;
    const VoiceSpan v = voice_span(uniform_i64(a.pos[b]), __builtin_amdgcn_readfirstlane(a.counts[b]),
                                   __builtin_amdgcn_readfirstlane(a.flags[b]), a.M, a.H);
    if (!v.ok) return;                                             // nothing is addressed with a bad count or position
    RingArgs r = ring_plan(v.p, v.n, a.H, v.end, a.cap);
    r.chunk = a.x + b * a.M * CX; r.ring = a.ring + b * a.cap * CX; r.Cx = CX;       // slot b's rows: stream 0 below
    ring_write<NT>(r, 0, blockIdx.y, gridDim.y, (int)threadIdx.x);
    const int64_t t0 = (int64_t)blockIdx.y * TILE;
    if (t0 >= v.n_out) return;                                     // (workgroup-uniform, before any barrier)
    float *dst = a.y + (b * (a.M + a.H) + t0) * 2;
    const v4i rdst = make_rsrc(dst, (v.n_out - t0) * 2 * 4);       // the rest of this slot's frames of this call
    const int shape = access_shape<2>(dst, 2);                     // workgroup-uniform
    each_tile<CX, MODE, R, EPI>(
        k, vs_lds, __builtin_amdgcn_readfirstlane(a.tables[b]), a.T,
        [&] { stream_stage<NT, CX>(r, vs_lds, 0, v.first_out + t0, 0, k.W, (int)threadIdx.x); },
        [&](int q, const float (&o)[4]) { store_result<2>(rdst, shape, k.stream_out, q, 1, 2, o); });
}

}  // namespace vnd

// ------------------------------------------------------------------------------
// C ABI (include/vnd_voice_stream.h)
// ------------------------------------------------------------------------------
typedef void (*voice_stream_kern_t)(const VoiceStreamArgs);

template <int CX, int MODE, bool EPI>
static voice_stream_kern_t voice_stream_by_r(int r)
{
    switch (r) {
    case 1: return voice_stream_kernel<CX, MODE, 1, EPI>;
    case 2: return voice_stream_kernel<CX, MODE, 2, EPI>;
    case 4: return voice_stream_kernel<CX, MODE, 4, EPI>;
    default: return nullptr;
    }
}

template <int CX>
static voice_stream_kern_t voice_stream_by_mode(const EachStreamPlan &p)
{
    if (p.epi) return p.fma ? voice_stream_by_r<CX, 1, true>(p.r) : voice_stream_by_r<CX, 0, true>(p.r);
    return p.fma ? voice_stream_by_r<CX, 1, false>(p.r) : voice_stream_by_r<CX, 0, false>(p.r);
}

// The tile of the pool: make_each_stream_plan's rule for a call of M output frames - what a slot in steady state
// returns - chosen once, and the tiles of the longest row a call can write, M + H.
static EachStreamPlan make_voice_stream_plan(const vnd_ctx *ctx, const vnd_taps *t, int64_t slots, int64_t M, int Cx, bool epi)
{
    EachStreamPlan p = make_each_stream_plan(ctx, t, slots, M, Cx, epi);
    const int64_t T = (int64_t)2 * kVpThreads * p.r, row = M + t->max_index;
    p.tiles = (int)std::max<int64_t>(1, (row + T - 1) / T);
    p.nblocks = (uint32_t)(slots * p.tiles);
    return p;
}

extern "C" {

static_assert((vnd::kVoiceMaxFrames + vnd::kVpMaxHalo) / (2 * vnd::kVpThreads) < 65535, "the tiles of the longest row fit a grid dimension");

vnd_status vnd_voice_stream_state_bytes(const vnd_taps *t, int64_t slots, int32_t in_channels, int64_t max_frames_per_call,
                                        int64_t *bytes)
{
    if (!t || !bytes) return fail(VND_ERR_INVALID, "null tap table or bytes");
    *bytes = 0;
    int64_t ring = 0;
    vnd_status st = vnd_each_stream_state_bytes(t, slots, in_channels, max_frames_per_call, &ring);
    if (st != VND_OK) return st;
    if (max_frames_per_call > kVoiceMaxFrames)
        return fail(VND_ERR_UNSUPPORTED, "max_frames_per_call %lld above 2^24: the tiles of a row are one grid dimension",
                    (long long)max_frames_per_call);
    *bytes = voice_position_bytes(slots) + ring;
    return VND_OK;
}

// The scalar side of the pool's checks, in the order the entries report them; *need = the bytes of its state.
static vnd_status voice_stream_scalars(const vnd_ctx *ctx, const vnd_taps *t, int64_t max_frames_per_call, int64_t slots,
                                       int32_t Cx, int32_t mode, int64_t *need)
{
    if (!ctx || !t) return fail(VND_ERR_INVALID, "null context or tap table");
    if (slots < 0) return fail(VND_ERR_INVALID, "negative slots");
    if (Cx != 1 && Cx != 2) return fail(VND_ERR_INVALID, "a pool of mono or stereo voices is taken, got %d channels", Cx);
    vnd_status st = each_bank_pairs(ctx, t);
    if (st != VND_OK) return st;
    if (max_frames_per_call < 0 || max_frames_per_call > ((int64_t)1 << 40))
        return fail(VND_ERR_INVALID, "max_frames_per_call %lld out of range", (long long)max_frames_per_call);
    if ((st = each_bank_limits(t, slots, mode, "voice", "slots", "stream it filter by filter")) != VND_OK) return st;
    return vnd_voice_stream_state_bytes(t, slots, Cx, max_frames_per_call, need);
}

static vnd_status voice_stream_rows(const vnd_taps *t, int64_t max_frames_per_call, int64_t slots)
{
    if (slots * (max_frames_per_call + t->max_index) * 2 > ((int64_t)1 << 40)) return fail(VND_ERR_UNSUPPORTED, "problem too large");
    return VND_OK;
}

// What the three entries check of the pool: scalars, the bank, the state.  Nothing is written.
static vnd_status voice_stream_pool(const vnd_ctx *ctx, const vnd_taps *t, const void *state, int64_t state_bytes,
                                    int64_t max_frames_per_call, int64_t slots, int32_t Cx, int32_t mode)
{
    int64_t need = 0;
    vnd_status st = voice_stream_scalars(ctx, t, max_frames_per_call, slots, Cx, mode, &need);
    if (st != VND_OK) return st;
    return voice_state_check("voice pool", state, state_bytes, need, slots);
}

vnd_status vnd_voice_stream_reset_dev(vnd_ctx *ctx, void *state, int64_t state_bytes, int64_t slots, int32_t Cx,
                                      const vnd_taps *t, int64_t max_frames_per_call, void *stream_)
{
    vnd_status st = voice_stream_pool(ctx, t, state, state_bytes, max_frames_per_call, slots, Cx, VND_MODE_EXACT);
    if (st != VND_OK) return st;
    return slots == 0 ? VND_OK : voice_reset_positions(ctx, state, slots, stream_);
}

static vnd_status voice_stream_check(const vnd_ctx *ctx, const vnd_taps *t, const void *state, int64_t state_bytes,
                                     int64_t max_frames_per_call, const float *x, const int32_t *counts, const int32_t *flags,
                                     const int32_t *tables, const float *y, const int32_t *out_counts, int64_t slots,
                                     int32_t Cx, int32_t mode)
{
    vnd_status st = voice_stream_pool(ctx, t, state, state_bytes, max_frames_per_call, slots, Cx, mode);
    if (st != VND_OK) return st;
    if (slots > 0 && (!counts || !flags || !tables || !out_counts || !y || (max_frames_per_call > 0 && !x)))
        return fail(VND_ERR_INVALID, "null chunk, counts, flags, table index, output or out_counts pointer");
    return voice_stream_rows(t, max_frames_per_call, slots);
}

vnd_status vnd_voice_stream_f32_dev(vnd_ctx *ctx, const vnd_taps *t, void *state, int64_t state_bytes,
                                    int64_t max_frames_per_call, const float *x, const int32_t *counts, const int32_t *flags,
                                    const int32_t *tables, float *y, int32_t *out_counts, int64_t slots, int32_t Cx,
                                    int32_t mode, int32_t ms_encode, int32_t use_width, double width, void *stream_)
{
    vnd_status st = voice_stream_check(ctx, t, state, state_bytes, max_frames_per_call, x, counts, flags, tables, y, out_counts,
                                       slots, Cx, mode);
    if (st != VND_OK) return st;
    if (slots == 0) return VND_OK;
    const bool epi = ms_encode || use_width;
    const EachStreamPlan p = make_voice_stream_plan(ctx, t, slots, max_frames_per_call, Cx, epi);
    VoiceStreamArgs a{};
    KArgs &k = a.k;
    table_args(k, t);
    k.C = t->C; k.Cx = Cx; k.W = p.W;
    k.epi_ms_encode = ms_encode ? 1 : 0; k.epi_use_width = use_width ? 1 : 0;
    k.epi_w_mid = (float)(1.0 - width); k.epi_w_side = (float)width;       // as the decorrelate stage passes the width
    a.x = x; a.y = y; a.counts = counts; a.flags = flags; a.tables = tables; a.out_counts = out_counts;
    a.pos = (int64_t *)state;
    a.ring = (float *)((char *)state + voice_position_bytes(slots));
    a.M = max_frames_per_call; a.H = t->max_index; a.cap = stream_capacity(t, max_frames_per_call);
    a.T = t->C / 2; a.slots = (int32_t)slots;
    DeviceScope on(ctx->device);
    if (!on.ok) return fail(VND_ERR_HIP, "cannot select device %d", ctx->device);
    voice_stream_kern_t kern = Cx == 2 ? voice_stream_by_mode<2>(p) : voice_stream_by_mode<1>(p);
    if (!kern) return fail(VND_ERR_UNSUPPORTED, "no stream kernel for this tile shape");
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(kern, dim3((unsigned)slots, (unsigned)p.tiles), dim3(kVpThreads), p.lds_bytes, stream, a);
    HIP_TRY(hipGetLastError());
    launch_voice_advance(a, slots, stream);
    HIP_TRY(hipGetLastError());
    return VND_OK;
}

vnd_status vnd_voice_stream_f32_host(vnd_ctx *ctx, const vnd_taps *t, void *state, int64_t state_bytes,
                                     int64_t max_frames_per_call, const float *x, const int32_t *counts, const int32_t *flags,
                                     const int32_t *tables, float *y, int32_t *out_counts, int64_t slots, int32_t Cx,
                                     int32_t mode, int32_t ms_encode, int32_t use_width, double width)
{
    vnd_status st = voice_stream_check(ctx, t, state, state_bytes, max_frames_per_call, x, counts, flags, tables, y, out_counts,
                                       slots, Cx, mode);
    if (st != VND_OK) return st;
    if (slots == 0) return VND_OK;
    const int32_t T = t->C / 2;
    for (int64_t b = 0; b < slots; ++b) {
        if (counts[b] < 0 || counts[b] > max_frames_per_call)
            return fail(VND_ERR_INVALID, "count %d of slot %lld is outside [0, %lld]", counts[b], (long long)b,
                        (long long)max_frames_per_call);
        if ((counts[b] > 0 || (flags[b] & VND_VOICE_END)) && (tables[b] < 0 || tables[b] >= T))
            return fail(VND_ERR_INVALID, "table %d of slot %lld is outside [0, %d)", tables[b], (long long)b, T);
    }
    const size_t x_bytes = (size_t)(slots * max_frames_per_call * Cx) * sizeof(float);
    const size_t y_bytes = (size_t)(slots * (max_frames_per_call + t->max_index) * 2) * sizeof(float);
    const size_t i_bytes = (size_t)slots * sizeof(int32_t);
    HostCall call(ctx);
    call.carve({y_bytes, x_bytes, i_bytes, i_bytes, i_bytes, i_bytes});
    float *y_dev = call.piece<float>(0), *x_dev = call.piece<float>(1);
    int32_t *c_dev = call.piece<int32_t>(2), *f_dev = call.piece<int32_t>(3), *t_dev = call.piece<int32_t>(4);
    int32_t *o_dev = call.piece<int32_t>(5);
    call.up(x_dev, x, x_bytes, "the chunk");
    call.up(y_dev, y, y_bytes, "y");                     // up and back whole: the rows at and past out_counts keep their bytes
    call.up(c_dev, counts, i_bytes, "counts");
    call.up(f_dev, flags, i_bytes, "flags");
    call.up(t_dev, tables, i_bytes, "tables");
    call.run([&] { return vnd_voice_stream_f32_dev(ctx, t, state, state_bytes, max_frames_per_call, x_dev, c_dev, f_dev, t_dev, y_dev, o_dev, slots, Cx, mode, ms_encode, use_width, width, call.stream()); });
    call.down(y, y_dev, y_bytes, "y");
    call.down(out_counts, o_dev, i_bytes, "out_counts");
    return call.finish("vnd_voice_stream_f32_host");
}

}  // extern "C"

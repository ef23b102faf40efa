// vnd_voice_fade_stream.hpp - a crossfading voice pool (include/vnd_voice_fade_stream.h): the voice pool of
// vnd_voice_stream.hpp whose live voices change their filter.  Beside its position a slot keeps one record (s, old, cur):
// the first frame of its latest fade, the table before it and the table after it.  A call with VND_VOICE_SWITCH that is
// accepted moves (old, cur, s) to (cur, tables[b], E): the fade begins at the first frame the slot has not yet returned,
// so nothing that was returned changes and nothing is returned twice.
//
// voice_fade_stream_kernel is voice_stream_kernel with the table of a tile chosen from the record.  Grid, slot-fast order,
// ring_plan / ring_write / stream_stage, the descriptor store and the plan (make_voice_stream_plan) are that kernel's.
// Per tile, workgroup-uniform:
//   - the tile lies wholly below s: each_tile with old;
//   - wholly at or past s + F: each_tile with cur - the steady state, and the instruction stream of voice_stream_kernel;
//   - otherwise fade_tile: the window is staged once, and per output channel vp_channel forms the lane's frames with old,
//     then with cur, and the two are blended in registers - old * gains[0][f - s] + cur * gains[1][f - s], two rounded
//     products and one rounded sum (-ffp-contract=off) - with the frames outside [s, s + F) selected from one side.  One
//     channel is finished before the next is formed, so the live frame pairs are each_tile's: 2 R plus vp_channel's R.
// each_tile itself is untouched, and so is every kernel of the existing pool.
//
// Every index that is built from device data, beyond vnd_voice_stream.hpp's list:
//   - the record: read whole, used only when the slot is not fresh - then an earlier call of this pool wrote it;
//   - gains: the index is f - s clamped into [0, F); nothing is read when F == 0;
//   - old, cur: bounds-checked against T (each_tile's check, and fade_tile's: NaN frames, nothing is indexed with a bad one);
//   - f - s: the tile's first frame less s is formed in int64; a tile that reaches fade_tile has it inside (-tile, F).
//
// voice_fade_advance_kernel, one lane per slot, follows on the same stream and writes pos, the record, out_counts and
// fade_left (vnd_voice_core.hpp, ORDERING: the kernel boundary orders every read of the slot's state before its update).
// Both kernels take everything from voice_fade_span.
#pragma once
#include "vnd_voice_stream.hpp"
#include "../../include/vnd_voice_fade_stream.h"

namespace vnd {

struct VoiceFadeRecord {
    int64_t s;                     // the first frame of the latest fade
    int32_t old, cur;              // the table before it and after it
};
static_assert(sizeof(VoiceFadeRecord) == 16, "one 16-byte record per slot");

struct VoiceFadeSpan {
    VoiceSpan v;                   // vnd_voice_stream.hpp's: p, n, first_out (E), n_out (E' - E), next, end, ok
    VoiceFadeRecord rec;           // the record the call's frames are formed with, and the slot keeps
    int32_t fade_left;             // frames of the fade not yet returned after the call; -1 for a bad slot
};

// One slot's side of a call (include/vnd_voice_fade_stream.h, "one call, per slot b"), from the stored position and record,
// counts[b], flags[b] and - read only for a fresh slot or an accepted switch - *table.
__host__ __device__ inline VoiceFadeSpan voice_fade_span(int64_t stored, VoiceFadeRecord rec, int32_t count, int32_t flags,
                                                         const int32_t *table, int64_t M, int64_t H, int64_t F)
{
    VoiceFadeSpan f{};
    f.v = voice_span(stored, count, flags, M, H);               // (a stored position of 0 is p = 0 with or without START)
    f.rec = rec;
    f.fade_left = -1;
    if (!f.v.ok) return f;
    const bool fresh = (flags & VND_VOICE_START) != 0 || stored == 0;
    const int64_t E = f.v.first_out, E1 = E + f.v.n_out;
    if (fresh) {
        const int32_t t = *table;
        f.rec = VoiceFadeRecord{-F, t, t};
    } else if ((flags & VND_VOICE_SWITCH) != 0 && E - F >= rec.s) {     // the previous fade has been returned whole
        f.rec = VoiceFadeRecord{E, rec.cur, *table};
    }
    const int64_t s = f.rec.s;                                  // min(F, max(0, s + F - E')), without a sum that could wrap
    f.fade_left = f.v.end ? 0 : (int32_t)(s >= E1 ? F : (s < E1 - F ? 0 : s + F - E1));
    return f;
}

struct VoiceFadeArgs {
    KArgs k;                                            // the bank's tables, k.C, k.Cx, k.W, k.epi_*; k.y and k.n are not read
    const float *__restrict__ x;                        // [slots][M][Cx]
    float *__restrict__ y;                              // [slots][M + H][2]
    float *__restrict__ ring;                           // [slots][cap][Cx]
    int64_t *__restrict__ pos;                          // [slots]
    VoiceFadeRecord *__restrict__ rec;                  // [slots]
    const float *__restrict__ gains;                    // [2][F]; null with F == 0
    const int32_t *__restrict__ counts;                 // [slots]
    const int32_t *__restrict__ flags;                  // [slots]
    const int32_t *__restrict__ tables;                 // [slots]
    int32_t *__restrict__ out_counts;                   // [slots]
    int32_t *__restrict__ fade_left;                    // [slots], or null
    int64_t M, H, cap, F;                               // max_frames_per_call, the bank's largest tap index, H + M, fade_frames
    int32_t T, slots;                                   // candidates in the bank
};

// The sibling of each_tile (vnd_each.hpp) for a tile that holds frames of a fade: frame 2q + e of the tile is frame
// rel0 + 2q + e of the fade, below 0 before it and from F on behind it.  old, cur and rel0 are workgroup-uniform; a table
// outside [0, T) gives NaN frames wherever it enters.
template <int CX, int MODE, int R, bool EPI, typename Stage, typename Store>
__device__ __forceinline__ void fade_tile(const KArgs &k, const float *lds, int32_t old, int32_t cur, int32_t T, int32_t rel0,
                                          int32_t F, const float *__restrict__ gains, Stage stage, Store store)
{
    const int tid = threadIdx.x;
    const bool old_ok = old >= 0 && old < T, cur_ok = cur >= 0 && cur < T;
    const float nan = __builtin_nanf("");
    stage();
    __syncthreads();
    const float *right = lds + (CX == 2 ? k.W : 0);
    v2f out[2][R];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const float *pa = (c ? right : lds) + 2 * tid;
        v2f in[R];
        if (old_ok) vp_channel<MODE, R>(k, 2 * old + c, pa, out[c]);
        else {
#pragma unroll
            for (int j = 0; j < R; ++j) out[c][j] = v2f{nan, nan};
        }
        if (cur_ok) vp_channel<MODE, R>(k, 2 * cur + c, pa, in);
        else {
#pragma unroll
            for (int j = 0; j < R; ++j) in[j] = v2f{nan, nan};
        }
#pragma unroll
        for (int j = 0; j < R; ++j) {
            const int rel = rel0 + 2 * (tid + kVpThreads * j);
            float o[2] = {out[c][j].x, out[c][j].y};
            const float n[2] = {in[j].x, in[j].y};
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int at = rel + e;
                float blend = n[e];
                if (F > 0) {
                    const int i = at < 0 ? 0 : (at >= F ? F - 1 : at);
                    blend = o[e] * gains[i] + n[e] * gains[F + i];
                }
                o[e] = at < 0 ? o[e] : (at >= F ? n[e] : blend);
            }
            out[c][j] = v2f{o[0], o[1]};
        }
    }
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const int q = tid + kVpThreads * j;
        float v[4] = {out[0][j].x, out[1][j].x, out[0][j].y, out[1][j].y};
        if constexpr (EPI) {
            const float2 x0 = *(const float2 *)(lds + 2 * q), x1 = *(const float2 *)(right + 2 * q);
            const float xin[4] = {x0.x, x1.x, x0.y, x1.y};
            epi_pointwise(k, v, xin);
        }
        store(q, v);
    }
}

// grid = (slots, max(1, ceil((M + H) / tile))); dynamic LDS = CX planes of k.W floats
template <int CX, int MODE, int R, bool EPI>
__global__ __launch_bounds__(kVpThreads) void voice_fade_stream_kernel(const VoiceFadeArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float vf_lds[];
    constexpr int NT = kVpThreads, TILE = 2 * NT * R;
    const KArgs &k = a.k;
    const int64_t b = blockIdx.x;
    const VoiceFadeRecord stored = a.rec[b];
    const VoiceFadeSpan f = voice_fade_span(
        uniform_i64(a.pos[b]),
        VoiceFadeRecord{uniform_i64(stored.s), __builtin_amdgcn_readfirstlane(stored.old), __builtin_amdgcn_readfirstlane(stored.cur)},
        __builtin_amdgcn_readfirstlane(a.counts[b]), __builtin_amdgcn_readfirstlane(a.flags[b]), a.tables + b, a.M, a.H, a.F);
    const VoiceSpan &v = f.v;
    if (!v.ok) return;                                             // nothing is addressed with a bad count or position
    RingArgs r = ring_plan(v.p, v.n, a.H, v.end, a.cap);
    r.chunk = a.x + b * a.M * CX; r.ring = a.ring + b * a.cap * CX; r.Cx = CX;       // slot b's rows: stream 0 below
    ring_write<NT>(r, 0, blockIdx.y, gridDim.y, (int)threadIdx.x);
    const int64_t t0 = (int64_t)blockIdx.y * TILE;
    if (t0 >= v.n_out) return;                                     // (workgroup-uniform, before any barrier)
    const int32_t old = __builtin_amdgcn_readfirstlane(f.rec.old), cur = __builtin_amdgcn_readfirstlane(f.rec.cur);
    const int64_t left = v.n_out - t0;
    const int64_t rel = v.first_out + t0 - uniform_i64(f.rec.s);  // the tile's first frame, counted from the fade's first
    const int64_t frames = left < TILE ? left : TILE;
    float *dst = a.y + (b * (a.M + a.H) + t0) * 2;
    const v4i rdst = make_rsrc(dst, left * 2 * 4);                 // the rest of this slot's frames of this call
    const int shape = access_shape<2>(dst, 2);                     // workgroup-uniform
    auto stage = [&] { stream_stage<NT, CX>(r, vf_lds, 0, v.first_out + t0, 0, k.W, (int)threadIdx.x); };
    auto store = [&](int q, const float (&o)[4]) { store_result<2>(rdst, shape, k.stream_out, q, 1, 2, o); };
    if (rel + frames <= 0 || rel >= a.F) {                         // one table: wholly below s, or at or past s + F
        each_tile<CX, MODE, R, EPI>(k, vf_lds, rel >= a.F ? cur : old, a.T, stage, store);
        return;
    }
    // here -TILE < rel < F <= 2^20: the int64 difference fits the int32 a lane adds its frame to
    fade_tile<CX, MODE, R, EPI>(k, vf_lds, old, cur, a.T, (int32_t)rel, (int32_t)a.F, a.gains, stage, store);
}

// grid = ceil(slots / kVoiceAdvanceThreads), one lane per slot: behind voice_fade_stream_kernel on the same stream
__global__ __launch_bounds__(kVoiceAdvanceThreads) void voice_fade_advance_kernel(const VoiceFadeArgs a)
{
    const int64_t b = (int64_t)blockIdx.x * kVoiceAdvanceThreads + threadIdx.x;
    if (b >= a.slots) return;
    const VoiceFadeSpan f = voice_fade_span(a.pos[b], a.rec[b], a.counts[b], a.flags[b], a.tables + b, a.M, a.H, a.F);
    a.out_counts[b] = (int32_t)f.v.n_out;
    if (a.fade_left) a.fade_left[b] = f.fade_left;
    if (!f.v.ok) return;                                           // nothing of a bad slot changes
    a.pos[b] = f.v.next;
    a.rec[b] = f.rec;
}

}  // namespace vnd

// ------------------------------------------------------------------------------
// C ABI (include/vnd_voice_fade_stream.h)
// ------------------------------------------------------------------------------
typedef void (*voice_fade_kern_t)(const VoiceFadeArgs);

template <int CX, int MODE, bool EPI>
static voice_fade_kern_t voice_fade_by_r(int r)
{
    switch (r) {
    case 1: return voice_fade_stream_kernel<CX, MODE, 1, EPI>;
    case 2: return voice_fade_stream_kernel<CX, MODE, 2, EPI>;
    case 4: return voice_fade_stream_kernel<CX, MODE, 4, EPI>;
    default: return nullptr;
    }
}

template <int CX>
static voice_fade_kern_t voice_fade_by_mode(const EachStreamPlan &p)
{
    if (p.epi) return p.fma ? voice_fade_by_r<CX, 1, true>(p.r) : voice_fade_by_r<CX, 0, true>(p.r);
    return p.fma ? voice_fade_by_r<CX, 1, false>(p.r) : voice_fade_by_r<CX, 0, false>(p.r);
}

static int64_t voice_fade_record_bytes(int64_t slots) { return slots * (int64_t)sizeof(vnd::VoiceFadeRecord); }

// fade_frames against the header's range, behind the pool's own scalar checks
static vnd_status voice_fade_frames_check(int64_t fade_frames)
{
    if (fade_frames < 0) return fail(VND_ERR_INVALID, "negative fade_frames");
    if (fade_frames > VND_VOICE_FADE_MAX_FRAMES)
        return fail(VND_ERR_UNSUPPORTED, "fade_frames %lld above %d", (long long)fade_frames, VND_VOICE_FADE_MAX_FRAMES);
    return VND_OK;
}

// The scalar side of the pool's checks: vnd_voice_stream.hpp's, then fade_frames; *need = the bytes of its state.
static vnd_status voice_fade_scalars(const vnd_ctx *ctx, const vnd_taps *t, int64_t max_frames_per_call, int64_t fade_frames,
                                     int64_t slots, int32_t Cx, int32_t mode, int64_t *need)
{
    int64_t plain = 0;
    vnd_status st = voice_stream_scalars(ctx, t, max_frames_per_call, slots, Cx, mode, &plain);
    if (st != VND_OK) return st;
    if ((st = voice_fade_frames_check(fade_frames)) != VND_OK) return st;
    *need = plain + voice_fade_record_bytes(slots);
    return VND_OK;
}

extern "C" {

vnd_status vnd_voice_fade_stream_state_bytes(const vnd_taps *t, int64_t slots, int32_t in_channels, int64_t max_frames_per_call,
                                             int64_t fade_frames, int64_t *bytes)
{
    if (!t || !bytes) return fail(VND_ERR_INVALID, "null tap table or bytes");
    *bytes = 0;
    int64_t plain = 0;
    vnd_status st = vnd_voice_stream_state_bytes(t, slots, in_channels, max_frames_per_call, &plain);
    if (st != VND_OK) return st;
    if ((st = voice_fade_frames_check(fade_frames)) != VND_OK) return st;
    *bytes = plain + voice_fade_record_bytes(slots);
    return VND_OK;
}

// What the entries check of the pool: scalars, the bank, fade_frames, the state.  Nothing is written.
static vnd_status voice_fade_pool(const vnd_ctx *ctx, const vnd_taps *t, const void *state, int64_t state_bytes,
                                  int64_t max_frames_per_call, int64_t fade_frames, int64_t slots, int32_t Cx, int32_t mode)
{
    int64_t need = 0;
    vnd_status st = voice_fade_scalars(ctx, t, max_frames_per_call, fade_frames, slots, Cx, mode, &need);
    if (st != VND_OK) return st;
    return voice_state_check("crossfading voice pool", state, state_bytes, need, slots);
}

vnd_status vnd_voice_fade_stream_reset_dev(vnd_ctx *ctx, void *state, int64_t state_bytes, int64_t slots, int32_t Cx,
                                           const vnd_taps *t, int64_t max_frames_per_call, int64_t fade_frames, void *stream_)
{
    vnd_status st = voice_fade_pool(ctx, t, state, state_bytes, max_frames_per_call, fade_frames, slots, Cx, VND_MODE_EXACT);
    if (st != VND_OK) return st;
    return slots == 0 ? VND_OK : voice_reset_positions(ctx, state, slots, stream_);
}

vnd_status vnd_voice_fade_stream_f32_dev(vnd_ctx *ctx, const vnd_taps *t, void *state, int64_t state_bytes,
                                         int64_t max_frames_per_call, int64_t fade_frames, const float *gains, const float *x,
                                         const int32_t *counts, const int32_t *flags, const int32_t *tables, float *y,
                                         int32_t *out_counts, int32_t *fade_left, int64_t slots, int32_t Cx, int32_t mode,
                                         int32_t ms_encode, int32_t use_width, double width, void *stream_)
{
    vnd_status st = voice_fade_pool(ctx, t, state, state_bytes, max_frames_per_call, fade_frames, slots, Cx, mode);
    if (st != VND_OK) return st;
    if (slots > 0 && (!counts || !flags || !tables || !out_counts || !y || (max_frames_per_call > 0 && !x)))
        return fail(VND_ERR_INVALID, "null chunk, counts, flags, table index, output or out_counts pointer");
    if (fade_frames > 0 && !gains) return fail(VND_ERR_INVALID, "null gains with fade_frames %lld", (long long)fade_frames);
    if ((st = voice_stream_rows(t, max_frames_per_call, slots)) != VND_OK) return st;
    if (slots == 0) return VND_OK;
    const bool epi = ms_encode || use_width;
    const EachStreamPlan p = make_voice_stream_plan(ctx, t, slots, max_frames_per_call, Cx, epi);
    VoiceFadeArgs a{};
    KArgs &k = a.k;
    table_args(k, t);
    k.C = t->C; k.Cx = Cx; k.W = p.W;
    k.epi_ms_encode = ms_encode ? 1 : 0; k.epi_use_width = use_width ? 1 : 0;
    k.epi_w_mid = (float)(1.0 - width); k.epi_w_side = (float)width;       // as the decorrelate stage passes the width
    a.x = x; a.y = y; a.counts = counts; a.flags = flags; a.tables = tables; a.out_counts = out_counts;
    a.fade_left = fade_left; a.gains = gains;
    a.pos = (int64_t *)state;
    a.rec = (VoiceFadeRecord *)((char *)state + voice_position_bytes(slots));
    a.ring = (float *)((char *)state + voice_position_bytes(slots) + voice_fade_record_bytes(slots));
    a.M = max_frames_per_call; a.H = t->max_index; a.cap = stream_capacity(t, max_frames_per_call); a.F = fade_frames;
    a.T = t->C / 2; a.slots = (int32_t)slots;
    DeviceScope on(ctx->device);
    if (!on.ok) return fail(VND_ERR_HIP, "cannot select device %d", ctx->device);
    voice_fade_kern_t kern = Cx == 2 ? voice_fade_by_mode<2>(p) : voice_fade_by_mode<1>(p);
    if (!kern) return fail(VND_ERR_UNSUPPORTED, "no stream kernel for this tile shape");
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(kern, dim3((unsigned)slots, (unsigned)p.tiles), dim3(kVpThreads), p.lds_bytes, stream, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(voice_fade_advance_kernel, dim3((unsigned)voice_advance_groups(slots)), dim3(kVoiceAdvanceThreads), 0,
                       stream, a);
    HIP_TRY(hipGetLastError());
    return VND_OK;
}

}  // extern "C"

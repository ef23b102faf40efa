// vnd_haas_voice_fade_stream.hpp - a crossfading voice pool of HaasEffect delays (include/vnd_haas_voice_fade_stream.h): the
// Haas voice pool of vnd_haas_voice_stream.hpp whose live voices change their delay.  Beside its position a slot keeps one
// record (s, old, cur): the first frame of its latest fade, the delay before it and the delay after it.  A call with
// VND_VOICE_SWITCH that is accepted moves (old, cur, s) to (cur, delays[b], p): the delay is causal, so the first frame the
// slot has not yet returned is its position, and nothing that was returned changes.
//
// haas_voice_fade_stream_kernel is haas_voice_stream_kernel with the delay of a lane chosen from the record.  Grid
// (slots, ceil((M + max_delay) / 256)), slot-fast order, ring_plan / ring_write / haas_stream_frame and one lane per output
// frame are that kernel's.  Per lane, with t its absolute frame:
//   - t < s: the delayed column is read at t - old;  t >= s + F: at t - cur - the steady state, and the instruction
//     sequence of haas_voice_stream_kernel with the selected delay;
//   - otherwise the lane makes a second haas_stream_frame / haas_column_of at t - old and blends the two columns in
//     float64 - old * (double)gains[0][t - s] + cur * (double)gains[1][t - s], two rounded products and one rounded sum
//     (-ffp-contract=off) - before haas_frame decodes the pair.
// haas_voice_stream_kernel itself is untouched.
//
// Every index that is built from device data, beyond vnd_haas_voice_stream.hpp's list:
//   - the record: read whole, used only when the slot is not fresh; a slot with work whose stored old or cur lies outside
//     [0, max_delay] is a bad slot and the workgroup leaves before anything is addressed with either;
//   - delays[b]: read when the slot is fresh with work or its switch is accepted, and checked against [0, max_delay] before
//     it enters the record: so 0 <= old, cur <= max_delay on every lane that reaches a frame;
//   - t - s: s is compared first (t < s), then the difference is formed as uint64, exact for t >= s whatever s holds, and
//     compared with F: a lane indexes gains only with 0 <= t - s < F, and nothing is read when F == 0;
//   - t - old and t - cur: both in [p - max_delay, p + n_out): below p the ring holds [p - max_delay, p)
//     (haas_stream_frame's own range check answers frames below 0 and at or past p + n with zeros, nothing is loaded);
//   - y: frame k < n_out = n + tail <= M + max(old, cur) <= M + max_delay = the row.
//
// haas_voice_fade_advance_kernel, one lane per slot, follows on the same stream and writes pos, the record, out_counts and
// fade_left (vnd_voice_core.hpp, ORDERING: the kernel boundary orders every read of the slot's state before its update).
// Both kernels take everything from haas_voice_fade_span.
#pragma once
#include "vnd_haas_voice_stream.hpp"
#include "vnd_voice_fade_stream.hpp"
#include "../../include/vnd_haas_voice_fade_stream.h"

namespace vnd {

struct HaasVoiceFadeRecord {
    int64_t s;                     // the first frame of the latest fade
    int32_t old, cur;              // the delay before it and after it, in frames
};
static_assert(sizeof(HaasVoiceFadeRecord) == 16, "one 16-byte record per slot");

struct HaasVoiceFadeSpan {
    int64_t p, n;                  // position the call starts at, frames pushed
    int64_t n_out;                 // n, and the tail with END; -1 for a bad slot
    int64_t next;                  // the position after the call
    HaasVoiceFadeRecord rec;       // the record the call's frames are formed with, and the slot keeps
    int32_t fade_left;             // frames of the fade not yet returned after the call; -1 for a bad slot
    bool end, ok, work;            // !ok: the slot is left alone; !work: an idle slot, nothing of it changes
};

// One slot's side of a call (include/vnd_haas_voice_fade_stream.h, "one call, per slot b"), from the stored position and
// record, counts[b], flags[b] and - read only for a fresh slot with work or an accepted switch - *delay.
__host__ __device__ inline HaasVoiceFadeSpan haas_voice_fade_span(int64_t stored, HaasVoiceFadeRecord rec, int32_t count,
                                                                  int32_t flags, const int32_t *delay, int64_t M,
                                                                  int32_t max_delay, int64_t F)
{
    const VoiceSpan h = voice_span(stored, count, flags, M, 0);   // H = 0, as haas_voice_span: p, n, next, end, ok
    HaasVoiceFadeSpan f{};
    f.rec = rec; f.next = stored; f.n_out = -1; f.fade_left = -1; f.end = h.end;
    if (!h.ok) return f;                                        // (ok and work are false, p = n = 0)
    const bool fresh = (flags & VND_VOICE_START) != 0 || stored == 0;
    f.work = count > 0 || (flags & (VND_VOICE_START | VND_VOICE_END | VND_VOICE_SWITCH)) != 0;
    if (fresh) {
        if (!f.work) {                                          // idle at position 0: no record to read, no fade
            f.ok = true; f.n_out = 0; f.fade_left = 0;
            return f;
        }
        const int32_t d = *delay;
        if (d < 0 || d > max_delay) return f;
        f.rec = HaasVoiceFadeRecord{-F, d, d};
    } else if (f.work) {
        if (rec.old < 0 || rec.old > max_delay || rec.cur < 0 || rec.cur > max_delay) return f;
        if ((flags & VND_VOICE_SWITCH) != 0 && h.p - F >= rec.s) {           // p >= s + F: the previous fade is through
            const int32_t d = *delay;
            if (d < 0 || d > max_delay) return f;
            f.rec = HaasVoiceFadeRecord{h.p, rec.cur, d};
        }
    }
    f.ok = true; f.p = h.p; f.n = h.n; f.next = h.next;
    const int64_t e = h.p + h.n, s = f.rec.s;
    // min(F, max(0, s + F - e)) and min(old, max(0, s + F - e)), without a sum that a planted s could wrap
    const int64_t left = s >= e ? F : (s < e - F ? 0 : s + F - e);
    f.fade_left = h.end ? 0 : (int32_t)left;
    f.n_out = h.n;
    if (h.end) {                                                // tail = max(cur, min(old, max(0, s + F - e)))
        const int64_t old = f.rec.old, cur = f.rec.cur;
        const int64_t reach = s >= e ? (s - e >= old ? old : (s - e + F < old ? s - e + F : old)) : (left < old ? left : old);
        f.n_out += cur > reach ? cur : reach;
    }
    return f;
}

struct HaasVoiceFadeArgs {
    HArgs h;                                            // Cx, delayed_channel, ms, use_width, w_mid, w_side
    const float *__restrict__ x;                        // [slots][M][Cx]
    double *__restrict__ y;                             // [slots][M + max_delay][2]
    float *__restrict__ ring;                           // [slots][cap][Cx]
    int64_t *__restrict__ pos;                          // [slots]
    HaasVoiceFadeRecord *__restrict__ rec;              // [slots]
    const float *__restrict__ gains;                    // [2][F]; null with F == 0
    const int32_t *__restrict__ counts;                 // [slots]
    const int32_t *__restrict__ flags;                  // [slots]
    const int32_t *__restrict__ delays;                 // [slots]
    int32_t *__restrict__ out_counts;                   // [slots]
    int32_t *__restrict__ fade_left;                    // [slots], or null
    int64_t M, cap, F;                                  // max_frames_per_call, max_delay + M, fade_frames
    int32_t max_delay, slots;
};

// grid = (slots, max(1, ceil((M + max_delay) / kHaasStreamThreads))): one lane per output frame of the longest row
__global__ __launch_bounds__(kHaasStreamThreads) void haas_voice_fade_stream_kernel(const HaasVoiceFadeArgs a)
{
    const int64_t b = blockIdx.x;
    const int tid = threadIdx.x;
    const HaasVoiceFadeRecord stored = a.rec[b];
    const HaasVoiceFadeSpan v = haas_voice_fade_span(
        uniform_i64(a.pos[b]),
        HaasVoiceFadeRecord{uniform_i64(stored.s), __builtin_amdgcn_readfirstlane(stored.old), __builtin_amdgcn_readfirstlane(stored.cur)},
        __builtin_amdgcn_readfirstlane(a.counts[b]), __builtin_amdgcn_readfirstlane(a.flags[b]), a.delays + b, a.M, a.max_delay,
        a.F);
    if (!v.ok || !v.work) return;                                  // a bad slot: nothing is addressed; an idle one: nothing to do
    const int Cx = a.h.Cx;
    HaasStreamArgs s{};
    s.h = a.h;
    s.r = ring_plan(v.p, v.n, a.max_delay, v.end, a.cap);
    s.r.chunk = a.x + b * a.M * Cx; s.r.ring = a.ring + b * a.cap * Cx; s.r.Cx = Cx;   // slot b's rows: stream 0 below
    s.ring_first = v.p - a.max_delay;
    s.ring_slot0 = s.r.wr_slot0 - (s.r.wr_first - s.ring_first);   // in [-cap, cap): vnd_haas_voice_stream.hpp
    if (s.ring_slot0 < 0) s.ring_slot0 += a.cap;
    ring_write<kHaasStreamThreads>(s.r, 0, blockIdx.y, gridDim.y, tid);
    const int64_t k = (int64_t)blockIdx.y * kHaasStreamThreads + tid;
    if (k >= v.n_out) return;
    const int64_t t = v.p + k;
    const int64_t fs = uniform_i64(v.rec.s);
    const int32_t old = __builtin_amdgcn_readfirstlane(v.rec.old), cur = __builtin_amdgcn_readfirstlane(v.rec.cur);
    const uint64_t rel = (uint64_t)t - (uint64_t)fs;               // exact where it is used: t >= s
    const bool blend = t >= fs && rel < (uint64_t)a.F;             // inside [s, s + F)
    const int64_t d = t < fs ? old : cur;
    double c[2], o[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        double l = 0.0, r = 0.0;
        const bool in = haas_stream_frame(s, 0, j == s.h.delayed_channel ? t - d : t, l, r);
        c[j] = in ? haas_column_of(s.h, j, l, r) : 0.0;                                   // np.roll: zeros wrap in
    }
    if (blend) {                                                   // c[delayed] is D_cur[t]: the other delay's column, then the blend
        const int j = s.h.delayed_channel;
        double l = 0.0, r = 0.0;
        const bool in = haas_stream_frame(s, 0, t - old, l, r);
        const double was = in ? haas_column_of(s.h, j, l, r) : 0.0;
        const double g0 = (double)a.gains[rel], g1 = (double)a.gains[a.F + (int64_t)rel];
        const double fall = was * g0, rise = c[j] * g1;
        c[j] = fall + rise;
    }
    haas_frame(s.h, c[0], c[1], o);
    *(double2 *)(a.y + (b * (a.M + a.max_delay) + k) * 2) = make_double2(o[0], o[1]);
}

// grid = ceil(slots / kVoiceAdvanceThreads), one lane per slot: behind haas_voice_fade_stream_kernel on the same stream
__global__ __launch_bounds__(kVoiceAdvanceThreads) void haas_voice_fade_advance_kernel(const HaasVoiceFadeArgs a)
{
    const int64_t b = (int64_t)blockIdx.x * kVoiceAdvanceThreads + threadIdx.x;
    if (b >= a.slots) return;
    const HaasVoiceFadeSpan v = haas_voice_fade_span(a.pos[b], a.rec[b], a.counts[b], a.flags[b], a.delays + b, a.M, a.max_delay,
                                                     a.F);
    a.out_counts[b] = (int32_t)v.n_out;
    if (a.fade_left) a.fade_left[b] = v.fade_left;
    if (!v.ok || !v.work) return;                                  // nothing of a bad slot changes, nor of an idle one
    a.pos[b] = v.next;
    a.rec[b] = v.rec;
}

}  // namespace vnd

// ------------------------------------------------------------------------------
// C ABI (include/vnd_haas_voice_fade_stream.h)
// ------------------------------------------------------------------------------
static int64_t haas_voice_fade_record_bytes(int64_t slots) { return slots * (int64_t)sizeof(vnd::HaasVoiceFadeRecord); }

extern "C" {

vnd_status vnd_haas_voice_fade_stream_state_bytes(int64_t slots, int32_t in_channels, int32_t max_delay,
                                                  int64_t max_frames_per_call, int64_t fade_frames, int64_t *bytes)
{
    if (!bytes) return fail(VND_ERR_INVALID, "null bytes");
    *bytes = 0;
    int64_t plain = 0;
    vnd_status st = vnd_haas_voice_stream_state_bytes(slots, in_channels, max_delay, max_frames_per_call, &plain);
    if (st != VND_OK) return st;
    if ((st = voice_fade_frames_check(fade_frames)) != VND_OK) return st;
    *bytes = plain + haas_voice_fade_record_bytes(slots);
    return VND_OK;
}

// What the entries check of the pool: scalars, fade_frames, the state.  Nothing is written.
static vnd_status haas_voice_fade_pool(const vnd_ctx *ctx, const void *state, int64_t state_bytes, int64_t max_frames_per_call,
                                       int64_t fade_frames, int64_t slots, int32_t Cx, int32_t max_delay)
{
    if (!ctx) return fail(VND_ERR_INVALID, "null context");
    int64_t need = 0;
    vnd_status st = vnd_haas_voice_fade_stream_state_bytes(slots, Cx, max_delay, max_frames_per_call, fade_frames, &need);
    if (st != VND_OK) return st;
    return voice_state_check("crossfading Haas voice pool", state, state_bytes, need, slots);
}

vnd_status vnd_haas_voice_fade_stream_reset_dev(vnd_ctx *ctx, void *state, int64_t state_bytes, int64_t slots, int32_t Cx,
                                                int32_t max_delay, int64_t max_frames_per_call, int64_t fade_frames,
                                                void *stream_)
{
    vnd_status st = haas_voice_fade_pool(ctx, state, state_bytes, max_frames_per_call, fade_frames, slots, Cx, max_delay);
    if (st != VND_OK) return st;
    return slots == 0 ? VND_OK : voice_reset_positions(ctx, state, slots, stream_);
}

vnd_status vnd_haas_voice_fade_stream_f64_dev(vnd_ctx *ctx, void *state, int64_t state_bytes, int64_t max_frames_per_call,
                                              int64_t fade_frames, const float *gains, const float *x, const int32_t *counts,
                                              const int32_t *flags, const int32_t *delays, double *y, int32_t *out_counts,
                                              int32_t *fade_left, int64_t slots, int32_t Cx, int32_t max_delay,
                                              int32_t delayed_channel, int32_t ms_mode, int32_t use_width, double width,
                                              void *stream_)
{
    vnd_status st = haas_voice_fade_pool(ctx, state, state_bytes, max_frames_per_call, fade_frames, slots, Cx, max_delay);
    if (st != VND_OK) return st;
    if (delayed_channel != 0 && delayed_channel != 1)
        return fail(VND_ERR_INVALID, "delayed_channel must be 0 or 1, got %d", delayed_channel);
    if (slots > 0 && (!counts || !flags || !delays || !out_counts || !y || (max_frames_per_call > 0 && !x)))
        return fail(VND_ERR_INVALID, "null chunk, counts, flags, delays, output or out_counts pointer");
    if (fade_frames > 0 && !gains) return fail(VND_ERR_INVALID, "null gains with fade_frames %lld", (long long)fade_frames);
    if (slots * (max_frames_per_call + max_delay) * 2 > ((int64_t)1 << 40)) return fail(VND_ERR_UNSUPPORTED, "problem too large");
    if (slots == 0) return VND_OK;
    HaasVoiceFadeArgs a{};
    a.h.Cx = Cx; a.h.delayed_channel = delayed_channel;
    a.h.ms = ms_mode ? 1 : 0; a.h.use_width = use_width ? 1 : 0; a.h.w_mid = 1.0 - width; a.h.w_side = width;
    a.x = x; a.y = y; a.counts = counts; a.flags = flags; a.delays = delays; a.out_counts = out_counts;
    a.fade_left = fade_left; a.gains = gains;
    a.pos = (int64_t *)state;
    a.rec = (HaasVoiceFadeRecord *)((char *)state + voice_position_bytes(slots));
    a.ring = (float *)((char *)state + voice_position_bytes(slots) + haas_voice_fade_record_bytes(slots));
    a.M = max_frames_per_call; a.max_delay = max_delay; a.cap = (int64_t)max_delay + max_frames_per_call; a.F = fade_frames;
    a.slots = (int32_t)slots;
    const int64_t row = max_frames_per_call + max_delay;
    const unsigned tiles = (unsigned)std::max<int64_t>(1, (row + kHaasStreamThreads - 1) / kHaasStreamThreads);
    DeviceScope on(ctx->device);
    if (!on.ok) return fail(VND_ERR_HIP, "cannot select device %d", ctx->device);
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(haas_voice_fade_stream_kernel, dim3((unsigned)slots, tiles), dim3(kHaasStreamThreads), 0, stream, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(haas_voice_fade_advance_kernel, dim3((unsigned)voice_advance_groups(slots)), dim3(kVoiceAdvanceThreads),
                       0, stream, a);
    HIP_TRY(hipGetLastError());
    return VND_OK;
}

}  // extern "C"

// vnd_haas_voice_stream.hpp - a voice pool of HaasEffect delays (include/vnd_haas_voice_stream.h): the per-stream Haas
// block stream of vnd_haas_stream.hpp with the stream position moved from the caller into the device state, one per slot,
// and a frame count, start / end flags and a delay per slot and call - the Haas sibling of vnd_voice_stream.hpp.  A call
// is a pure function of device memory: it can be captured in a graph and replayed.
//
// haas_voice_stream_kernel is the sibling of haas_stream_kernel<EACH>: one lane per output frame, 256 lanes per workgroup.
// Its grid is fixed by the pool - (slots, ceil((M + max_delay) / 256)), the longest row a call can write - and not by the
// call, and the SLOT is the fast dimension, for the reason vnd_voice_stream.hpp gives: in steady state only the first
// tiles of a row have frames, and with the tile as the fast dimension the working workgroups land on few XCDs.  A
// workgroup reads pos[b], counts[b], flags[b] and delays[b] of its slot once, workgroup-uniform, and derives from them
// what the host derives for the lockstep stream: the span (haas_voice_span: voice_span with H = 0, then the voice's own
// tail) and the ring side of the call (ring_plan, the host's own function, reach = max_delay).  It then builds a
// HaasStreamArgs whose chunk and ring pointers are offset to slot b, so ring_write and haas_stream_frame are called
// unchanged with stream 0, and each frame is haas_column_of / haas_frame of vnd_haas.hpp on the same float32 samples:
// the float64 operation sequence of haas_stream_kernel and the one-shot kernels, which depends neither on the tile nor on
// the call, so a voice's concatenated outputs are vnd_haas_f64_*'s bit for bit, whatever its neighbours do.
//
// THE RING, per slot, with H = max_delay and cap = max_delay + M (the contract of vnd_stream.hpp's RingArgs): a call at
// position p reads ring frames in [p - d, p), inside [p - max_delay, p), and writes the chunk's last min(n, max_delay)
// frames, inside [p, p + n).  A read frame f and a written frame g have 0 < g - f <= max_delay + n - 1 < cap: they never
// share a slot, no ordering between a call's workgroups is needed, and every frame is written once.  Every earlier call
// of the voice kept its last min(n, max_delay) frames, so [max(0, p - max_delay), p) is there whatever the block sizes
// were; a frame below 0 is never loaded, so the ring needs no clearing when a slot changes hands.
//
// Every index that is built from device data:
//   - counts[b] outside [0, M]: the workgroup leaves before anything is addressed with it;
//   - pos[b] outside [0, 2^60] (a state that was never reset) without START: the same - so p >= 0 below;
//   - delays[b] outside [0, max_delay] on a slot with work: the same; on an idle slot (n = 0, no flag) it is not looked
//     at: that slot has n_out = 0 and writes nothing to the ring, so no lane reaches a frame;
//   - chunk frames: ring_write reads [wr_first - p, n) of the slot's row of x, haas_stream_frame [0, n): inside [0, M);
//   - ring slots: wr_slot0 = wr_first % cap lies in [0, cap) and is walked forward with one wrap; ring_slot0 is the slot
//     of p - max_delay, wr_slot0 less (wr_first - (p - max_delay)) = max(n, max_delay) (n + max_delay on END), which is
//     in [0, cap], plus cap if that is below 0: in [0, cap) - no second modulo; haas_stream_frame walks it forward by
//     less than max_delay <= cap with one wrap;
//   - y: frame k < n_out <= M + max_delay = the row.
//
// voice_advance_kernel<HaasVoiceArgs>, one lane per slot, follows on the same stream and writes pos[b] and out_counts[b]
// (vnd_voice_core.hpp).
#pragma once
#include "vnd_haas_stream.hpp"
#include "vnd_voice_stream.hpp"
#include "../../include/vnd_haas_voice_stream.h"

namespace vnd {

// ceil(row / 256) workgroups are gridDim.y, at most 65535
constexpr int64_t kHaasVoiceMaxRow = (int64_t)65535 * kHaasStreamThreads;
static_assert(kHaasVoiceMaxRow == VND_HAAS_VOICE_MAX_ROW_FRAMES, "the header states the longest row");

// One slot's side of a call, from the stored position, counts[b], flags[b] and delays[b] alone.
struct HaasVoiceSpan {
    int64_t p, n, d;               // position the call starts at, frames pushed, the voice's delay
    int64_t n_out;                 // n, and the d tail frames with END; -1 for a bad slot
    int64_t next;                  // the position after the call
    bool end, ok;                  // !ok: a bad count, position or delay - the slot is left alone
};

__host__ __device__ inline HaasVoiceSpan haas_voice_span(int64_t stored, int32_t count, int32_t flags, int32_t delay,
                                                         int64_t M, int32_t max_delay)
{
    const VoiceSpan v = voice_span(stored, count, flags, M, 0);        // H = 0: the delay is causal, n frames come back
    HaasVoiceSpan s{};
    s.p = v.p; s.n = v.n; s.n_out = v.n_out; s.next = v.next; s.end = v.end; s.ok = v.ok;
    if (!v.ok) return s;
    if (count == 0 && !(flags & (VND_VOICE_START | VND_VOICE_END))) return s;      // idle: its delay is not looked at
    if (delay < 0 || delay > max_delay) {
        s.ok = false; s.p = 0; s.n = 0; s.n_out = -1; s.next = stored;
        return s;
    }
    s.d = delay;
    if (s.end) s.n_out += delay;
    return s;
}

struct HaasVoiceArgs {
    HArgs h;                                            // Cx, delayed_channel, ms, use_width, w_mid, w_side
    const float *__restrict__ x;                        // [slots][M][Cx]
    double *__restrict__ y;                             // [slots][M + max_delay][2]
    float *__restrict__ ring;                           // [slots][cap][Cx]
    int64_t *__restrict__ pos;                          // [slots]
    const int32_t *__restrict__ counts;                 // [slots]
    const int32_t *__restrict__ flags;                  // [slots]
    const int32_t *__restrict__ delays;                 // [slots]
    int32_t *__restrict__ out_counts;                   // [slots]
    int64_t M, cap;                                     // max_frames_per_call, max_delay + M
    int32_t max_delay, slots;
    __device__ VoiceAnswer advance(int64_t b) const
    {
        const HaasVoiceSpan v = haas_voice_span(pos[b], counts[b], flags[b], delays[b], M, max_delay);
        return {(int32_t)v.n_out, v.ok, v.next};
    }
};

// grid = (slots, max(1, ceil((M + max_delay) / kHaasStreamThreads))): one lane per output frame of the longest row
__global__ __launch_bounds__(kHaasStreamThreads) void haas_voice_stream_kernel(const HaasVoiceArgs a)
{
    const int64_t b = blockIdx.x;
    const int tid = threadIdx.x;
    const HaasVoiceSpan v = haas_voice_span(uniform_i64(a.pos[b]), __builtin_amdgcn_readfirstlane(a.counts[b]),
                                            __builtin_amdgcn_readfirstlane(a.flags[b]),
                                            __builtin_amdgcn_readfirstlane(a.delays[b]), a.M, a.max_delay);
    if (!v.ok) return;                                             // nothing is addressed with a bad count, position or delay
    const int Cx = a.h.Cx;
    HaasStreamArgs s{};
    s.h = a.h;
    s.r = ring_plan(v.p, v.n, a.max_delay, v.end, a.cap);
    s.r.chunk = a.x + b * a.M * Cx; s.r.ring = a.ring + b * a.cap * Cx; s.r.Cx = Cx;   // slot b's rows: stream 0 below
    s.ring_first = v.p - a.max_delay;
    s.ring_slot0 = s.r.wr_slot0 - (s.r.wr_first - s.ring_first);   // in [-cap, cap): the header comment
    if (s.ring_slot0 < 0) s.ring_slot0 += a.cap;
    ring_write<kHaasStreamThreads>(s.r, 0, blockIdx.y, gridDim.y, tid);
    const int64_t k = (int64_t)blockIdx.y * kHaasStreamThreads + tid;
    if (k >= v.n_out) return;
    const int64_t t = v.p + k;
    double c[2], o[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        double l = 0.0, r = 0.0;
        const bool in = haas_stream_frame(s, 0, j == s.h.delayed_channel ? t - v.d : t, l, r);
        c[j] = in ? haas_column_of(s.h, j, l, r) : 0.0;                                   // np.roll: zeros wrap in
    }
    haas_frame(s.h, c[0], c[1], o);
    *(double2 *)(a.y + (b * (a.M + a.max_delay) + k) * 2) = make_double2(o[0], o[1]);
}

}  // namespace vnd

// ------------------------------------------------------------------------------
// C ABI (include/vnd_haas_voice_stream.h)
// ------------------------------------------------------------------------------
extern "C" {

vnd_status vnd_haas_voice_stream_state_bytes(int64_t slots, int32_t in_channels, int32_t max_delay,
                                             int64_t max_frames_per_call, int64_t *bytes)
{
    if (!bytes) return fail(VND_ERR_INVALID, "null bytes");
    *bytes = 0;
    int64_t ring = 0;
    vnd_status st = haas_state_bytes(slots, in_channels, max_delay, max_frames_per_call, VND_ERR_UNSUPPORTED, &ring);
    if (st != VND_OK) return st;
    if (max_frames_per_call + max_delay > kHaasVoiceMaxRow)
        return fail(VND_ERR_UNSUPPORTED, "a row of %lld frames, above %lld: its workgroups are one grid dimension",
                    (long long)(max_frames_per_call + max_delay), (long long)kHaasVoiceMaxRow);
    *bytes = voice_position_bytes(slots) + ring;
    return VND_OK;
}

// What the three entries check of the pool: scalars and the state.  Nothing is written.
static vnd_status haas_voice_pool(const vnd_ctx *ctx, const void *state, int64_t state_bytes, int64_t max_frames_per_call,
                                  int64_t slots, int32_t Cx, int32_t max_delay)
{
    if (!ctx) return fail(VND_ERR_INVALID, "null context");
    int64_t need = 0;
    vnd_status st = vnd_haas_voice_stream_state_bytes(slots, Cx, max_delay, max_frames_per_call, &need);
    if (st != VND_OK) return st;
    return voice_state_check("Haas voice pool", state, state_bytes, need, slots);
}

vnd_status vnd_haas_voice_stream_reset_dev(vnd_ctx *ctx, void *state, int64_t state_bytes, int64_t slots, int32_t Cx,
                                           int32_t max_delay, int64_t max_frames_per_call, void *stream_)
{
    vnd_status st = haas_voice_pool(ctx, state, state_bytes, max_frames_per_call, slots, Cx, max_delay);
    if (st != VND_OK) return st;
    return slots == 0 ? VND_OK : voice_reset_positions(ctx, state, slots, stream_);
}

static vnd_status haas_voice_check(const vnd_ctx *ctx, const void *state, int64_t state_bytes, int64_t max_frames_per_call,
                                   const float *x, const int32_t *counts, const int32_t *flags, const int32_t *delays,
                                   const double *y, const int32_t *out_counts, int64_t slots, int32_t Cx, int32_t max_delay,
                                   int32_t delayed_channel)
{
    vnd_status st = haas_voice_pool(ctx, state, state_bytes, max_frames_per_call, slots, Cx, max_delay);
    if (st != VND_OK) return st;
    if (delayed_channel != 0 && delayed_channel != 1)
        return fail(VND_ERR_INVALID, "delayed_channel must be 0 or 1, got %d", delayed_channel);
    if (slots > 0 && (!counts || !flags || !delays || !out_counts || !y || (max_frames_per_call > 0 && !x)))
        return fail(VND_ERR_INVALID, "null chunk, counts, flags, delays, output or out_counts pointer");
    if (slots * (max_frames_per_call + max_delay) * 2 > ((int64_t)1 << 40)) return fail(VND_ERR_UNSUPPORTED, "problem too large");
    return VND_OK;
}

vnd_status vnd_haas_voice_stream_f64_dev(vnd_ctx *ctx, void *state, int64_t state_bytes, int64_t max_frames_per_call,
                                         const float *x, const int32_t *counts, const int32_t *flags, const int32_t *delays,
                                         double *y, int32_t *out_counts, int64_t slots, int32_t Cx, int32_t max_delay,
                                         int32_t delayed_channel, int32_t ms_mode, int32_t use_width, double width,
                                         void *stream_)
{
    vnd_status st = haas_voice_check(ctx, state, state_bytes, max_frames_per_call, x, counts, flags, delays, y, out_counts,
                                     slots, Cx, max_delay, delayed_channel);
    if (st != VND_OK) return st;
    if (slots == 0) return VND_OK;
    HaasVoiceArgs a{};
    a.h.Cx = Cx; a.h.delayed_channel = delayed_channel;
    a.h.ms = ms_mode ? 1 : 0; a.h.use_width = use_width ? 1 : 0; a.h.w_mid = 1.0 - width; a.h.w_side = width;
    a.x = x; a.y = y; a.counts = counts; a.flags = flags; a.delays = delays; a.out_counts = out_counts;
    a.pos = (int64_t *)state;
    a.ring = (float *)((char *)state + voice_position_bytes(slots));
    a.M = max_frames_per_call; a.max_delay = max_delay; a.cap = (int64_t)max_delay + max_frames_per_call;
    a.slots = (int32_t)slots;
    const int64_t row = max_frames_per_call + max_delay;
    const unsigned tiles = (unsigned)std::max<int64_t>(1, (row + kHaasStreamThreads - 1) / kHaasStreamThreads);
    DeviceScope on(ctx->device);
    if (!on.ok) return fail(VND_ERR_HIP, "cannot select device %d", ctx->device);
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(haas_voice_stream_kernel, dim3((unsigned)slots, tiles), dim3(kHaasStreamThreads), 0, stream, a);
    HIP_TRY(hipGetLastError());
    launch_voice_advance(a, slots, stream);
    HIP_TRY(hipGetLastError());
    return VND_OK;
}

vnd_status vnd_haas_voice_stream_f64_host(vnd_ctx *ctx, void *state, int64_t state_bytes, int64_t max_frames_per_call,
                                          const float *x, const int32_t *counts, const int32_t *flags, const int32_t *delays,
                                          double *y, int32_t *out_counts, int64_t slots, int32_t Cx, int32_t max_delay,
                                          int32_t delayed_channel, int32_t ms_mode, int32_t use_width, double width)
{
    vnd_status st = haas_voice_check(ctx, state, state_bytes, max_frames_per_call, x, counts, flags, delays, y, out_counts,
                                     slots, Cx, max_delay, delayed_channel);
    if (st != VND_OK) return st;
    if (slots == 0) return VND_OK;
    for (int64_t b = 0; b < slots; ++b) {
        if (counts[b] < 0 || counts[b] > max_frames_per_call)
            return fail(VND_ERR_INVALID, "count %d of slot %lld is outside [0, %lld]", counts[b], (long long)b,
                        (long long)max_frames_per_call);
        const bool work = counts[b] > 0 || (flags[b] & (VND_VOICE_START | VND_VOICE_END));
        if (work && (delays[b] < 0 || delays[b] > max_delay))
            return fail(VND_ERR_INVALID, "delay %d of slot %lld is outside [0, %d]", delays[b], (long long)b, max_delay);
    }
    const size_t x_bytes = (size_t)(slots * max_frames_per_call * Cx) * sizeof(float);
    const size_t y_bytes = (size_t)(slots * (max_frames_per_call + max_delay) * 2) * sizeof(double);
    const size_t i_bytes = (size_t)slots * sizeof(int32_t);
    HostCall call(ctx);
    call.carve({y_bytes, x_bytes, i_bytes, i_bytes, i_bytes, i_bytes});
    double *y_dev = call.piece<double>(0);
    float *x_dev = call.piece<float>(1);
    int32_t *c_dev = call.piece<int32_t>(2), *f_dev = call.piece<int32_t>(3), *d_dev = call.piece<int32_t>(4);
    int32_t *o_dev = call.piece<int32_t>(5);
    call.up(x_dev, x, x_bytes, "the chunk");
    call.up(y_dev, y, y_bytes, "y");                     // up and back whole: the rows at and past out_counts keep their bytes
    call.up(c_dev, counts, i_bytes, "counts");
    call.up(f_dev, flags, i_bytes, "flags");
    call.up(d_dev, delays, i_bytes, "delays");
    call.run([&] { return vnd_haas_voice_stream_f64_dev(ctx, state, state_bytes, max_frames_per_call, x_dev, c_dev, f_dev, d_dev, y_dev, o_dev, slots, Cx, max_delay, delayed_channel, ms_mode, use_width, width, call.stream()); });
    call.down(y, y_dev, y_bytes, "y");
    call.down(out_counts, o_dev, i_bytes, "out_counts");
    return call.finish("vnd_haas_voice_stream_f64_host");
}

}  // extern "C"

// vnd_haas_stream.hpp - chunked streaming of the HaasEffect delay, one delay for the pool (include/vnd_haas_stream.h) or
// one per stream (include/vnd_each_stream.h): one kernel, one set of checks, one pair of entries behind both.
//
// The delay is causal: output frame t reads input frame t for the undelayed column and t - d for the delayed one, so a call
// that pushes n_in frames per stream at absolute position pos writes outputs [pos, pos + n_in) of every stream, and the
// final call the `reach` tail frames as well: reach = d, or the pool's max_delay where every stream has its own
// d_b <= max_delay (the rows at or past a stream's own n + d_b are then written as +0.0).  Input frames below pos come from
// the stream's ring, frames from pos on from the caller's chunk, frames below 0 and past the end as 0 - what haas_column
// of the one-shot kernel reads outside [0, n).  The ring and its contract are vnd_stream.hpp's (RingArgs), with this reach;
// with reach = 0 there is no state.  Each output frame is haas_column_of / haas_frame of vnd_haas.hpp on the same float32
// samples, so it is the same float64 operation sequence as haas_kernel / haas_each_kernel: the concatenated outputs are
// bit-identical to vnd_haas_f64_* / vnd_haas_each_f64_*.
// Memory-bound: one lane per output frame, one float2 (float for mono) load per column, one double2 store.
#pragma once
#include "vnd_stream.hpp"
#include "../../include/vnd_haas_stream.h"
#include "../../include/vnd_each_stream.h"

namespace vnd {

constexpr int kHaasStreamThreads = 256;

struct HaasStreamArgs {
    HArgs h;                           // Cx, delay (the pool's), delayed_channel, ms, use_width, w_mid, w_side (h.x, h.y, h.n unused)
    RingArgs r;
    double *__restrict__ y;            // [batch][n_out][2]
    const int32_t *__restrict__ delays;    // [batch], a delay per stream (EACH)
    int64_t n_out;
    int64_t ring_first, ring_slot0;    // pos - reach (may be below 0) and its slot, ring_first mod cap in [0, cap)
    int32_t max_delay;                 // (EACH)
};

// Input frame f >= pos - reach of stream s as float32 samples widened to double: (l, r), r = 0 for mono.
// false: frame f reads as zeros, and nothing is loaded.  A frame in [0, pos) comes from the ring at
// ring_slot0 + (f - ring_first), less cap if that is past the end: 0 <= f - ring_first < reach <= cap and
// 0 <= ring_slot0 < cap, so the slot is in [0, cap); it is f mod cap because ring_slot0 = ring_first mod cap.
__device__ __forceinline__ bool haas_stream_frame(const HaasStreamArgs &a, int64_t s, int64_t f, double &l, double &r)
{
    const int Cx = a.h.Cx;
    if (f < 0 || f >= a.r.pos + a.r.n_in) return false;
    const float *__restrict__ p;
    if (f >= a.r.pos) {
        p = a.r.chunk + (s * a.r.n_in + (f - a.r.pos)) * Cx;
    } else {
        int64_t slot = a.ring_slot0 + (f - a.ring_first);
        if (slot >= a.r.cap) slot -= a.r.cap;
        p = a.r.ring + (s * a.r.cap + slot) * Cx;
    }
    if (Cx == 1) {
        l = (double)p[0]; r = 0.0;
    } else {
        const float2 v = *(const float2 *)p;
        l = (double)v.x; r = (double)v.y;
    }
    return true;
}

// grid = (max(1, ceil(n_out / kHaasStreamThreads)), batch): one lane per output frame.  EACH: the delay is the stream's own.
template <bool EACH>
__global__ __launch_bounds__(kHaasStreamThreads) void haas_stream_kernel(const HaasStreamArgs a)
{
    const int64_t s = blockIdx.y;
    const int tid = threadIdx.x;
    ring_write<kHaasStreamThreads>(a.r, s, blockIdx.x, gridDim.x, tid);
    const int64_t k = (int64_t)blockIdx.x * kHaasStreamThreads + tid;
    if (k >= a.n_out) return;
    const int64_t t = a.r.pos + k;
    const int32_t d = EACH ? a.delays[s] : a.h.delay;
    double v[2];
    if (EACH && (d < 0 || d > a.max_delay)) {           // outside the contract: the stream's rows are NaN
        v[0] = v[1] = __builtin_nan("");
    } else if (EACH && t >= a.r.pos + a.r.n_in + d) {   // past this stream's own n + d frames (final call): padding
        v[0] = v[1] = 0.0;
    } else {
        double c[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            double l = 0.0, r = 0.0;
            const bool in = haas_stream_frame(a, s, j == a.h.delayed_channel ? t - d : t, l, r);
            c[j] = in ? haas_column_of(a.h, j, l, r) : 0.0;                               // np.roll: zeros wrap in
        }
        haas_frame(a.h, c[0], c[1], v);
    }
    *(double2 *)(a.y + (s * a.n_out + k) * 2) = make_double2(v[0], v[1]);
}

}  // namespace vnd

// The state of either form; reach = the delay or max_delay.  The two differ in how a pool above VND_MAX_STREAMS is refused:
// too_many = VND_ERR_INVALID with the range check of the batch, VND_ERR_UNSUPPORTED ("split the pool") after the others.
static vnd_status haas_state_bytes(int64_t batch, int32_t in_channels, int32_t reach, int64_t max_frames_per_call,
                                   vnd_status too_many, int64_t *bytes)
{
    const bool each = too_many == VND_ERR_UNSUPPORTED;
    if (!bytes) return fail(VND_ERR_INVALID, "null bytes");
    *bytes = 0;
    if (each && batch < 0) return fail(VND_ERR_INVALID, "negative batch");
    if (!each && (batch < 0 || batch > VND_MAX_STREAMS))
        return fail(too_many, "batch %lld outside 0..%d", (long long)batch, VND_MAX_STREAMS);
    if (in_channels != 1 && in_channels != 2)
        return fail(VND_ERR_INVALID, "HaasEffect takes a mono or stereo signal, got %d channels", in_channels);
    if (reach < 0) return fail(VND_ERR_INVALID, "negative %s %d", each ? "max_delay" : "delay", reach);
    if (max_frames_per_call < 0 || max_frames_per_call > ((int64_t)1 << 40))
        return fail(VND_ERR_INVALID, "max_frames_per_call %lld out of range", (long long)max_frames_per_call);
    if (batch > VND_MAX_STREAMS) return fail(too_many, "more than %d streams per call: split the pool", VND_MAX_STREAMS);
    if (reach == 0) return VND_OK;                       // no frame is ever read back: no state
    *bytes = batch * ((int64_t)reach + max_frames_per_call) * in_channels * (int64_t)sizeof(float);
    return VND_OK;
}

// Every argument check, before anything is enqueued; *n_out from n_in, reach and final alone.  delays: null for one delay.
static vnd_status haas_stream_check(const vnd_ctx *ctx, const void *state, int64_t state_bytes, int64_t max_frames_per_call,
                                    const float *x, const double *y, int64_t batch, int64_t pos, int64_t n_in, int32_t Cx,
                                    int32_t final_, bool each, const int32_t *delays, int32_t reach, int32_t delayed_channel,
                                    int64_t *n_out)
{
    if (!ctx) return fail(VND_ERR_INVALID, "null context");
    if (!n_out) return fail(VND_ERR_INVALID, "null n_out");
    *n_out = 0;
    int64_t need = 0;
    vnd_status st = haas_state_bytes(batch, Cx, reach, max_frames_per_call, each ? VND_ERR_UNSUPPORTED : VND_ERR_INVALID, &need);
    if (st != VND_OK) return st;
    if (delayed_channel != 0 && delayed_channel != 1)
        return fail(VND_ERR_INVALID, "delayed_channel must be 0 or 1, got %d", delayed_channel);
    if ((st = block_stream_check(pos, n_in, max_frames_per_call, state_bytes, need)) != VND_OK) return st;
    const int64_t total = n_in + (final_ ? reach : 0);
    if (batch > 0 && ((need > 0 && !state) || (n_in > 0 && !x) || (total > 0 && (!y || (each && !delays)))))
        return fail(VND_ERR_INVALID, each ? "null state, chunk, output or delay pointer" : "null state, chunk or output pointer");
    if (batch * total * 2 > ((int64_t)1 << 40)) return fail(VND_ERR_UNSUPPORTED, "problem too large");
    *n_out = total;
    return VND_OK;
}

static vnd_status haas_stream_dev(vnd_ctx *ctx, void *state, int64_t state_bytes, int64_t max_frames_per_call, const float *x,
                                  double *y, int64_t batch, int64_t pos, int64_t n_in, int32_t Cx, int32_t final_, bool each,
                                  const int32_t *delays, int32_t reach, int32_t delayed_channel, int32_t ms_mode,
                                  int32_t use_width, double width, int64_t *n_out, void *stream)
{
    vnd_status st = haas_stream_check(ctx, state, state_bytes, max_frames_per_call, x, y, batch, pos, n_in, Cx, final_, each,
                                      delays, reach, delayed_channel, n_out);
    if (st != VND_OK) return st;
    using namespace vnd;
    HaasStreamArgs a{};
    a.h.Cx = Cx; a.h.delay = each ? 0 : reach; a.h.delayed_channel = delayed_channel;
    a.h.ms = ms_mode ? 1 : 0; a.h.use_width = use_width ? 1 : 0; a.h.w_mid = 1.0 - width; a.h.w_side = width;
    a.r = ring_plan(pos, n_in, reach, final_, (int64_t)reach + max_frames_per_call);
    a.r.chunk = x; a.r.ring = (float *)state; a.r.Cx = Cx;
    a.y = y; a.delays = delays; a.max_delay = reach; a.n_out = *n_out;
    a.ring_first = pos - reach;
    a.ring_slot0 = a.r.cap > 0 ? ((a.ring_first % a.r.cap) + a.r.cap) % a.r.cap : 0;
    if (ring_idle(a.r, batch, a.n_out)) return VND_OK;
    const int64_t blocks = std::max<int64_t>(1, (a.n_out + kHaasStreamThreads - 1) / kHaasStreamThreads);
    if (blocks > 0x7fffffffLL) return fail(VND_ERR_UNSUPPORTED, "too many frames in one call");
    DeviceScope on(ctx->device);
    if (!on.ok) return fail(VND_ERR_HIP, "cannot select device %d", ctx->device);
    hipLaunchKernelGGL(each ? haas_stream_kernel<true> : haas_stream_kernel<false>, dim3((unsigned)blocks, (unsigned)batch),
                       dim3(kHaasStreamThreads), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return VND_OK;
}

static vnd_status haas_stream_host(vnd_ctx *ctx, void *state, int64_t state_bytes, int64_t max_frames_per_call, const float *x,
                                   double *y, int64_t batch, int64_t pos, int64_t n_in, int32_t Cx, int32_t final_, bool each,
                                   const int32_t *delays, int32_t reach, int32_t delayed_channel, int32_t ms_mode,
                                   int32_t use_width, double width, int64_t *n_out, const char *name)
{
    vnd_status st = haas_stream_check(ctx, state, state_bytes, max_frames_per_call, x, y, batch, pos, n_in, Cx, final_, each,
                                      delays, reach, delayed_channel, n_out);
    if (st != VND_OK) return st;
    const int64_t nout = *n_out;
    if (batch == 0 || (n_in == 0 && nout == 0)) return VND_OK;
    const HostIndex ix{delays, reach, true, "delay", "delays", "stream"};
    HostCall call(ctx);
    call.staged(x, (size_t)(batch * n_in * Cx) * sizeof(float), "the chunk", y, (size_t)(batch * nout * 2) * sizeof(double),
                each ? &ix : nullptr, batch, 0, n_out, [&](void *x_dev, void *y_dev, int32_t *d_dev, void *, hipStream_t s) {
        int64_t got = 0;
        return haas_stream_dev(ctx, state, state_bytes, max_frames_per_call, (const float *)x_dev, (double *)y_dev, batch, pos, n_in,
                               Cx, final_, each, d_dev, reach, delayed_channel, ms_mode, use_width, width, &got, s);
    });
    return call.finish(name);
}

extern "C" {

vnd_status vnd_haas_stream_state_bytes(int64_t batch, int32_t in_channels, int32_t delay, int64_t max_frames_per_call,
                                       int64_t *bytes)
{
    return haas_state_bytes(batch, in_channels, delay, max_frames_per_call, VND_ERR_INVALID, bytes);
}

vnd_status vnd_haas_each_stream_state_bytes(int64_t batch, int32_t in_channels, int32_t max_delay, int64_t max_frames_per_call,
                                            int64_t *bytes)
{
    return haas_state_bytes(batch, in_channels, max_delay, max_frames_per_call, VND_ERR_UNSUPPORTED, bytes);
}

vnd_status vnd_haas_stream_f64_dev(vnd_ctx *ctx, void *state, int64_t state_bytes, int64_t max_frames_per_call,
                                   const float *x, double *y, int64_t batch, int64_t pos, int64_t n_in, int32_t Cx,
                                   int32_t final_, int32_t delay, int32_t delayed_channel, int32_t ms_mode,
                                   int32_t use_width, double width, int64_t *n_out, void *stream)
{
    return haas_stream_dev(ctx, state, state_bytes, max_frames_per_call, x, y, batch, pos, n_in, Cx, final_, false, nullptr,
                           delay, delayed_channel, ms_mode, use_width, width, n_out, stream);
}

vnd_status vnd_haas_stream_f64_host(vnd_ctx *ctx, void *state, int64_t state_bytes, int64_t max_frames_per_call,
                                    const float *x, double *y, int64_t batch, int64_t pos, int64_t n_in, int32_t Cx,
                                    int32_t final_, int32_t delay, int32_t delayed_channel, int32_t ms_mode,
                                    int32_t use_width, double width, int64_t *n_out)
{
    return haas_stream_host(ctx, state, state_bytes, max_frames_per_call, x, y, batch, pos, n_in, Cx, final_, false, nullptr,
                            delay, delayed_channel, ms_mode, use_width, width, n_out, "vnd_haas_stream_f64_host");
}

vnd_status vnd_haas_each_stream_f64_dev(vnd_ctx *ctx, void *state, int64_t state_bytes, int64_t max_frames_per_call,
                                        const float *x, double *y, int64_t batch, int64_t pos, int64_t n_in, int32_t Cx,
                                        int32_t final_, const int32_t *delays, int32_t max_delay, int32_t delayed_channel,
                                        int32_t ms_mode, int32_t use_width, double width, int64_t *n_out, void *stream)
{
    return haas_stream_dev(ctx, state, state_bytes, max_frames_per_call, x, y, batch, pos, n_in, Cx, final_, true, delays,
                           max_delay, delayed_channel, ms_mode, use_width, width, n_out, stream);
}

vnd_status vnd_haas_each_stream_f64_host(vnd_ctx *ctx, void *state, int64_t state_bytes, int64_t max_frames_per_call,
                                         const float *x, double *y, int64_t batch, int64_t pos, int64_t n_in, int32_t Cx,
                                         int32_t final_, const int32_t *delays, int32_t max_delay, int32_t delayed_channel,
                                         int32_t ms_mode, int32_t use_width, double width, int64_t *n_out)
{
    return haas_stream_host(ctx, state, state_bytes, max_frames_per_call, x, y, batch, pos, n_in, Cx, final_, true, delays,
                            max_delay, delayed_channel, ms_mode, use_width, width, n_out, "vnd_haas_each_stream_f64_host");
}

}  // extern "C"

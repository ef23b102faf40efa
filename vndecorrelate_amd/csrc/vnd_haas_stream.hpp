// vnd_haas_stream.hpp - chunked streaming of the HaasEffect delay (include/vnd_haas_stream.h).
//
// The delay is causal: output frame t reads input frame t for the undelayed column and t - d for the delayed one, so a call
// that pushes n_in frames per stream at absolute position pos writes outputs [pos, pos + n_in) of every stream, and the
// final call the d tail frames as well.  Input frames below pos come from a per-stream RING in device memory (capacity
// d + max_frames_per_call, slot = absolute frame mod capacity), frames from pos on from the caller's chunk, frames below 0
// and past the end as 0 - what haas_column of the one-shot kernel reads outside [0, n).  The same launch copies the chunk's
// last min(n_in, d) frames into the ring: a read frame f and a written frame g have 0 < g - f <= d + n_in - 1 < capacity,
// so no slot is both read and written in one call (the argument of vnd_stream.hpp with H = d), and every frame is written
// once.  Each output frame is haas_column_of / haas_frame of vnd_haas.hpp on the same float32 samples, so it is the same
// float64 operation sequence as haas_kernel: the concatenated outputs are bit-identical to vnd_haas_f64_*.
// Memory-bound: one lane per output frame, one float2 (float for mono) load per column, one double2 store.
#pragma once
#include "../../include/vnd_haas_stream.h"

namespace vnd {

constexpr int kHaasStreamThreads = 256;

struct HSArgs {
    HArgs h;                           // Cx, delay, delayed_channel, ms, use_width, w_mid, w_side (h.x, h.y, h.n unused)
    const float *__restrict__ chunk;   // [batch][n_in][Cx]
    float *__restrict__ ring;          // [batch][cap][Cx]
    double *__restrict__ y;            // [batch][n_out][2]
    int64_t pos, n_in, n_out;
    int64_t cap;                       // ring capacity, frames
    int64_t ring_first, ring_slot0;    // first frame a call can read from the ring (max(0, pos - d)) and its slot
    int64_t wr_first, wr_count, wr_slot0;   // chunk frames [wr_first, wr_first + wr_count) (absolute) go to the ring
};

// Input frame f of stream s as float32 samples widened to double: (l, r), r = 0 for mono.  false: frame f reads as zeros.
// Frames below pos come from the ring, where a frame below 0 loads the slot of ring_first (in bounds; at position 0 a slot
// this call may also write) and the value is discarded: the delayed column's source changes only where t - d crosses pos,
// and the undelayed one's where t crosses pos + n_in, so at most two waves of a stream diverge on it.
__device__ __forceinline__ bool haas_stream_frame(const HSArgs &a, int64_t s, int64_t f, double &l, double &r)
{
    const int Cx = a.h.Cx;
    const float *__restrict__ p;
    if (f >= a.pos) {
        if (f >= a.pos + a.n_in) return false;
        p = a.chunk + (s * a.n_in + (f - a.pos)) * Cx;
    } else {
        int64_t slot = a.ring_slot0 + (f > a.ring_first ? f - a.ring_first : 0);     // f - ring_first < d <= cap
        if (slot >= a.cap) slot -= a.cap;
        p = a.ring + (s * a.cap + slot) * Cx;
    }
    if (Cx == 1) {
        l = (double)p[0]; r = 0.0;
    } else {
        const float2 v = *(const float2 *)p;
        l = (double)v.x; r = (double)v.y;
    }
    return f >= 0;
}

__global__ __launch_bounds__(kHaasStreamThreads) void haas_stream_kernel(const HSArgs a)
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
    double c[2], v[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        double l = 0.0, r = 0.0;
        const bool in = haas_stream_frame(a, s, j == a.h.delayed_channel ? t - a.h.delay : t, l, r);
        c[j] = in ? haas_column_of(a.h, j, l, r) : 0.0;                                   // np.roll: zeros wrap in
    }
    haas_frame(a.h, c[0], c[1], v);
    *(double2 *)(a.y + (s * a.n_out + k) * 2) = make_double2(v[0], v[1]);
}

}  // namespace vnd

static int64_t haas_stream_capacity(int32_t delay, int64_t max_frames_per_call)
{
    return (int64_t)delay + max_frames_per_call;
}

extern "C" {

vnd_status vnd_haas_stream_state_bytes(int64_t batch, int32_t in_channels, int32_t delay, int64_t max_frames_per_call,
                                       int64_t *bytes)
{
    if (!bytes) return fail(VND_ERR_INVALID, "null bytes");
    *bytes = 0;
    if (batch < 0 || batch > VND_MAX_STREAMS) return fail(VND_ERR_INVALID, "batch %lld outside 0..%d", (long long)batch, VND_MAX_STREAMS);
    if (in_channels != 1 && in_channels != 2)
        return fail(VND_ERR_INVALID, "HaasEffect takes a mono or stereo signal, got %d channels", in_channels);
    if (delay < 0) return fail(VND_ERR_INVALID, "negative delay %d", delay);
    if (max_frames_per_call < 0 || max_frames_per_call > ((int64_t)1 << 40))
        return fail(VND_ERR_INVALID, "max_frames_per_call %lld out of range", (long long)max_frames_per_call);
    if (delay == 0) return VND_OK;                       // no frame is ever read back: no state
    *bytes = batch * haas_stream_capacity(delay, max_frames_per_call) * in_channels * (int64_t)sizeof(float);
    return VND_OK;
}

// Every argument check, before anything is enqueued; *n_out from position, n_in, d and final alone.
static vnd_status haas_stream_check(vnd_ctx *ctx, const void *state, int64_t state_bytes, int64_t max_frames_per_call,
                                    const float *x, const double *y, int64_t batch, int64_t pos, int64_t n_in, int32_t Cx,
                                    int32_t final_, int32_t delay, int32_t delayed_channel, int64_t *n_out)
{
    if (!ctx) return fail(VND_ERR_INVALID, "null context");
    if (!n_out) return fail(VND_ERR_INVALID, "null n_out");
    *n_out = 0;
    int64_t need = 0;
    vnd_status st = vnd_haas_stream_state_bytes(batch, Cx, delay, max_frames_per_call, &need);
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
    const int64_t total = n_in + (final_ ? delay : 0);
    if (batch > 0 && ((need > 0 && !state) || (n_in > 0 && !x) || (total > 0 && !y)))
        return fail(VND_ERR_INVALID, "null state, chunk or output pointer");
    if (batch * total * 2 > ((int64_t)1 << 40)) return fail(VND_ERR_UNSUPPORTED, "problem too large");
    *n_out = total;
    return VND_OK;
}

vnd_status vnd_haas_stream_f64_dev(vnd_ctx *ctx, void *state, int64_t state_bytes, int64_t max_frames_per_call,
                                   const float *x, double *y, int64_t batch, int64_t pos, int64_t n_in, int32_t Cx,
                                   int32_t final_, int32_t delay, int32_t delayed_channel, int32_t ms_mode,
                                   int32_t use_width, double width, int64_t *n_out, void *stream)
{
    vnd_status st = haas_stream_check(ctx, state, state_bytes, max_frames_per_call, x, y, batch, pos, n_in, Cx, final_,
                                      delay, delayed_channel, n_out);
    if (st != VND_OK) return st;
    using namespace vnd;
    HSArgs a{};
    a.h.Cx = Cx; a.h.delay = delay; a.h.delayed_channel = delayed_channel;
    a.h.ms = ms_mode ? 1 : 0; a.h.use_width = use_width ? 1 : 0; a.h.w_mid = 1.0 - width; a.h.w_side = width;
    a.chunk = x; a.ring = (float *)state; a.y = y;
    a.pos = pos; a.n_in = n_in; a.n_out = *n_out;
    a.cap = haas_stream_capacity(delay, max_frames_per_call);
    a.ring_first = std::max<int64_t>(0, pos - delay);
    a.ring_slot0 = a.cap > 0 ? a.ring_first % a.cap : 0;
    // the last d frames of the chunk are what later calls read (none after the final call, none without a delay)
    a.wr_first = (final_ || delay == 0) ? pos + n_in : std::max<int64_t>(pos, pos + n_in - delay);
    a.wr_count = pos + n_in - a.wr_first;
    a.wr_slot0 = a.cap > 0 ? a.wr_first % a.cap : 0;
    if (batch == 0 || (a.n_out == 0 && a.wr_count == 0)) return VND_OK;
    const int64_t blocks = std::max<int64_t>(1, (a.n_out + kHaasStreamThreads - 1) / kHaasStreamThreads);
    if (blocks > 0x7fffffffLL) return fail(VND_ERR_UNSUPPORTED, "too many frames in one call");
    DeviceScope on(ctx->device);
    if (!on.ok) return fail(VND_ERR_HIP, "cannot select device %d", ctx->device);
    hipLaunchKernelGGL(haas_stream_kernel, dim3((unsigned)blocks, (unsigned)batch), dim3(kHaasStreamThreads), 0,
                       (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return VND_OK;
}

vnd_status vnd_haas_stream_f64_host(vnd_ctx *ctx, void *state, int64_t state_bytes, int64_t max_frames_per_call,
                                    const float *x, double *y, int64_t batch, int64_t pos, int64_t n_in, int32_t Cx,
                                    int32_t final_, int32_t delay, int32_t delayed_channel, int32_t ms_mode,
                                    int32_t use_width, double width, int64_t *n_out)
{
    vnd_status st = haas_stream_check(ctx, state, state_bytes, max_frames_per_call, x, y, batch, pos, n_in, Cx, final_,
                                      delay, delayed_channel, n_out);
    if (st != VND_OK) return st;
    const int64_t nout = *n_out;
    if (batch == 0 || (n_in == 0 && nout == 0)) return VND_OK;
    HostCall call(ctx);
    const size_t x_bytes = (size_t)(batch * n_in * Cx) * sizeof(float);
    const size_t y_bytes = (size_t)(batch * nout * 2) * sizeof(double);
    call.carve({x_bytes, y_bytes});
    float *x_dev = call.piece<float>(0);
    double *y_dev = call.piece<double>(1);
    call.up(x_dev, x, x_bytes, "the chunk");
    int64_t got = 0;
    call.run([&] { return vnd_haas_stream_f64_dev(ctx, state, state_bytes, max_frames_per_call, x_dev, y_dev, batch, pos, n_in, Cx,
                                                  final_, delay, delayed_channel, ms_mode, use_width, width, &got, call.stream()); });
    call.down(y, y_dev, y_bytes, "y");
    return call.finish("vnd_haas_stream_f64_host");
}

}  // extern "C"

// vnd_correlogram_stream.hpp - the cross-correlogram streamed block by block (include/vnd_correlogram_stream.h).
// (one translation unit: included by vnd_amd.hip after vnd_correlogram.hpp; everything static here is private to the library)
//
// The compute is correlogram_kernel's (vnd_correlogram.hpp), instantiated with a second sample source, CgRing: frame
// f < pos of a window comes from the per-stream ring, slot f mod cap; frame f >= pos from the caller's chunk at f - pos.
// The block ranges, the staging, cg_load / cg_block, the energy chains and butterfly and the float32 normaliser are the
// one-shot kernel's, so every row is the same operation sequence on the same values: bit for bit the one-shot call's row.
//
// Ring (its own, planar float2 from strided sources; the contract is RingArgs' of vnd_stream.hpp with reach = W - 1).
// Per stream, cap = W - 1 + max_frames_per_call frames of interleaved float32 (x, y) pairs.  A call's launch copies
// the chunk's last min(n_in, W - 1) frames into the ring.  Why no slot is both read and written in one call:
//   * the windows completing in a call are w >= wc(pos), and window wc(pos) was not complete at pos: wc(pos) H + W - 1 >=
//     pos, so every frame read from the ring lies in [pos - W + 1, pos);
//   * the frames written lie in [pos + n_in - min(n_in, W - 1), pos + n_in);
//   * so a written frame g and a read frame f satisfy 0 < g - f <= W - 2 + n_in < cap: different slots.
// Why the ring holds what is read: frame f in [pos - W + 1, pos) was written by the call that pushed it (it was among that
// call's last W - 1 frames, as every later frame up to pos is), and a frame g > f overwrites its slot only if g >= f + cap
// > pos.  Windows start at frame 0 or later, so slots before frame 0 are never read and the ring needs no clearing.
// The slot of a window's first frame is one 64-bit modulo per window; a staged run is consecutive frames, so slot0 + i
// (i < W <= cap) wraps with one conditional subtract.
#pragma once
#include "../../include/vnd_correlogram_stream.h"

struct CgStreamArgs {
    CgArgs cg;                        // x, y, stream_stride, frame_stride: the chunk; windows: rows of this call
    float2 *__restrict__ ring;        // [batch][cap] (x, y)
    int64_t pos, cap;
    int64_t w0;                       // window of row 0
    int64_t wr_first, wr_count, wr_slot0;   // chunk frames [wr_first, wr_first + wr_count) (absolute) go to the ring
};

struct CgRing {
    using Args = CgStreamArgs;
    static constexpr bool kRing = true;
    struct Run {
        const float *px, *py;         // the chunk of the stream
        const float2 *ring;           // the ring of the stream
        int64_t rel, slot0, cap;      // rel: the window's first frame - pos
        int32_t fs;
        __device__ __forceinline__ int64_t slot(int i) const
        {
            const int64_t s = slot0 + i;
            return s >= cap ? s - cap : s;
        }
        __device__ __forceinline__ float x(int i) const
        {
            const int64_t r = rel + i;
            return r >= 0 ? px[r * fs] : ring[slot(i)].x;
        }
        __device__ __forceinline__ float y(int i) const
        {
            const int64_t r = rel + i;
            return r >= 0 ? py[r * fs] : ring[slot(i)].y;
        }
    };
    using View = const Args &;
    __device__ static __forceinline__ View view(const Args &a) { return a; }
    __device__ static __forceinline__ const CgArgs &cg(const Args &a) { return a.cg; }
    __device__ static __forceinline__ int64_t stream(const Args &) { return blockIdx.y; }
    __device__ static __forceinline__ int64_t group(const Args &a) { return cg_grid_group(a.cg); }
    __device__ static __forceinline__ int tile(const Args &a) { return cg_grid_tile(a.cg); }
    __device__ static __forceinline__ int64_t first_frame(const Args &a, int64_t ww) { return (a.w0 + ww) * a.cg.hop; }
    __device__ static __forceinline__ int64_t slot0_of(const Args &a, int64_t ww) { return first_frame(a, ww) % a.cap; }
    __device__ static __forceinline__ Run run(const Args &a, int64_t b, int64_t ww, int64_t slot0)
    {
        return Run{a.cg.x + b * a.cg.stream_stride, a.cg.y + b * a.cg.stream_stride, a.ring + b * a.cap,
                   first_frame(a, ww) - a.pos, slot0, a.cap, a.cg.frame_stride};
    }
    // The chunk frames later calls read, into the ring: the stream's workgroups share them in grid-stride order.  A
    // launch without rows only does this.
    __device__ static __forceinline__ bool prologue(const Args &a, int64_t b)
    {
        const float *cx = a.cg.x + b * a.cg.stream_stride, *cy = a.cg.y + b * a.cg.stream_stride;
        float2 *ring = a.ring + b * a.cap;
        const int64_t rel0 = a.wr_first - a.pos;
        for (int64_t k = (int64_t)blockIdx.x * kCgThreads + threadIdx.x; k < a.wr_count;
             k += (int64_t)gridDim.x * kCgThreads) {
            int64_t s = a.wr_slot0 + k;
            if (s >= a.cap) s -= a.cap;
            const int64_t r = (rel0 + k) * a.cg.frame_stride;
            ring[s] = make_float2(cx[r], cy[r]);
        }
        return a.cg.windows > 0;
    }
};

static int64_t cg_windows_complete(int64_t p, int64_t W, int64_t H) { return p >= W ? (p - W) / H + 1 : 0; }

extern "C" {

vnd_status vnd_correlogram_stream_state_bytes(int64_t batch, int32_t window, int64_t max_frames_per_call, int64_t *bytes)
{
    if (!bytes) return fail(VND_ERR_INVALID, "null bytes");
    *bytes = 0;
    if (batch < 1 || window < 1 || max_frames_per_call < 1)
        return fail(VND_ERR_INVALID, "batch, window and max_frames_per_call must be >= 1");
    if (window > VND_CORRELOGRAM_MAX_WINDOW)
        return fail(VND_ERR_UNSUPPORTED, "window %d above the %d-sample cap", window, VND_CORRELOGRAM_MAX_WINDOW);
    int64_t cap, need;
    if (__builtin_add_overflow(max_frames_per_call, (int64_t)window - 1, &cap) || __builtin_mul_overflow(batch, cap, &need)
        || __builtin_mul_overflow(need, (int64_t)sizeof(float2), &need) || need > INT64_MAX / 8)
        return fail(VND_ERR_INVALID, "state of %lld streams x %lld frames overflows", (long long)batch,
                    (long long)max_frames_per_call);
    *bytes = need;
    return VND_OK;
}

vnd_status vnd_correlogram_stream_f32_dev(vnd_ctx *ctx, void *state, int64_t state_bytes, int64_t max_frames_per_call,
                                          const float *x, const float *y, int64_t stream_stride, int32_t frame_stride,
                                          float *out, int64_t batch, int64_t pos, int64_t n_in, int32_t window, int32_t hop,
                                          int32_t num_lags, float eps, int64_t *n_rows, void *stream_)
{
    if (!ctx) return fail(VND_ERR_INVALID, "null context");
    if (!n_rows) return fail(VND_ERR_INVALID, "null n_rows");
    *n_rows = 0;
    if (batch < 1 || stream_stride < 1 || frame_stride < 1 || window < 1 || hop < 1 || num_lags < 1 ||
        max_frames_per_call < 1)
        return fail(VND_ERR_INVALID, "batch, strides, window, hop, num_lags and max_frames_per_call must be >= 1");
    if (pos < 0 || n_in < 0) return fail(VND_ERR_INVALID, "negative position or frame count");
    if (pos > ((int64_t)1 << 60)) return fail(VND_ERR_INVALID, "position %lld out of range", (long long)pos);
    if (window > VND_CORRELOGRAM_MAX_WINDOW)
        return fail(VND_ERR_UNSUPPORTED, "window %d above the %d-sample cap", window, VND_CORRELOGRAM_MAX_WINDOW);
    int64_t need = 0;
    vnd_status st = vnd_correlogram_stream_state_bytes(batch, window, max_frames_per_call, &need);
    if (st != VND_OK) return st;
    if (n_in > max_frames_per_call)
        return fail(VND_ERR_INVALID, "%lld frames in one call, above max_frames_per_call %lld", (long long)n_in,
                    (long long)max_frames_per_call);
    if (state_bytes < need)
        return fail(VND_ERR_INVALID, "state of %lld bytes, the stream needs %lld", (long long)state_bytes, (long long)need);
    const int64_t w0 = cg_windows_complete(pos, window, hop);
    const int64_t rows = cg_windows_complete(pos + n_in, window, hop) - w0;
    if (n_in == 0) return VND_OK;                               // nothing to read, keep or write: no launch
    if (!state || !x || !y || (rows > 0 && !out)) return fail(VND_ERR_INVALID, "null state, chunk or output pointer");
    // extents in floats: the last sample of the chunk's last stream, and the output
    int64_t span, xlast, outn = 0;
    if (__builtin_mul_overflow(batch - 1, stream_stride, &span) ||
        __builtin_mul_overflow(n_in - 1, (int64_t)frame_stride, &xlast) || __builtin_add_overflow(span, xlast, &span) ||
        __builtin_mul_overflow(batch, rows, &outn) || __builtin_mul_overflow(outn, (int64_t)num_lags, &outn) ||
        span > INT64_MAX / 8 || outn > INT64_MAX / 8)
        return fail(VND_ERR_INVALID, "buffer extents overflow");
    const int64_t xb = (span + 1) * (int64_t)sizeof(float), ob = outn * (int64_t)sizeof(float);
    auto overlap = [](const void *p, int64_t pb, const void *q, int64_t qb) {
        const char *p0 = (const char *)p, *q0 = (const char *)q;
        return pb > 0 && qb > 0 && p0 < q0 + qb && q0 < p0 + pb;
    };
    for (const float *p : {x, y})
        if (overlap(p, xb, out, ob) || overlap(p, xb, state, need))
            return fail(VND_ERR_INVALID, "out and the state must not overlap the chunk");
    if (overlap(out, ob, state, need)) return fail(VND_ERR_INVALID, "out must not overlap the state");
    DeviceScope on(ctx->device);
    if (!on.ok) return fail(VND_ERR_HIP, "cannot select device %d", ctx->device);
    hipStream_t stream = (hipStream_t)stream_;

    CgStreamArgs c{};
    c.cg.x = x; c.cg.y = y; c.cg.out = out; c.cg.windows = rows; c.cg.stream_stride = stream_stride;
    c.cg.frame_stride = frame_stride; c.cg.W = window; c.cg.hop = hop; c.cg.num_lags = num_lags;
    c.cg.jmax = (int32_t)std::min<int64_t>(num_lags, 2 * (int64_t)window - 1);
    c.cg.tiles = (int32_t)((num_lags + kCgTile - 1) / kCgTile);
    c.cg.eps = eps;
    c.ring = (float2 *)state; c.pos = pos; c.cap = max_frames_per_call + window - 1; c.w0 = w0;
    c.wr_count = std::min<int64_t>(n_in, window - 1);
    c.wr_first = pos + n_in - c.wr_count;
    c.wr_slot0 = c.wr_first % c.cap;
    // as the one-shot call: at most 2^23 workgroups per launch in x, VND_MAX_STREAMS in y.  The ring copy rides in the
    // first launch of each slice of streams; without rows that launch has just enough workgroups for it.
    const int64_t groups = (rows + kCgG - 1) / kCgG;
    const int64_t per_launch = std::max<int64_t>(1, ((int64_t)1 << 23) / c.cg.tiles);
    const int64_t copy_blocks = std::max<int64_t>(1, (c.wr_count + kCgThreads - 1) / kCgThreads);
    for (int64_t b0 = 0; b0 < batch; b0 += VND_MAX_STREAMS) {
        const int64_t nb = std::min<int64_t>(VND_MAX_STREAMS, batch - b0);
        CgStreamArgs s = c;
        s.cg.x = x + b0 * stream_stride; s.cg.y = y + b0 * stream_stride; s.cg.out = out + b0 * rows * (int64_t)num_lags;
        s.ring = c.ring + b0 * c.cap;
        int64_t g0 = 0;
        do {
            s.cg.group0 = g0;
            const int64_t ng = std::min(per_launch, groups - g0);
            const int64_t blocks = ng > 0 ? ng * c.cg.tiles : copy_blocks;
            hipLaunchKernelGGL(correlogram_kernel<CgRing>, dim3((unsigned)blocks, (unsigned)nb), dim3(kCgThreads), 0, stream, s);
            s.wr_count = 0;                                     // the ring copy is done by the first launch
            g0 += per_launch;
        } while (g0 < groups);
    }
    HIP_TRY(hipGetLastError());
    *n_rows = rows;
    return VND_OK;
}

}  // extern "C"

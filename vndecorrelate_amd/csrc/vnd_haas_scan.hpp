// vnd_haas_scan.hpp - the Haas-delay optimiser's scan on the device (include/vnd_scan.h, include/vnd_haas_search.h):
// the eight polar moments (vnd_moments.hpp's quantities and order) of HaasEffect(delay d_p).decorrelate(x[s_p]) for
// P pairs (signal s_p, delay d_p) of a pool x[batch][n][Cx], without writing any delayed signal.  The single-signal
// scan (vnd_haas_scan_f64_*) is the case "every pair is signal 0" (signals == nullptr).
//
// Frame k of pair p (k in [0, n + d_p)) is haas_column / haas_frame of vnd_haas.hpp at (k, k - d_p), so it is
// bit-identical to the reference's float64 frame, and polar_add64 (vnd_polar.hpp) takes it in float64 as the
// reference's polar_coordinates does.  The roll's zero prefix and the tail past the signal are ordinary frames.
//
// Shape: the hot loop is one float64 atan2 and one sqrt per (frame, pair) - FP64 VALU, not memory.  A workgroup
// owns a tile of kHsTile frames and a block of kHsBlock consecutive pairs, which it walks as runs of one signal.
// The undelayed column of the tile is the same for every pair of a run: each lane keeps its kHsPer frames of it in
// registers.  The delayed column is staged once per run in LDS over the run's history window
// [t0 - dmax, t0 + kHsTile - dmin) (pairs sorted by (signal, delay) keep runs long and dmax - dmin small), and the
// run's pairs sweep the tile from there.  A run whose window does not fit kHsWin reads the delayed column through
// haas_column from global memory instead: the same values, so the same bits.
//
// Sums are float64 in a fixed order: per lane over its frames, a fixed shuffle tree and wave order per (tile, pair)
// partial, then a fixed-order reduction of pair p's ceil((n + d_p) / kHsTile) partials.  Neither the other pairs of a
// launch, nor their order, nor the launch's extent enter pair p's order, so results are bit-identical across runs
// and across how the pairs are ordered and split into launches.
//
// The two kernels' bodies are templates over where a signal's frames come from (HsFrames below: a contiguous pool), so
// that vnd_haas_scan_voice_stream.hpp can run the same text over the rings of a voice pool and the two cannot drift.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vnd_haas.hpp"
#include "vnd_polar.hpp"
#include "../../include/vnd_scan.h"
#include "../../include/vnd_haas_search.h"

namespace vnd {

constexpr int kHsThreads = 256;
constexpr int kHsPer = 8;                               // frames per lane and tile
constexpr int kHsTile = kHsThreads * kHsPer;            // 2048 frames per workgroup
constexpr int kHsBlock = 16;                            // pairs per workgroup
constexpr int kHsWin = 4096;                            // staged delayed-column doubles (32 KB of LDS)

__host__ __device__ __forceinline__ int64_t hs_chunks(int64_t frames) { return (frames + kHsTile - 1) / kHsTile; }

// Where a run's frames come from.  The scan's body (hs_scan_body, hs_reduce_body) is written once over an Args type with
//   signal(f)    the signal of pair f, as stored (any int32)
//   valid(s, d)  whether pair (s, d) is inside the contract - nothing is addressed with an s or a d that is not
//   open(s)      the frames of a valid signal s (workgroup-uniform): n, and column(h, c, k), column c of the padded buffer
//                before the roll at frame k - zero outside [0, n)
// and the fields h, delays, partials, moments, F and cap.  Two instantiations: HsArgs below, a contiguous pool
// x[batch][n][Cx] where every signal has h.n frames, and HsRingArgs of vnd_haas_scan_voice_stream.hpp, the windows a voice
// pool keeps in rings, each with a length of its own.
struct HsFrames {
    const float *__restrict__ xs;                       // [n][Cx]
    int64_t n;
    __device__ __forceinline__ double column(const HArgs &h, int c, int64_t k) const { return haas_column(h, xs, c, k); }
};

struct HsArgs {
    HArgs h;                                            // pool (h.x, h.n, h.Cx) and the shared configuration
    const int32_t *__restrict__ signals;                // [F] signal of each pair; nullptr: every pair is signal 0
    const int32_t *__restrict__ delays;                 // [F]
    double *__restrict__ partials;                      // [F][cap][8]
    double *__restrict__ moments;                       // [F][8]
    int32_t F;                                          // pairs
    int32_t batch;                                      // signals in the pool
    int64_t cap;                                        // partials per pair the workspace holds
    __device__ __forceinline__ int32_t signal(int f) const { return signals ? signals[f] : 0; }
    __device__ __forceinline__ bool valid(int32_t s, int32_t d) const
    {
        return s >= 0 && s < batch && d >= 0 && hs_chunks(h.n + d) <= cap;
    }
    __device__ __forceinline__ HsFrames open(int32_t s) const { return {h.x + (int64_t)s * h.n * h.Cx, h.n}; }
};

// fixed-order sum (max for slot 4) of v over the workgroup; the result is valid in thread 0
__device__ __forceinline__ void hs_block_reduce(double v[kMoments], double (*red)[kMoments])
{
#pragma unroll
    for (int k = 0; k < kMoments; ++k) {
#pragma unroll
        for (int sh = 32; sh > 0; sh >>= 1) {
            const double o = __shfl_xor(v[k], sh);
            v[k] = k == 4 ? fmax(v[k], o) : v[k] + o;
        }
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < kMoments; ++k) red[threadIdx.x >> 6][k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < kMoments; ++k) {
            double t = red[0][k];
            for (int w = 1; w < kHsThreads / 64; ++w) t = k == 4 ? fmax(t, red[w][k]) : t + red[w][k];
            v[k] = t;
        }
    }
    __syncthreads();                                    // red[] is free for the next candidate
}

// The scan of one workgroup: tile blockIdx.x of the block of pairs blockIdx.y.  grid = (tiles, ceil(F / kHsBlock))
template <class Args>
__device__ __forceinline__ void hs_scan_body(const Args &a)
{
    __shared__ double hist[kHsWin];
    __shared__ double red[kHsThreads / 64][kMoments];
    __shared__ int32_t dl[kHsBlock], sl[kHsBlock];      // delay (-1: outside the contract) and signal of each pair
    __shared__ int32_t run[kHsBlock][3];                // at a run's first pair: its end, dmin and dmax
    const int f0 = blockIdx.y * kHsBlock;
    const int nb = min(kHsBlock, a.F - f0);
    if ((int)threadIdx.x < nb) {
        const int32_t s = a.signal(f0 + threadIdx.x), d = a.delays[f0 + threadIdx.x];
        sl[threadIdx.x] = s;
        dl[threadIdx.x] = a.valid(s, d) ? d : -1;
    }
    __syncthreads();
    if ((int)threadIdx.x < nb && (threadIdx.x == 0 || sl[threadIdx.x - 1] != sl[threadIdx.x])) {
        int c = threadIdx.x;
        int32_t dmin = INT32_MAX, dmax = -1;            // over the run's valid pairs
        for (; c < nb && sl[c] == sl[threadIdx.x]; ++c) {
            if (dl[c] >= 0) { dmin = min(dmin, dl[c]); dmax = max(dmax, dl[c]); }
        }
        run[threadIdx.x][0] = c; run[threadIdx.x][1] = dmin; run[threadIdx.x][2] = dmax;
    }
    __syncthreads();
    const HArgs &h = a.h;
    const int cu = 1 - h.delayed_channel, cd = h.delayed_channel;
    const int64_t t0 = (int64_t)blockIdx.x * kHsTile;
    // runs of consecutive pairs of one signal (wave-uniform: every bound comes from LDS)
    for (int r0 = 0, r1; r0 < nb; r0 = r1) {
        r1 = run[r0][0];
        const int32_t s = __builtin_amdgcn_readfirstlane(sl[r0]);
        const int32_t dmin = run[r0][1], dmax = run[r0][2];
        if (dmax < 0) continue;                         // no pair of the run is inside the contract
        const auto x = a.open(s);                       // (s is valid: a pair of the run is)
        if (t0 >= x.n + dmax) continue;                 // no pair of the run reaches this tile
        // the delayed column over [t0 - dmax, t0 + kHsTile - dmin)
        const int64_t span = (int64_t)kHsTile + dmax - dmin;
        const bool staged = span <= kHsWin;
        if (staged) {
            __syncthreads();                            // the previous run's readers are done with hist
            const int64_t k0 = t0 - dmax;
            for (int i = threadIdx.x; i < span; i += kHsThreads) hist[i] = x.column(h, cd, k0 + i);
            __syncthreads();
        }
        double und[kHsPer];                             // the undelayed column at this lane's frames
#pragma unroll
        for (int j = 0; j < kHsPer; ++j) und[j] = x.column(h, cu, t0 + threadIdx.x + j * kHsThreads);

        for (int c = r0; c < r1; ++c) {
            const int32_t d = __builtin_amdgcn_readfirstlane(dl[c]);
            if (d < 0) continue;
            const int64_t len = x.n + d;
            if (t0 >= len) continue;                    // (uniform) pair c has no frame here
            PolarAcc64 acc;
#pragma unroll
            for (int j = 0; j < kHsPer; ++j) {
                const int64_t k = t0 + threadIdx.x + j * kHsThreads;
                if (k < len) {
                    const double del = staged ? hist[(k - t0) + (dmax - d)] : x.column(h, cd, k - d);
                    double v[2];
                    haas_frame(h, cu == 0 ? und[j] : del, cu == 0 ? del : und[j], v);
                    polar_add64(acc, v[0], v[1]);
                }
            }
            double v[kMoments];
            polar_values64(v, acc);
            hs_block_reduce(v, red);
            if (threadIdx.x == 0) {
                double *p = a.partials + ((int64_t)(f0 + c) * a.cap + blockIdx.x) * kMoments;
#pragma unroll
                for (int k = 0; k < kMoments; ++k) p[k] = v[k];
            }
        }
    }
}

__global__ __launch_bounds__(kHsThreads) void haas_scan_kernel(const HsArgs a) { hs_scan_body(a); }

// One workgroup per pair: lanes stride over its ceil((n + d) / kHsTile) partials, then the fixed tree.  A pair
// outside the contract (for HsArgs: signal outside [0, batch), negative delay, or more partials than the workspace
// holds) gets NaN moments.
template <class Args>
__device__ __forceinline__ void hs_reduce_body(const Args &a)
{
    __shared__ double red[kHsThreads / 64][kMoments];
    const int f = blockIdx.x;
    const int32_t d = a.delays[f];
    const int32_t s = a.signal(f);
    const bool ok = a.valid(s, d);
    const int64_t chunks = ok ? hs_chunks(a.open(s).n + d) : 0;
    double v[kMoments];
#pragma unroll
    for (int k = 0; k < kMoments; ++k) v[k] = 0.0;
    for (int64_t c = threadIdx.x; c < chunks; c += kHsThreads) {
        const double *p = a.partials + ((int64_t)f * a.cap + c) * kMoments;
#pragma unroll
        for (int k = 0; k < kMoments; ++k) v[k] = k == 4 ? fmax(v[k], p[k]) : v[k] + p[k];
    }
    hs_block_reduce(v, red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < kMoments; ++k) a.moments[(int64_t)f * kMoments + k] = ok ? v[k] : __builtin_nan("");
    }
}

__global__ __launch_bounds__(kHsThreads) void haas_scan_reduce_kernel(const HsArgs a) { hs_reduce_body(a); }

}  // namespace vnd

static_assert(VND_HAAS_SCAN_MAX_DELAYS == 65535 * vnd::kHsBlock, "the grid's y extent bounds the delays per call");
static_assert(VND_HAAS_PAIRS_MAX == 65535 * vnd::kHsBlock, "the grid's y extent bounds the pairs per call");

extern "C" {

static vnd_status haas_scan_check(int64_t n_frames, int32_t n_delays, int32_t in_channels, int32_t delayed_channel)
{
    if (n_frames < 0 || n_delays < 0) return fail(VND_ERR_INVALID, "negative frame or delay count");
    if (in_channels != 1 && in_channels != 2)
        return fail(VND_ERR_INVALID, "a Haas scan takes a mono or stereo signal, got %d channels", in_channels);
    if (delayed_channel != 0 && delayed_channel != 1)
        return fail(VND_ERR_INVALID, "delayed_channel must be 0 or 1, got %d", delayed_channel);
    if (n_delays > VND_HAAS_SCAN_MAX_DELAYS)
        return fail(VND_ERR_UNSUPPORTED, "more than %d delays per call: split them", VND_HAAS_SCAN_MAX_DELAYS);
    return VND_OK;
}

vnd_status vnd_haas_scan_workspace_bytes(int64_t n_frames, int32_t n_delays, int32_t max_delay, int64_t *bytes)
{
    if (!bytes) return fail(VND_ERR_INVALID, "null bytes");
    *bytes = 0;
    if (n_frames < 0 || n_delays < 0 || max_delay < 0)
        return fail(VND_ERR_INVALID, "negative frame count, delay count or delay");
    const int64_t chunks = (n_frames + max_delay + kHsTile - 1) / kHsTile;
    if (chunks > (1 << 23)) return fail(VND_ERR_UNSUPPORTED, "signal plus delay above %lld frames", (long long)kHsTile << 23);
    *bytes = chunks * n_delays * kMoments * (int64_t)sizeof(double);
    return VND_OK;
}

// Both _dev entries: validated scalars in, the two kernels enqueued on the caller's stream.
static vnd_status haas_pairs_launch(vnd_ctx *ctx, const float *x, int32_t batch, int64_t n_frames, int32_t in_channels,
                                    const int32_t *signals, const int32_t *delays, int32_t n_pairs,
                                    int32_t delayed_channel, int32_t ms_mode, int32_t use_width, double width,
                                    double *moments, void *workspace, int64_t workspace_bytes, void *stream_)
{
    if (workspace_bytes < 0) return fail(VND_ERR_INVALID, "negative workspace size");
    if (n_pairs == 0) return VND_OK;
    if (!delays || !moments || (n_frames > 0 && batch > 0 && !x))
        return fail(VND_ERR_INVALID, "null signal, delay or moments pointer");
    const int64_t per = (int64_t)n_pairs * kMoments * (int64_t)sizeof(double);
    const int64_t cap = std::min<int64_t>(workspace_bytes / per, 1 << 23);
    if (cap > 0 && !workspace) return fail(VND_ERR_INVALID, "null workspace");
    DeviceScope on(ctx->device);
    hipStream_t stream = (hipStream_t)stream_;
    HsArgs a{};
    a.h.x = x; a.h.n = n_frames; a.h.Cx = in_channels; a.h.delayed_channel = delayed_channel;
    a.h.ms = ms_mode ? 1 : 0; a.h.use_width = use_width ? 1 : 0; a.h.w_mid = 1.0 - width; a.h.w_side = width;
    a.signals = signals; a.delays = delays; a.partials = (double *)workspace; a.moments = moments; a.F = n_pairs;
    a.batch = batch; a.cap = cap;
    if (cap > 0)
        hipLaunchKernelGGL(haas_scan_kernel, dim3((unsigned)cap, (unsigned)((n_pairs + kHsBlock - 1) / kHsBlock)),
                           dim3(kHsThreads), 0, stream, a);
    hipLaunchKernelGGL(haas_scan_reduce_kernel, dim3((unsigned)n_pairs), dim3(kHsThreads), 0, stream, a);
    HIP_TRY(hipGetLastError());
    return VND_OK;
}

// Both _host entries after their checks, host pointers in: the arrays staged in `ws` bytes of partial sums and four more pieces
// (signals == null: the scan of one signal, no index array).
static vnd_status haas_pairs_host(vnd_ctx *ctx, const char *name, const float *x, int32_t batch, int64_t n_frames,
                                  int32_t in_channels, const int32_t *signals, const int32_t *delays, int32_t n_pairs,
                                  int32_t delayed_channel, int32_t ms_mode, int32_t use_width, double width, double *moments,
                                  int64_t ws)
{
    HostCall call(ctx);
    const size_t x_bytes = (size_t)batch * n_frames * in_channels * sizeof(float);
    const size_t i_bytes = (size_t)n_pairs * sizeof(int32_t), s_bytes = signals ? i_bytes : 0;
    const size_t m_bytes = (size_t)n_pairs * kMoments * sizeof(double);
    call.carve({(size_t)ws, m_bytes, s_bytes, i_bytes, x_bytes});
    double *m_dev = call.piece<double>(1);
    int32_t *s_dev = signals ? call.piece<int32_t>(2) : nullptr, *d_dev = call.piece<int32_t>(3);
    float *x_dev = call.piece<float>(4);
    call.up(x_dev, x, x_bytes, "x");
    call.up(s_dev, signals, s_bytes, "signals");
    call.up(d_dev, delays, i_bytes, "delays");
    call.run([&] { return haas_pairs_launch(ctx, x_dev, batch, n_frames, in_channels, s_dev, d_dev, n_pairs, delayed_channel,
                                            ms_mode, use_width, width, m_dev, call.piece<char>(0), ws, call.stream()); });
    call.down(moments, m_dev, m_bytes, "moments");
    return call.finish(name);
}

vnd_status vnd_haas_scan_f64_dev(vnd_ctx *ctx, const float *x, int64_t n_frames, int32_t in_channels,
                                 const int32_t *delays, int32_t n_delays, int32_t delayed_channel, int32_t ms_mode,
                                 int32_t use_width, double width, double *moments, void *workspace,
                                 int64_t workspace_bytes, void *stream_)
{
    if (!ctx) return fail(VND_ERR_INVALID, "null context");
    vnd_status st = haas_scan_check(n_frames, n_delays, in_channels, delayed_channel);
    if (st != VND_OK) return st;
    return haas_pairs_launch(ctx, x, 1, n_frames, in_channels, nullptr, delays, n_delays, delayed_channel, ms_mode,
                             use_width, width, moments, workspace, workspace_bytes, stream_);
}

vnd_status vnd_haas_scan_f64_host(vnd_ctx *ctx, const float *x, int64_t n_frames, int32_t in_channels,
                                  const int32_t *delays, int32_t n_delays, int32_t delayed_channel, int32_t ms_mode,
                                  int32_t use_width, double width, double *moments)
{
    if (!ctx) return fail(VND_ERR_INVALID, "null context");
    vnd_status st = haas_scan_check(n_frames, n_delays, in_channels, delayed_channel);
    if (st != VND_OK) return st;
    if (n_delays == 0) return VND_OK;
    if (!delays || !moments || (n_frames > 0 && !x)) return fail(VND_ERR_INVALID, "null signal, delay or moments pointer");
    int32_t dmax = 0;
    for (int32_t f = 0; f < n_delays; ++f) {
        if (delays[f] < 0) return fail(VND_ERR_INVALID, "delay %d of candidate %d is negative", delays[f], f);
        dmax = std::max(dmax, delays[f]);
    }
    int64_t ws = 0;
    st = vnd_haas_scan_workspace_bytes(n_frames, n_delays, dmax, &ws);
    if (st != VND_OK) return st;
    return haas_pairs_host(ctx, "vnd_haas_scan_f64_host", x, 1, n_frames, in_channels, nullptr, delays, n_delays, delayed_channel,
                           ms_mode, use_width, width, moments, ws);
}

// ---- include/vnd_haas_search.h: (signal, delay) pairs of a pool ----------------------------------------------------
static vnd_status haas_pairs_check(int32_t batch, int64_t n_frames, int32_t n_pairs, int32_t in_channels,
                                   int32_t delayed_channel)
{
    if (batch < 0 || n_frames < 0 || n_pairs < 0) return fail(VND_ERR_INVALID, "negative batch, frame or pair count");
    if (in_channels != 1 && in_channels != 2)
        return fail(VND_ERR_INVALID, "a Haas scan takes mono or stereo signals, got %d channels", in_channels);
    if (delayed_channel != 0 && delayed_channel != 1)
        return fail(VND_ERR_INVALID, "delayed_channel must be 0 or 1, got %d", delayed_channel);
    if (n_pairs > VND_HAAS_PAIRS_MAX)
        return fail(VND_ERR_UNSUPPORTED, "more than %d pairs per call: split them", VND_HAAS_PAIRS_MAX);
    if (n_frames > 0 && (int64_t)batch > INT64_MAX / 2 / n_frames)
        return fail(VND_ERR_UNSUPPORTED, "pool of %d x %lld frames too large", batch, (long long)n_frames);
    return VND_OK;
}

vnd_status vnd_haas_pairs_workspace_bytes(int64_t n_frames, int32_t n_pairs, int32_t max_delay, int64_t *bytes)
{
    return vnd_haas_scan_workspace_bytes(n_frames, n_pairs, max_delay, bytes);
}

vnd_status vnd_haas_pairs_f64_dev(vnd_ctx *ctx, const float *x, int32_t batch, int64_t n_frames, int32_t in_channels,
                                  const int32_t *signals, const int32_t *delays, int32_t n_pairs,
                                  int32_t delayed_channel, int32_t ms_mode, int32_t use_width, double width,
                                  double *moments, void *workspace, int64_t workspace_bytes, void *stream_)
{
    if (!ctx) return fail(VND_ERR_INVALID, "null context");
    vnd_status st = haas_pairs_check(batch, n_frames, n_pairs, in_channels, delayed_channel);
    if (st != VND_OK) return st;
    if (n_pairs > 0 && !signals) return fail(VND_ERR_INVALID, "null signal index pointer");
    return haas_pairs_launch(ctx, x, batch, n_frames, in_channels, signals, delays, n_pairs, delayed_channel, ms_mode,
                             use_width, width, moments, workspace, workspace_bytes, stream_);
}

vnd_status vnd_haas_pairs_f64_host(vnd_ctx *ctx, const float *x, int32_t batch, int64_t n_frames, int32_t in_channels,
                                   const int32_t *signals, const int32_t *delays, int32_t n_pairs,
                                   int32_t delayed_channel, int32_t ms_mode, int32_t use_width, double width,
                                   double *moments)
{
    if (!ctx) return fail(VND_ERR_INVALID, "null context");
    vnd_status st = haas_pairs_check(batch, n_frames, n_pairs, in_channels, delayed_channel);
    if (st != VND_OK) return st;
    if (n_pairs == 0) return VND_OK;
    if (!signals || !delays || !moments || (n_frames > 0 && batch > 0 && !x))
        return fail(VND_ERR_INVALID, "null signal, signal index, delay or moments pointer");
    int32_t dmax = 0;
    for (int32_t p = 0; p < n_pairs; ++p) {
        if (signals[p] < 0 || signals[p] >= batch)
            return fail(VND_ERR_INVALID, "signal %d of pair %d is outside [0, %d)", signals[p], p, batch);
        if (delays[p] < 0) return fail(VND_ERR_INVALID, "delay %d of pair %d is negative", delays[p], p);
        dmax = std::max(dmax, delays[p]);
    }
    int64_t ws = 0;
    st = vnd_haas_pairs_workspace_bytes(n_frames, n_pairs, dmax, &ws);
    if (st != VND_OK) return st;
    return haas_pairs_host(ctx, "vnd_haas_pairs_f64_host", x, batch, n_frames, in_channels, signals, delays, n_pairs,
                           delayed_channel, ms_mode, use_width, width, moments, ws);
}

}  // extern "C"

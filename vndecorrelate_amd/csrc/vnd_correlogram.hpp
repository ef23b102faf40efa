// vnd_correlogram.hpp - the reference's cross_correlogram (utils/dsp.py:313-356) on the device: windowed, normalised
// np.correlate(x_w, y_w, 'full') of many streams at once (include/vnd_analysis.h).
// (one translation unit: included by vnd_amd.hip after vnd_dense.hpp; everything static here is private to the library)
#pragma once
#include "../../include/vnd_analysis.h"

// Numerics.  One window's full correlation is a dense FIR: with h[k] = y_w[W-1-k] and x_w = 0 outside [0, W),
// num[j] = sum over k of h[k] * x_w[j - k].  Each num[j] is one float64 FMA chain over k ascending of the exact products
// f64(h) * f64(x), rounded once to float32; taps that reach the zero padding add an exact 0, so the chain is the same
// whatever the tiling.  Exx, Eyy: float64 sums (a fixed lane-strided split and a butterfly), each rounded once.  The
// normaliser is float32 as NumPy 2 computes it (weak Python-float eps): d = f32(sqrtf(f32(Exx * Eyy)) + eps), out = num / d,
// all correctly rounded, f32 denormals kept (the library is built without flush-to-zero).
//
// Form (FP64-bound: W^2 useful FMAs per window against 4 (2W - 1) bytes of output).  A workgroup of 4 waves owns kCgG = 4
// consecutive windows of one stream and kCgTile = 1024 consecutive lag columns of each; wave q takes columns
// [256 q, 256 q + 256) of the tile, lanes 16 g .. 16 g + 15 of it window g, each lane kCgR = 16 consecutive columns in 16
// float64 accumulators.  Four windows per wave rather than one keeps a wave's column span at 256: the taps a wave runs are
// the union over its columns (the triangle of useful work is trimmed per wave), so a narrow span wastes little of it
// (W = 882: 78 % of the FMAs run are useful, against 46 % with one window per wave).  As in vnd_dense.hpp, x is staged in
// LDS as float32 (zeros outside the window) and slides through two 16-value float64 register arrays, 16 new values (four
// ds_read_b128) per block of 16 taps and 256 v_fma_f64; h is staged per chunk of kCgTaps taps as float64 and read by
// its 16 lanes with one broadcast address per window (512-tap chunks: 41 KB of LDS, 3 workgroups per CU, as the VGPRs
// allow).  Columns past 2W - 1 are zero stores; the energies are computed by the same workgroup (wave g: window g), so the
// kernel needs no workspace and no second pass.
constexpr int kCgThreads = 256;
constexpr int kCgR = 16;                                      // columns per lane, taps per block
constexpr int kCgG = 4;                                       // windows per workgroup (and per wave)
constexpr int kCgSpan = (64 / kCgG) * kCgR;                   // 256 columns per wave and window
constexpr int kCgTile = (kCgThreads / 64) * kCgSpan;          // 1024 columns per workgroup and window
constexpr int kCgTaps = 512;                                  // taps per staged chunk: a multiple of kCgR
static_assert(VND_CORRELOGRAM_MAX_WINDOW <= (1 << 20), "int32 column arithmetic");

struct CgArgs {
    const float *__restrict__ x;
    const float *__restrict__ y;
    float *__restrict__ out;          // [batch][windows][num_lags]
    int64_t windows, stream_stride;
    int64_t group0;                   // first window group of this launch
    int32_t frame_stride, W, hop, num_lags, jmax;   // jmax = min(num_lags, 2W - 1)
    int32_t tiles;                    // column tiles per window group
    float eps;
};

// The sample sources of correlogram_kernel: the one place it reads x and y.  A source names the kernel's argument
// type (Args; cg(a) is its CgArgs) and, per window ww of stream b, gives a Run of the window's W consecutive frames:
// run.x(i) and run.y(i), i in [0, W).  slot0 is the ring slot of the window's first frame
// (slot0_of(a, ww): one 64-bit modulo per window, not per sample); a source without a ring ignores it.  prologue(a, b)
// runs first in every workgroup; false ends the workgroup.
// What the body takes from the launch comes through the source too: view(args) is what every other hook is handed - the
// kernel's arguments themselves for a source whose launch is uniform, a per-workgroup copy built from device memory for
// one whose is not (vnd_correlogram_voice_stream.hpp) - cg(view) carries the row count (windows) and the base of the
// rows (out) the workgroup writes, and stream / group / tile are its coordinates.
__device__ __forceinline__ int64_t cg_grid_group(const CgArgs &a) { return a.group0 + blockIdx.x / (unsigned)a.tiles; }
__device__ __forceinline__ int cg_grid_tile(const CgArgs &a) { return (int)(blockIdx.x % (unsigned)a.tiles); }

struct CgSignal {                               // the one-shot call: x[b * stream_stride + f * frame_stride]
    using Args = CgArgs;
    static constexpr bool kRing = false;
    struct Run {
        const float *px, *py;
        int64_t bs, f0;               // b * stream_stride, the window's first frame
        int32_t fs;
        __device__ __forceinline__ float x(int i) const { return px[bs + (f0 + i) * (int64_t)fs]; }
        __device__ __forceinline__ float y(int i) const { return py[bs + (f0 + i) * (int64_t)fs]; }
    };
    using View = const Args &;
    __device__ static __forceinline__ View view(const Args &a) { return a; }
    __device__ static __forceinline__ const CgArgs &cg(const Args &a) { return a; }
    __device__ static __forceinline__ int64_t stream(const Args &) { return blockIdx.y; }
    __device__ static __forceinline__ int64_t group(const Args &a) { return cg_grid_group(a); }
    __device__ static __forceinline__ int tile(const Args &a) { return cg_grid_tile(a); }
    __device__ static __forceinline__ bool prologue(const Args &, int64_t) { return true; }
    __device__ static __forceinline__ int64_t slot0_of(const Args &, int64_t) { return 0; }
    __device__ static __forceinline__ Run run(const Args &a, int64_t b, int64_t ww, int64_t)
    {
        return Run{a.x, a.y, b * a.stream_stride, ww * a.hop, a.frame_stride};
    }
};

__device__ __forceinline__ void cg_load(double (&v)[kCgR], const float *p)
{
#pragma unroll
    for (int q = 0; q < kCgR / 4; ++q) {
        const float4 f = reinterpret_cast<const float4 *>(p)[q];
        v[4 * q + 0] = (double)f.x; v[4 * q + 1] = (double)f.y; v[4 * q + 2] = (double)f.z; v[4 * q + 3] = (double)f.w;
    }
}

// One block of 16 taps k0 + i (i ascending); column j of the lane takes x at window offset 15 - i + j: lo[15 - i + j]
// below 16, hi[-1 - i + j] from there.  hp: the block's 16 taps in LDS.
__device__ __forceinline__ void cg_block(double (&acc)[kCgR], const double (&lo)[kCgR], const double (&hi)[kCgR],
                                         const double *hp)
{
#pragma unroll
    for (int i = 0; i < kCgR; ++i) {
        const double hk = hp[i];
#pragma unroll
        for (int j = 0; j < kCgR; ++j) {
            const int m = kCgR - 1 - i + j;
            acc[j] = fma(hk, m < kCgR ? lo[m] : hi[m - kCgR], acc[j]);
        }
    }
}

template <class Src>
__global__ __launch_bounds__(kCgThreads) void correlogram_kernel(const typename Src::Args args)
{
    typename Src::View sa = Src::view(args);
    const CgArgs &a = Src::cg(sa);
    __shared__ __align__(16) float xs[kCgG][kCgTile + kCgTaps];
    __shared__ __align__(16) double hs[kCgG][kCgTaps];
    __shared__ float en[kCgG][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane >> 4;                                    // the lane's window in the group
    const int64_t group = Src::group(sa);
    const int T0 = Src::tile(sa) * kCgTile;
    const int64_t b = Src::stream(sa);
    const int64_t w = group * kCgG + g;                         // the lane's window
    const int t0 = wave * kCgSpan + (lane & 15) * kCgR;         // the lane's first column, relative to T0
    const int W = a.W;
    float *__restrict__ orow = a.out + (b * a.windows + w) * (int64_t)a.num_lags;
    __shared__ int64_t slot0[kCgG];                             // (a ring source: the ring slot of each window's frame 0)
    if (!Src::prologue(sa, b)) return;

    if (T0 >= a.jmax) {                                         // a tile of trailing zero columns only
        if (w < a.windows)
#pragma unroll
            for (int j = 0; j < kCgR; ++j) {
                const int col = T0 + t0 + j;
                if (col < a.num_lags) orow[col] = 0.0f;
            }
        return;
    }

    // the energies of window `wave` of the group: lane-strided float64 FMA chains, then a butterfly (every lane ends
    // with the same bits: each step adds the same two values in either order)
    {
        const int64_t ww = group * kCgG + wave;
        double ex = 0.0, ey = 0.0;
        if (ww < a.windows) {
            const int64_t s0 = Src::slot0_of(sa, ww);
            if (Src::kRing && lane == 0) slot0[wave] = s0;     // read by the staging loops after the next barrier
            const typename Src::Run r = Src::run(sa, b, ww, s0);
            for (int i = lane; i < W; i += 64) {
                const double xv = (double)r.x(i), yv = (double)r.y(i);
                ex = fma(xv, xv, ex);
                ey = fma(yv, yv, ey);
            }
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            ex += __shfl_xor(ex, m, 64);
            ey += __shfl_xor(ey, m, 64);
        }
        if (lane == 0) { en[wave][0] = (float)ex; en[wave][1] = (float)ey; }
    }

    double acc[kCgR];
#pragma unroll
    for (int j = 0; j < kCgR; ++j) acc[j] = 0.0;

    // taps of the workgroup and of this wave: column j has taps [max(0, j - W + 1), min(W - 1, j)]; columns >= jmax
    // are not computed
    const int lastcol = min(T0 + kCgTile, a.jmax) - 1;
    const int kA = max(0, T0 - W + 1), kB = min(W - 1, lastcol);
    const int J0 = T0 + wave * kCgSpan;
    const int kAq = max(0, J0 - W + 1), kBq = J0 >= a.jmax ? -1 : min(W - 1, min(J0 + kCgSpan, a.jmax) - 1);

    for (int kc0 = kA; kc0 <= kB; kc0 += kCgTaps) {
        const int kc_end = min(kc0 + kCgTaps, kB + 1);
        const int L = kc_end - kc0;
        const int Lr = (L + kCgR - 1) & ~(kCgR - 1);
        // xs[g][s] = x_w[gbase + s], s < kCgTile + Lr: tap k of column T0 + t reads s = t + (kc_end - 1 - k), at most
        // kCgTile - 1 + Lr.  hs[g][p] = h[kc_end - Lr + p] for p < Lr, 0 below kc0 (the bottom block's taps of the
        // previous chunk: they add an exact 0 here).
        const int gbase = T0 - (kc_end - 1);
        __syncthreads();                                        // the previous chunk's reads are done
        for (int e = threadIdx.x; e < kCgG * (kCgTile + Lr); e += kCgThreads) {
            const int gg = e / (kCgTile + Lr), s = e - gg * (kCgTile + Lr);
            const int64_t ww = group * kCgG + gg;
            const int i = gbase + s;
            float v = 0.0f;
            if (ww < a.windows && i >= 0 && i < W)
                v = Src::run(sa, b, ww, Src::kRing ? slot0[gg] : 0).x(i);
            xs[gg][s] = v;
        }
        for (int e = threadIdx.x; e < kCgG * Lr; e += kCgThreads) {
            const int gg = e / Lr, p = e - gg * Lr;
            const int64_t ww = group * kCgG + gg;
            const int k = kc_end - Lr + p;
            double v = 0.0;
            if (ww < a.windows && k >= kc0)
                v = (double)Src::run(sa, b, ww, Src::kRing ? slot0[gg] : 0).y(W - 1 - k);
            hs[gg][p] = v;
        }
        __syncthreads();
        // this wave's blocks: block U covers taps [kc_end - 16 - U, kc_end - U); keep those that meet [kAq, kBq]
        // (wave-uniform bounds), from the top of the window down (U descending = k ascending)
        const int uTop = min(Lr - kCgR, kc_end - 1 - kAq);
        const int uBot = max(0, kc_end - kCgR - kBq);
        if (kAq > kBq || uTop < uBot) continue;
        const int Uhi = uTop & ~(kCgR - 1);
        const int Ulo = (uBot + kCgR - 1) & ~(kCgR - 1);
        if (Uhi < Ulo) continue;
        const float *xw = xs[g] + t0;
        const double *hw = hs[g] + (Lr - kCgR);
        double A[kCgR], B[kCgR];
        int U = Uhi;
        cg_load(A, xw + U);
        cg_load(B, xw + U + kCgR);
        cg_block(acc, A, B, hw - U);
        int left = (U - Ulo) / kCgR;                            // blocks below the top one
        for (; left >= 2; left -= 2) {
            U -= kCgR;
            cg_load(B, xw + U);
            cg_block(acc, B, A, hw - U);
            U -= kCgR;
            cg_load(A, xw + U);
            cg_block(acc, A, B, hw - U);
        }
        if (left) {
            U -= kCgR;
            cg_load(B, xw + U);
            cg_block(acc, B, A, hw - U);
        }
    }
    __syncthreads();                                            // en[] is written
    if (w >= a.windows) return;
    // sqrtf, not __fsqrt_rn: on gfx950 the latter is the bare v_sqrt_f32 (not correctly rounded); sqrtf adds the fix-up
    const float d = __fadd_rn(sqrtf(__fmul_rn(en[g][0], en[g][1])), a.eps);
#pragma unroll
    for (int j = 0; j < kCgR; ++j) {
        const int col = T0 + t0 + j;
        if (col < a.num_lags) orow[col] = col < a.jmax ? __fdiv_rn((float)acc[j], d) : 0.0f;
    }
}

extern "C" {

vnd_status vnd_correlogram_f32_dev(vnd_ctx *ctx, const float *x, const float *y, float *out, int64_t batch,
                                   int64_t n_frames, int64_t stream_stride, int32_t frame_stride, int32_t window,
                                   int32_t hop, int32_t num_lags, float eps, void *stream_)
{
    if (!ctx) return fail(VND_ERR_INVALID, "null context");
    if (batch < 1 || n_frames < 1 || stream_stride < 1 || frame_stride < 1 || window < 1 || hop < 1 || num_lags < 1)
        return fail(VND_ERR_INVALID, "batch, n_frames, strides, window, hop and num_lags must be >= 1");
    if (!x || !y || !out) return fail(VND_ERR_INVALID, "null signal or output pointer");
    if (window > VND_CORRELOGRAM_MAX_WINDOW)
        return fail(VND_ERR_UNSUPPORTED, "window %d above the %d-sample cap", window, VND_CORRELOGRAM_MAX_WINDOW);
    const int64_t windows = n_frames >= window ? (n_frames - window) / hop + 1 : 0;
    // extents in floats: the last sample of the last stream, and the output
    int64_t span, xlast, rows, outn;
    if (__builtin_mul_overflow(batch - 1, stream_stride, &span) ||
        __builtin_mul_overflow(n_frames - 1, (int64_t)frame_stride, &xlast) || __builtin_add_overflow(span, xlast, &span) ||
        __builtin_mul_overflow(batch, windows, &rows) || __builtin_mul_overflow(rows, (int64_t)num_lags, &outn) ||
        span > INT64_MAX / 8 || outn > INT64_MAX / 8)
        return fail(VND_ERR_INVALID, "buffer extents overflow");
    if (windows == 0) return VND_OK;
    const int64_t xb = (span + 1) * (int64_t)sizeof(float), ob = outn * (int64_t)sizeof(float);
    const char *o0 = (const char *)out;
    for (const float *p : {x, y}) {
        const char *p0 = (const char *)p;
        if (p0 < o0 + ob && o0 < p0 + xb) return fail(VND_ERR_INVALID, "out must not overlap x or y");
    }
    DeviceScope on(ctx->device);
    hipStream_t stream = (hipStream_t)stream_;

    CgArgs c{};
    c.x = x; c.y = y; c.out = out; c.windows = windows; c.stream_stride = stream_stride;
    c.frame_stride = frame_stride; c.W = window; c.hop = hop; c.num_lags = num_lags;
    c.jmax = (int32_t)std::min<int64_t>(num_lags, 2 * (int64_t)window - 1);
    c.tiles = (int32_t)((num_lags + kCgTile - 1) / kCgTile);
    c.eps = eps;
    // a dispatch counts its work-items in 32 bits: at most 2^23 workgroups per launch in x, VND_MAX_STREAMS in y
    const int64_t groups = (windows + kCgG - 1) / kCgG;
    const int64_t per_launch = std::max<int64_t>(1, ((int64_t)1 << 23) / c.tiles);
    for (int64_t b0 = 0; b0 < batch; b0 += VND_MAX_STREAMS) {
        const int64_t nb = std::min<int64_t>(VND_MAX_STREAMS, batch - b0);
        CgArgs s = c;
        s.x = x + b0 * stream_stride; s.y = y + b0 * stream_stride; s.out = out + b0 * windows * (int64_t)num_lags;
        for (int64_t g0 = 0; g0 < groups; g0 += per_launch) {
            s.group0 = g0;
            const int64_t ng = std::min(per_launch, groups - g0);
            hipLaunchKernelGGL(correlogram_kernel<CgSignal>, dim3((unsigned)(ng * c.tiles), (unsigned)nb), dim3(kCgThreads), 0, stream, s);
        }
    }
    HIP_TRY(hipGetLastError());
    return VND_OK;
}

}  // extern "C"

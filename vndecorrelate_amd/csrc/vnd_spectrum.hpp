// vnd_spectrum.hpp - short-time spectra of a pool (include/vnd_spectrum.h): scipy.signal.spectrogram's power columns and the
// Welch sums Pxx, Pyy, Pxy, by a batched real-input FFT in LDS.
// (one translation unit: included by vnd_amd.hip after vnd_level.hpp; it reuses vnd_scope.hpp's overlap test and limits)
//
// A workgroup of 256 threads owns a run of consecutive segments of one signal - of one channel (spectrogram_kernel) or of
// both (cross_spectra_kernel).  It
//   1. stages the union of the run's frames in LDS, once: with hop < nperseg a frame belongs to nperseg / hop segments;
//   2. transforms the run in passes of G = 2048 / (nfft / 2) segments, each segment on its own slot of N = nfft / 2 complex
//      points: the mean (float64, a fixed tree over 256 / G threads a segment), (x - mean) * window into the slot - even
//      samples real, odd imaginary - then the Stockham stages, every pass 512 radix-4 (1024 radix-2) butterflies, two (four)
//      a thread, read into registers, barrier, written back to the same array in autosort order, barrier;
//   3. forms each bin by the split step X[k] = E[k] + w^k O[k] from Z[k] and conj(Z[N - k]);
//   4. spectrogram: writes the powers into a [bin][segment] tile and, after the run, stores the tile with the segment on the
//      lane: a wave stores consecutive t of a bin;
//      cross spectra: thread k adds bin k's powers and products of the pass to float64 registers in ascending t, and stores the
//      run's sums to work memory; cross_finish_kernel adds the runs in ascending order, divides and rounds once.
// A segment's arithmetic does not depend on its slot, its run or its neighbours: every column is the one-segment call's, bit
// for bit.
//
// LDS layout: re and im of the points are two arrays of the sample type (4- or 8-byte accesses, never a
// pair), point e at e + 5 * (e >> 5): five pad elements after every 32 points.  A stage reads 32 consecutive points a
// half-wave (conflict-free) and writes runs of Ns points 4 Ns apart, which unpadded fall 4 deep on a bank for Ns <= 8; the
// odd shift a row of 32 leaves every stage of every nfft, float32 and float64, at most 2 deep by the bank rule.
//
// Every index that is built from device data: n_each[b] alone - spectrum_segments clamps it to [0, n_frames] before the segment
// count is formed, and a workgroup stages, transforms and reads only segments below that count.
#pragma once
#include "../../include/vnd_spectrum.h"

constexpr int kSpectrumThreads = 256;
constexpr int kSpectrumCap = 2048;                                    // complex points of one pass
constexpr int kSpectrumZ = kSpectrumCap + 5 * (kSpectrumCap >> 5);            // ... padded
constexpr int kSpectrumLdsBytes = 156 * 1024;                         // dynamic LDS of a workgroup; 2 KiB more are static
constexpr int kSpectrumBinsPerThread = (VND_SPECTRUM_MAX_NFFT / 2 + 1 + kSpectrumThreads - 1) / kSpectrumThreads;

template <class T>
struct SpectrumArgs {
    const T *__restrict__ x;
    const T *__restrict__ win;              // [nperseg]
    const T *__restrict__ tw;               // [nfft][2]
    const int32_t *__restrict__ n_each;
    int64_t n_frames, stream_stride, segments;                    // segments: the pool's columns
    int64_t groups;                                               // runs a signal: ceil(segments / run)
    int32_t frame_stride, channels, nperseg, hop, nfft, log_n, detrend, run;
    T scale;
    T *__restrict__ sxx;
    T *__restrict__ pxx;
    T *__restrict__ pyy;
    T *__restrict__ pxy;
    double *__restrict__ work;              // [batch][groups][F][1 or 4]
    int64_t batch;
};

__device__ __forceinline__ int spectrum_pad(int e) { return e + 5 * (e >> 5); }

template <class T>
__device__ __forceinline__ int64_t spectrum_segments(const SpectrumArgs<T> &a, int64_t b)
{
    int64_t m = a.n_frames;
    if (a.n_each) {
        const int32_t v = a.n_each[b];
        m = (v >= 0 && (int64_t)v <= a.n_frames) ? (int64_t)v : 0;
    }
    return m >= a.nperseg ? (m - a.nperseg) / a.hop + 1 : 0;
}

// Segments gb .. gb + G - 1 of the staged run (those below nseg), transformed: Z of slot g at points g * N .. g * N + N - 1.
// Called by every thread of the workgroup; the points are complete, and visible, when it returns.
template <class T>
__device__ void spectrum_transform(const SpectrumArgs<T> &a, T *__restrict__ zre, T *__restrict__ zim, const T *__restrict__ stage,
                               int gb, int nseg, double *red)
{
    const int tid = threadIdx.x;
    const int ln = a.log_n, N = 1 << ln;
    const int G = kSpectrumCap >> ln, P = kSpectrumThreads / G;           // G in 1..64, P in 4..256
    if (a.detrend) {
        const int g = tid / P, p = tid - g * P;
        double s = 0.0;
        if (gb + g < nseg) {
            const T *seg = stage + (gb + g) * a.hop;
            for (int i = p; i < a.nperseg; i += P) s += (double)seg[i];
        }
        red[tid] = s;
        for (int h = P >> 1; h > 0; h >>= 1) {
            __syncthreads();
            if (p < h) red[tid] += red[tid + h];
        }
        __syncthreads();
    }
    for (int e = tid; e < kSpectrumCap; e += kSpectrumThreads) {
        const int g = e >> ln, k = e & (N - 1);
        T v0 = (T)0, v1 = (T)0;
        if (gb + g < nseg) {
            const T *seg = stage + (gb + g) * a.hop;
            const T mean = a.detrend ? (T)(red[g * P] / (double)a.nperseg) : (T)0;
            const int i0 = 2 * k;
            if (i0 < a.nperseg) v0 = (seg[i0] - mean) * a.win[i0];
            if (i0 + 1 < a.nperseg) v1 = (seg[i0 + 1] - mean) * a.win[i0 + 1];
        }
        zre[spectrum_pad(e)] = v0;
        zim[spectrum_pad(e)] = v1;
    }
    __syncthreads();

    int ns = 1;
    if (ln & 1) {                                                 // the radix-2 stage: Ns = 1, no twiddle
        T r0[4], i0[4], r1[4], i1[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int bf = tid + u * kSpectrumThreads;
            const int g = bf >> (ln - 1), j = bf & ((N >> 1) - 1);
            const int in0 = (g << ln) + j, in1 = in0 + (N >> 1);
            r0[u] = zre[spectrum_pad(in0)]; i0[u] = zim[spectrum_pad(in0)];
            r1[u] = zre[spectrum_pad(in1)]; i1[u] = zim[spectrum_pad(in1)];
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int bf = tid + u * kSpectrumThreads;
            const int g = bf >> (ln - 1), j = bf & ((N >> 1) - 1);
            const int o0 = (g << ln) + 2 * j, o1 = o0 + 1;
            zre[spectrum_pad(o0)] = r0[u] + r1[u]; zim[spectrum_pad(o0)] = i0[u] + i1[u];
            zre[spectrum_pad(o1)] = r0[u] - r1[u]; zim[spectrum_pad(o1)] = i0[u] - i1[u];
        }
        __syncthreads();
        ns = 2;
    }
    for (; ns < N; ns <<= 2) {
        T vr[2][4], vi[2][4];
        const int quarter = N >> 2;
        const int step = a.nfft / (ns << 2);                      // the twiddle of (r, k) is tw[r * k * step]
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int bf = tid + u * kSpectrumThreads;
            const int g = bf >> (ln - 2), j = bf & (quarter - 1), k = j & (ns - 1);
            const int in0 = (g << ln) + j;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const T xr = zre[spectrum_pad(in0 + r * quarter)], xi = zim[spectrum_pad(in0 + r * quarter)];
                if (r == 0 || ns == 1) {
                    vr[u][r] = xr; vi[u][r] = xi;
                } else {
                    const T wr = a.tw[2 * (r * k * step)], wi = a.tw[2 * (r * k * step) + 1];
                    const T m0 = xr * wr, m1 = xi * wi, m2 = xr * wi, m3 = xi * wr;
                    vr[u][r] = m0 - m1; vi[u][r] = m2 + m3;
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int bf = tid + u * kSpectrumThreads;
            const int g = bf >> (ln - 2), j = bf & (quarter - 1), k = j & (ns - 1);
            const int o0 = (g << ln) + ((j - k) << 2) + k;
            const T t0r = vr[u][0] + vr[u][2], t0i = vi[u][0] + vi[u][2];
            const T t1r = vr[u][0] - vr[u][2], t1i = vi[u][0] - vi[u][2];
            const T t2r = vr[u][1] + vr[u][3], t2i = vi[u][1] + vi[u][3];
            const T dr = vr[u][1] - vr[u][3], di = vi[u][1] - vi[u][3];      // times -i: (di, -dr)
            zre[spectrum_pad(o0)] = t0r + t2r;          zim[spectrum_pad(o0)] = t0i + t2i;
            zre[spectrum_pad(o0 + ns)] = t1r + di;      zim[spectrum_pad(o0 + ns)] = t1i - dr;
            zre[spectrum_pad(o0 + 2 * ns)] = t0r - t2r; zim[spectrum_pad(o0 + 2 * ns)] = t0i - t2i;
            zre[spectrum_pad(o0 + 3 * ns)] = t1r - di;  zim[spectrum_pad(o0 + 3 * ns)] = t1i + dr;
        }
        __syncthreads();
    }
}

// Bin k (0 .. N) of the segment whose points start at `base`: the split step of the real-input transform.
template <class T>
__device__ __forceinline__ void spectrum_bin(const SpectrumArgs<T> &a, const T *__restrict__ zre, const T *__restrict__ zim, int base,
                                         int k, T &xr, T &xi)
{
    const int N = 1 << a.log_n;
    const int k0 = base + (k & (N - 1)), k1 = base + ((N - k) & (N - 1));
    const T zr = zre[spectrum_pad(k0)], zi = zim[spectrum_pad(k0)];
    const T cr = zre[spectrum_pad(k1)], ci = -zim[spectrum_pad(k1)];
    const T er = (T)0.5 * (zr + cr), ei = (T)0.5 * (zi + ci);
    const T pr = (T)0.5 * (zi - ci), pi = (T)-0.5 * (zr - cr);      // O[k] = (Z[k] - conj(Z[N - k])) / 2i
    const T wr = a.tw[2 * k], wi = a.tw[2 * k + 1];
    const T m0 = wr * pr, m1 = wi * pi, m2 = wr * pi, m3 = wi * pr;
    xr = er + (m0 - m1);
    xi = ei + (m2 + m3);
}

template <class T>
__device__ __forceinline__ T spectrum_scaled(const SpectrumArgs<T> &a, T v, int k)
{
    const T s = v * a.scale;
    return (k == 0 || k == (1 << a.log_n)) ? s : s * (T)2;
}

// grid = batch * channels * groups workgroups; dynamic LDS: the points, the staged frames, the [bin][segment] tile
template <class T>
__global__ __launch_bounds__(kSpectrumThreads) void spectrogram_kernel(const SpectrumArgs<T> a)
{
    extern __shared__ __attribute__((aligned(16))) double spectrum_lds[];
    __shared__ double red[kSpectrumThreads];
    const int tid = threadIdx.x;
    const int N = 1 << a.log_n, F = N + 1, G = kSpectrumCap >> a.log_n;
    const int64_t bc = (int64_t)blockIdx.x / a.groups, b = bc / a.channels;
    const int c = (int)(bc - b * a.channels);
    const int64_t t0 = ((int64_t)blockIdx.x - bc * a.groups) * a.run;
    const int64_t segs = spectrum_segments(a, b);
    const int cols = (int)((a.segments - t0 < a.run) ? a.segments - t0 : a.run);        // columns written: >= 1 by the grid
    const int64_t left = segs - t0;
    const int nseg = left <= 0 ? 0 : (left < cols ? (int)left : cols);                  // ... of which are the signal's
    T *zre = (T *)spectrum_lds, *zim = zre + kSpectrumZ, *stage = zim + kSpectrumZ;
    T *tile = stage + ((a.run - 1) * a.hop + a.nperseg);
    const int pitch = a.run | 1;
    if (nseg > 0) {                                               // (workgroup-uniform)
        const int span = (nseg - 1) * a.hop + a.nperseg;
        const T *__restrict__ src = a.x + b * a.stream_stride + c + t0 * a.hop * (int64_t)a.frame_stride;
        for (int i = tid; i < span; i += kSpectrumThreads) stage[i] = src[(int64_t)i * a.frame_stride];
        __syncthreads();
        for (int gb = 0; gb < nseg; gb += G) {
            spectrum_transform(a, zre, zim, stage, gb, nseg, red);
            const int cnt = nseg - gb < G ? nseg - gb : G;
            for (int e = tid; e < cnt * F; e += kSpectrumThreads) {
                const int g = e / F, k = e - g * F;
                T xr, xi;
                spectrum_bin(a, zre, zim, g << a.log_n, k, xr, xi);
                const T m0 = xr * xr, m1 = xi * xi;
                tile[k * pitch + gb + g] = spectrum_scaled(a, m0 + m1, k);
            }
            __syncthreads();
        }
    }
    T *__restrict__ out = a.sxx + bc * F * a.segments + t0;
    for (int e = tid; e < F * cols; e += kSpectrumThreads) {
        const int k = e / cols, r = e - k * cols;
        out[(int64_t)k * a.segments + r] = r < nseg ? tile[k * pitch + r] : (T)0;
    }
}

// grid = batch * groups workgroups; dynamic LDS: the points, (stereo) the left spectra of a pass, the staged frames
template <class T, int CH>
__global__ __launch_bounds__(kSpectrumThreads) void cross_spectra_kernel(const SpectrumArgs<T> a)
{
    constexpr int Q = CH == 2 ? 4 : 1;
    extern __shared__ __attribute__((aligned(16))) double spectrum_lds[];
    __shared__ double red[kSpectrumThreads];
    const int tid = threadIdx.x;
    const int N = 1 << a.log_n, F = N + 1, G = kSpectrumCap >> a.log_n;
    const int64_t b = (int64_t)blockIdx.x / a.groups, run = (int64_t)blockIdx.x - b * a.groups;
    const int64_t t0 = run * a.run;
    const int64_t left = spectrum_segments(a, b) - t0;
    if (left <= 0) return;                                        // (workgroup-uniform, before any barrier)
    const int nseg = left < a.run ? (int)left : a.run;
    T *zre = (T *)spectrum_lds, *zim = zre + kSpectrumZ;
    T *xlr = zim + kSpectrumZ, *xli = xlr + (CH == 2 ? kSpectrumZ : 0);
    T *stage = xli + (CH == 2 ? kSpectrumZ : 0);
    const int room = (a.run - 1) * a.hop + a.nperseg;             // a channel's staged frames
    const int span = (nseg - 1) * a.hop + a.nperseg;
    const T *__restrict__ src = a.x + b * a.stream_stride + t0 * a.hop * (int64_t)a.frame_stride;
    for (int e = tid; e < span * CH; e += kSpectrumThreads) {
        const int i = e / CH, c = e - i * CH;
        stage[c * room + i] = src[(int64_t)i * a.frame_stride + c];
    }
    __syncthreads();
    double acc[kSpectrumBinsPerThread][Q];
#pragma unroll
    for (int i = 0; i < kSpectrumBinsPerThread; ++i)
#pragma unroll
        for (int q = 0; q < Q; ++q) acc[i][q] = 0.0;
    for (int gb = 0; gb < nseg; gb += G) {
        const int cnt = nseg - gb < G ? nseg - gb : G;
        spectrum_transform(a, zre, zim, stage, gb, nseg, red);
        if (CH == 2) {
            for (int e = tid; e < cnt * F; e += kSpectrumThreads) {
                const int g = e / F, k = e - g * F;
                T xr, xi;
                spectrum_bin(a, zre, zim, g << a.log_n, k, xr, xi);
                xlr[e] = xr;
                xli[e] = xi;
            }
            __syncthreads();
            spectrum_transform(a, zre, zim, stage + room, gb, nseg, red);
        }
#pragma unroll
        for (int i = 0; i < kSpectrumBinsPerThread; ++i) {
            const int k = tid + i * kSpectrumThreads;
            if (k >= F) continue;
            for (int g = 0; g < cnt; ++g) {                       // ascending t
                T xr, xi;
                spectrum_bin(a, zre, zim, g << a.log_n, k, xr, xi);
                const T m0 = xr * xr, m1 = xi * xi;
                if (CH == 1) {
                    acc[i][0] += (double)spectrum_scaled(a, m0 + m1, k);
                } else {
                    const T lr = xlr[g * F + k], li = xli[g * F + k];
                    const T l0 = lr * lr, l1 = li * li;
                    const T c0 = lr * xr, c1 = li * xi, c2 = lr * xi, c3 = li * xr;
                    acc[i][0] += (double)spectrum_scaled(a, l0 + l1, k);
                    acc[i][Q > 1 ? 1 : 0] += (double)spectrum_scaled(a, m0 + m1, k);
                    acc[i][Q > 2 ? 2 : 0] += (double)spectrum_scaled(a, c0 + c1, k);         // conj(X_L) * X_R
                    acc[i][Q > 3 ? 3 : 0] += (double)spectrum_scaled(a, c2 - c3, k);
                }
            }
        }
        __syncthreads();
    }
    double *__restrict__ w = a.work + (b * a.groups + run) * F * Q;
#pragma unroll
    for (int i = 0; i < kSpectrumBinsPerThread; ++i) {
        const int k = tid + i * kSpectrumThreads;
        if (k >= F) continue;
#pragma unroll
        for (int q = 0; q < Q; ++q) w[(int64_t)k * Q + q] = acc[i][q];
    }
}

// a thread per (signal, bin): the runs in ascending order, the mean over the signal's own segments, rounded once
template <class T, int CH>
__global__ __launch_bounds__(kSpectrumThreads) void cross_finish_kernel(const SpectrumArgs<T> a)
{
    constexpr int Q = CH == 2 ? 4 : 1;
    const int F = (1 << a.log_n) + 1;
    const int64_t i = (int64_t)blockIdx.x * kSpectrumThreads + threadIdx.x;
    if (i >= a.batch * F) return;
    const int64_t b = i / F, k = i - b * F;
    const int64_t segs = spectrum_segments(a, b);
    const int64_t runs = (segs + a.run - 1) / a.run;              // <= groups: segs <= segments
    double s[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) s[q] = 0.0;
    for (int64_t r = 0; r < runs; ++r) {
        const double *__restrict__ w = a.work + ((b * a.groups + r) * F + k) * Q;
#pragma unroll
        for (int q = 0; q < Q; ++q) s[q] += w[q];
    }
    const double d = segs > 0 ? (double)segs : 1.0;
    a.pxx[i] = (T)(s[0] / d);
    if (CH == 2) {
        a.pyy[i] = (T)(s[Q > 1 ? 1 : 0] / d);
        a.pxy[2 * i] = (T)(s[Q > 2 ? 2 : 0] / d);
        a.pxy[2 * i + 1] = (T)(s[Q > 3 ? 3 : 0] / d);
    }
}

// ---- the host side ---------------------------------------------------------------------------------------------------------
// The run length: the longest, up to VND_SPECTRUM_RUN, whose staged frames (and tile) fit the LDS budget beside the points;
// a whole number of passes when it is more than one.  (run = 1 fits for every supported shape.)
static int spectrum_run(int32_t nfft, int32_t nperseg, int32_t hop, int64_t sample_bytes, int32_t cross_channels)
{
    const int64_t budget = kSpectrumLdsBytes / sample_bytes;
    const int64_t bins = nfft / 2 + 1;
    const int G = kSpectrumCap / (nfft / 2);
    int run = 1;
    if (cross_channels) cross_channels = 2;                       // one run length for a pool and its mono views: the same sums
    for (int r = 2; r <= VND_SPECTRUM_RUN; ++r) {
        const int64_t room = (int64_t)(r - 1) * hop + nperseg;
        const int64_t need = cross_channels ? 2 * kSpectrumZ * (cross_channels == 2 ? 2 : 1) + cross_channels * room
                                            : 2 * kSpectrumZ + room + bins * (r | 1);
        if (need > budget) break;
        run = r;
    }
    if (run > G) run -= run % G;
    return run;
}

static size_t spectrum_lds_bytes(int32_t nfft, int32_t nperseg, int32_t hop, int run, int64_t sample_bytes, int32_t cross_channels)
{
    const int64_t room = (int64_t)(run - 1) * hop + nperseg;
    const int64_t bins = nfft / 2 + 1;
    const int64_t n = cross_channels ? 2 * kSpectrumZ * (cross_channels == 2 ? 2 : 1) + cross_channels * room
                                     : 2 * kSpectrumZ + room + bins * (run | 1);
    return (size_t)(n * sample_bytes);
}

static vnd_status spectrum_check_transform(int32_t nperseg, int32_t hop, int32_t nfft)
{
    if (nperseg < 2 || hop < 1) return fail(VND_ERR_INVALID, "nperseg - 1 and hop must be >= 1");
    if (nfft < VND_SPECTRUM_MIN_NFFT || nfft > VND_SPECTRUM_MAX_NFFT || (nfft & (nfft - 1)) != 0)
        return fail(VND_ERR_UNSUPPORTED, "nfft %d is not a power of two in [%d, %d]", nfft, VND_SPECTRUM_MIN_NFFT, VND_SPECTRUM_MAX_NFFT);
    if (nperseg > nfft) return fail(VND_ERR_UNSUPPORTED, "nperseg %d above nfft %d", nperseg, nfft);
    if (hop > nperseg) return fail(VND_ERR_UNSUPPORTED, "hop %d above nperseg %d: frames between segments", hop, nperseg);
    return VND_OK;
}

struct SpectrumShape {
    int64_t frame_bytes, segments, groups;
    int run, log_n;
};

// The checks the entries share, up to the shape: INVALID arguments, then UNSUPPORTED shapes.
template <class T>
static vnd_status spectrum_check(const T *x, int64_t batch, int64_t n_frames, int64_t stream_stride, int32_t frame_stride,
                             int32_t channels, const T *win, const T *tw, int32_t nperseg, int32_t hop, int32_t nfft, double scale,
                             int32_t cross, SpectrumShape *sh)
{
    if (!x || !win || !tw) return fail(VND_ERR_INVALID, "null frames, window or twiddles pointer");
    if (batch < 1 || n_frames < 1) return fail(VND_ERR_INVALID, "batch and n_frames must be >= 1");
    if (stream_stride < 1 || frame_stride < 1) return fail(VND_ERR_INVALID, "strides must be >= 1");
    if (channels != 1 && channels != 2) return fail(VND_ERR_INVALID, "channels must be 1 or 2, not %d", channels);
    if (channels > frame_stride) return fail(VND_ERR_INVALID, "%d channels in a frame stride of %d", channels, frame_stride);
    if (nperseg < 2 || hop < 1) return fail(VND_ERR_INVALID, "nperseg - 1 and hop must be >= 1");
    if (n_frames < nperseg) return fail(VND_ERR_INVALID, "n_frames %lld below nperseg %d: no whole segment", (long long)n_frames, nperseg);
    if (scale != scale) return fail(VND_ERR_INVALID, "scale is NaN");
    if (!(scale > 0.0 && scale <= (double)std::numeric_limits<T>::max() && (T)scale > (T)0))
        return fail(VND_ERR_INVALID, "scale %g is not positive and finite in the sample type", scale);
    vnd_status st = spectrum_check_transform(nperseg, hop, nfft);
    if (st != VND_OK) return st;
    if (batch > VND_MAX_STREAMS) return fail(VND_ERR_UNSUPPORTED, "batch %lld above %d: split the pool", (long long)batch, VND_MAX_STREAMS);
    if (n_frames > (int64_t)INT32_MAX) return fail(VND_ERR_UNSUPPORTED, "n_frames %lld above 2^31 - 1", (long long)n_frames);
    int64_t span, last;
    if (__builtin_mul_overflow(batch - 1, stream_stride, &span) ||
        __builtin_mul_overflow(n_frames - 1, (int64_t)frame_stride, &last) ||
        __builtin_add_overflow(span, last, &span) || span > ((int64_t)1 << 59))
        return fail(VND_ERR_UNSUPPORTED, "the pool's extents overflow");
    sh->frame_bytes = (span + channels) * (int64_t)sizeof(T);
    sh->segments = (n_frames - nperseg) / hop + 1;
    sh->run = spectrum_run(nfft, nperseg, hop, (int64_t)sizeof(T), cross ? channels : 0);
    sh->groups = (sh->segments + sh->run - 1) / sh->run;
    sh->log_n = 0;
    while ((2 << sh->log_n) < nfft) ++sh->log_n;
    if (sh->groups * batch * (cross ? 1 : channels) > kScopeMaxGroups)
        return fail(VND_ERR_UNSUPPORTED, "%lld workgroups in one launch, above 2^23: split the pool",
                    (long long)(sh->groups * batch * (cross ? 1 : channels)));
    return VND_OK;
}

template <class T>
static void spectrum_fill(SpectrumArgs<T> &a, const T *x, int64_t batch, int64_t n_frames, int64_t stream_stride, int32_t frame_stride,
                      int32_t channels, const T *win, const T *tw, int32_t nperseg, int32_t hop, int32_t nfft, int32_t detrend,
                      double scale, const int32_t *n_each, const SpectrumShape &sh)
{
    a.x = x; a.win = win; a.tw = tw; a.n_each = n_each;
    a.n_frames = n_frames; a.stream_stride = stream_stride; a.segments = sh.segments; a.groups = sh.groups;
    a.frame_stride = frame_stride; a.channels = channels; a.nperseg = nperseg; a.hop = hop; a.nfft = nfft; a.log_n = sh.log_n;
    a.detrend = detrend != 0; a.run = sh.run; a.scale = (T)scale; a.batch = batch;
}

template <class T>
static vnd_status spectrogram_dev(vnd_ctx *ctx, const T *x, int64_t batch, int64_t n_frames, int64_t stream_stride,
                                  int32_t frame_stride, int32_t channels, const T *win, const T *tw, int32_t nperseg, int32_t hop,
                                  int32_t nfft, int32_t detrend, double scale, const int32_t *n_each, T *sxx, void *stream_)
{
    if (!sxx) return fail(VND_ERR_INVALID, "null sxx pointer");
    SpectrumShape sh{};
    vnd_status st = spectrum_check(x, batch, n_frames, stream_stride, frame_stride, channels, win, tw, nperseg, hop, nfft, scale, 0, &sh);
    if (st != VND_OK) return st;
    const int64_t bins = nfft / 2 + 1;
    int64_t elems;
    if (__builtin_mul_overflow(batch * channels * bins, sh.segments, &elems) || elems > ((int64_t)1 << 59))
        return fail(VND_ERR_UNSUPPORTED, "the spectrogram's extents overflow");
    const int64_t out_bytes = elems * (int64_t)sizeof(T);
    const ScopeRegion ins[] = {{x, sh.frame_bytes}, {win, nperseg * (int64_t)sizeof(T)}, {tw, 2 * (int64_t)nfft * (int64_t)sizeof(T)},
                               {n_each, batch * 4}};
    for (const ScopeRegion &in : ins)
        if (scope_overlap(sxx, out_bytes, in.p, in.bytes))
            return fail(VND_ERR_INVALID, "sxx must not overlap the frames, the window, the twiddles or n_each");
    if (!ctx) return fail(VND_ERR_INVALID, "null context");
    DeviceScope on(ctx->device);
    if (!on.ok) return fail(VND_ERR_HIP, "cannot select device %d", ctx->device);
    hipStream_t stream = (hipStream_t)stream_;
    SpectrumArgs<T> a{};
    spectrum_fill(a, x, batch, n_frames, stream_stride, frame_stride, channels, win, tw, nperseg, hop, nfft, detrend, scale, n_each, sh);
    a.sxx = sxx;
    const size_t lds = spectrum_lds_bytes(nfft, nperseg, hop, sh.run, (int64_t)sizeof(T), 0);
    if ((st = allow_lds(ctx, (const void *)spectrogram_kernel<T>, lds)) != VND_OK) return st;
    hipLaunchKernelGGL(spectrogram_kernel<T>, dim3((unsigned)(batch * channels * sh.groups)), dim3(kSpectrumThreads), lds, stream, a);
    HIP_TRY(hipGetLastError());
    return VND_OK;
}

static int64_t spectrum_work_bytes(int64_t batch, int64_t groups, int32_t nfft, int32_t channels)
{
    return batch * groups * (nfft / 2 + 1) * (channels == 2 ? 4 : 1) * 8;      // < 2^16 * 2^31 * 2^12 * 2^5
}

template <class T>
static vnd_status cross_spectra_dev(vnd_ctx *ctx, const T *x, int64_t batch, int64_t n_frames, int64_t stream_stride,
                                    int32_t frame_stride, int32_t channels, const T *win, const T *tw, int32_t nperseg,
                                    int32_t hop, int32_t nfft, int32_t detrend, double scale, const int32_t *n_each, T *pxx, T *pyy,
                                    T *pxy, void *work, int64_t work_bytes, void *stream_)
{
    if (!pxx || (channels == 2 && (!pyy || !pxy))) return fail(VND_ERR_INVALID, "null pxx, pyy or pxy pointer");
    if (!work) return fail(VND_ERR_INVALID, "null work pointer: the runs' sums need vnd_cross_spectra_work_bytes of memory");
    if ((uintptr_t)work % 8 != 0) return fail(VND_ERR_INVALID, "the work memory is not 8-byte aligned");
    SpectrumShape sh{};
    vnd_status st = spectrum_check(x, batch, n_frames, stream_stride, frame_stride, channels, win, tw, nperseg, hop, nfft, scale, 1, &sh);
    if (st != VND_OK) return st;
    const int64_t need = spectrum_work_bytes(batch, sh.groups, nfft, channels);
    if (work_bytes < need)
        return fail(VND_ERR_INVALID, "work of %lld bytes, the call needs %lld", (long long)work_bytes, (long long)need);
    const int64_t bins = nfft / 2 + 1, row = batch * bins * (int64_t)sizeof(T);
    const ScopeRegion outs[] = {{pxx, row}, {channels == 2 ? pyy : nullptr, row}, {channels == 2 ? pxy : nullptr, 2 * row}, {work, need}};
    const ScopeRegion ins[] = {{x, sh.frame_bytes}, {win, nperseg * (int64_t)sizeof(T)}, {tw, 2 * (int64_t)nfft * (int64_t)sizeof(T)},
                               {n_each, batch * 4}};
    for (int i = 0; i < 4; ++i) {
        for (const ScopeRegion &in : ins)
            if (scope_overlap(outs[i].p, outs[i].bytes, in.p, in.bytes))
                return fail(VND_ERR_INVALID, "pxx, pyy, pxy and work must not overlap the frames, the window, the twiddles or n_each");
        for (int k = i + 1; k < 4; ++k)
            if (scope_overlap(outs[i].p, outs[i].bytes, outs[k].p, outs[k].bytes))
                return fail(VND_ERR_INVALID, "pxx, pyy, pxy and work must not overlap one another");
    }
    if (!ctx) return fail(VND_ERR_INVALID, "null context");
    DeviceScope on(ctx->device);
    if (!on.ok) return fail(VND_ERR_HIP, "cannot select device %d", ctx->device);
    hipStream_t stream = (hipStream_t)stream_;
    SpectrumArgs<T> a{};
    spectrum_fill(a, x, batch, n_frames, stream_stride, frame_stride, channels, win, tw, nperseg, hop, nfft, detrend, scale, n_each, sh);
    a.pxx = pxx; a.pyy = pyy; a.pxy = pxy; a.work = (double *)work;
    const size_t lds = spectrum_lds_bytes(nfft, nperseg, hop, sh.run, (int64_t)sizeof(T), channels);
    const dim3 grid((unsigned)(batch * sh.groups)), finish((unsigned)((batch * bins + kSpectrumThreads - 1) / kSpectrumThreads));
    if (channels == 2) {
        if ((st = allow_lds(ctx, (const void *)cross_spectra_kernel<T, 2>, lds)) != VND_OK) return st;
        hipLaunchKernelGGL((cross_spectra_kernel<T, 2>), grid, dim3(kSpectrumThreads), lds, stream, a);
        hipLaunchKernelGGL((cross_finish_kernel<T, 2>), finish, dim3(kSpectrumThreads), 0, stream, a);
    } else {
        if ((st = allow_lds(ctx, (const void *)cross_spectra_kernel<T, 1>, lds)) != VND_OK) return st;
        hipLaunchKernelGGL((cross_spectra_kernel<T, 1>), grid, dim3(kSpectrumThreads), lds, stream, a);
        hipLaunchKernelGGL((cross_finish_kernel<T, 1>), finish, dim3(kSpectrumThreads), 0, stream, a);
    }
    HIP_TRY(hipGetLastError());
    return VND_OK;
}

extern "C" {

vnd_status vnd_spectrum_run_length(int32_t nfft, int32_t nperseg, int32_t hop, int32_t is_float64, int32_t cross_channels,
                                   int32_t *run)
{
    if (!run) return fail(VND_ERR_INVALID, "null run");
    *run = 0;
    if (cross_channels < 0 || cross_channels > 2) return fail(VND_ERR_INVALID, "cross_channels must be 0, 1 or 2");
    const vnd_status st = spectrum_check_transform(nperseg, hop, nfft);
    if (st != VND_OK) return st;
    *run = spectrum_run(nfft, nperseg, hop, is_float64 ? 8 : 4, cross_channels);
    return VND_OK;
}

vnd_status vnd_cross_spectra_work_bytes(int64_t batch, int64_t n_frames, int32_t channels, int32_t nperseg, int32_t hop,
                                        int32_t nfft, int32_t is_float64, int64_t *bytes)
{
    if (!bytes) return fail(VND_ERR_INVALID, "null bytes");
    *bytes = 0;
    if (batch < 1 || n_frames < 1) return fail(VND_ERR_INVALID, "batch and n_frames must be >= 1");
    if (channels != 1 && channels != 2) return fail(VND_ERR_INVALID, "channels must be 1 or 2, not %d", channels);
    const vnd_status st = spectrum_check_transform(nperseg, hop, nfft);
    if (st != VND_OK) return st;
    if (n_frames < nperseg) return fail(VND_ERR_INVALID, "n_frames %lld below nperseg %d: no whole segment", (long long)n_frames, nperseg);
    if (batch > VND_MAX_STREAMS) return fail(VND_ERR_UNSUPPORTED, "batch %lld above %d: split the pool", (long long)batch, VND_MAX_STREAMS);
    if (n_frames > (int64_t)INT32_MAX) return fail(VND_ERR_UNSUPPORTED, "n_frames %lld above 2^31 - 1", (long long)n_frames);
    const int run = spectrum_run(nfft, nperseg, hop, is_float64 ? 8 : 4, channels);
    const int64_t segments = (n_frames - nperseg) / hop + 1;
    *bytes = spectrum_work_bytes(batch, (segments + run - 1) / run, nfft, channels);
    return VND_OK;
}

vnd_status vnd_spectrogram_f32_dev(vnd_ctx *ctx, const float *frames, int64_t batch, int64_t n_frames, int64_t stream_stride,
                                   int32_t frame_stride, int32_t channels, const float *window, const float *twiddles,
                                   int32_t nperseg, int32_t hop, int32_t nfft, int32_t detrend, double scale, const int32_t *n_each,
                                   float *sxx, void *stream)
{
    return spectrogram_dev<float>(ctx, frames, batch, n_frames, stream_stride, frame_stride, channels, window, twiddles, nperseg, hop,
                                  nfft, detrend, scale, n_each, sxx, stream);
}

vnd_status vnd_spectrogram_f64_dev(vnd_ctx *ctx, const double *frames, int64_t batch, int64_t n_frames, int64_t stream_stride,
                                   int32_t frame_stride, int32_t channels, const double *window, const double *twiddles,
                                   int32_t nperseg, int32_t hop, int32_t nfft, int32_t detrend, double scale, const int32_t *n_each,
                                   double *sxx, void *stream)
{
    return spectrogram_dev<double>(ctx, frames, batch, n_frames, stream_stride, frame_stride, channels, window, twiddles, nperseg, hop,
                                   nfft, detrend, scale, n_each, sxx, stream);
}

vnd_status vnd_cross_spectra_f32_dev(vnd_ctx *ctx, const float *frames, int64_t batch, int64_t n_frames, int64_t stream_stride,
                                     int32_t frame_stride, int32_t channels, const float *window, const float *twiddles,
                                     int32_t nperseg, int32_t hop, int32_t nfft, int32_t detrend, double scale,
                                     const int32_t *n_each, float *pxx, float *pyy, float *pxy, void *work, int64_t work_bytes,
                                     void *stream)
{
    return cross_spectra_dev<float>(ctx, frames, batch, n_frames, stream_stride, frame_stride, channels, window, twiddles, nperseg,
                                    hop, nfft, detrend, scale, n_each, pxx, pyy, pxy, work, work_bytes, stream);
}

vnd_status vnd_cross_spectra_f64_dev(vnd_ctx *ctx, const double *frames, int64_t batch, int64_t n_frames, int64_t stream_stride,
                                     int32_t frame_stride, int32_t channels, const double *window, const double *twiddles,
                                     int32_t nperseg, int32_t hop, int32_t nfft, int32_t detrend, double scale,
                                     const int32_t *n_each, double *pxx, double *pyy, double *pxy, void *work, int64_t work_bytes,
                                     void *stream)
{
    return cross_spectra_dev<double>(ctx, frames, batch, n_frames, stream_stride, frame_stride, channels, window, twiddles, nperseg,
                                     hop, nfft, detrend, scale, n_each, pxx, pyy, pxy, work, work_bytes, stream);
}

}  // extern "C"

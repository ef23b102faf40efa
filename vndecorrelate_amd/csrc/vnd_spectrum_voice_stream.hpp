// vnd_spectrum_voice_stream.hpp - the short-time spectra of a voice pool (include/vnd_spectrum_voice_stream.h): the columns of
// spectrogram_kernel and the Welch means of cross_spectra_kernel / cross_finish_kernel (vnd_spectrum.hpp) with the signal
// arriving block by block, the position per slot in the device state and a count and start / end flags per slot and call -
// what vnd_correlogram_voice_stream.hpp is to the correlogram.
// (one translation unit: included by vnd_amd.hip after vnd_spectrum.hpp and vnd_voice_stream.hpp)
//
// The compute is the one-shot call's: spectrum_transform, spectrum_bin and spectrum_scaled unchanged, on the LDS plan of
// cross_spectra_kernel - the points, (stereo) the left spectra of a pass, (R - 1) hop + nperseg staged frames a channel - so
// it fits wherever the one-shot call does.  Two things are new: where a staged frame comes from, and where a run's sum
// starts.
//
// spectrum_voice_kernel, grid (slots, G), G = ceil(RC / R) + 1, 256 threads.  The SLOT is the fast dimension (DESIGN.md
// 3.16): workgroups are dealt round-robin over the XCDs by their linear index, and in steady state only the first groups of a
// slot have segments.  Every workgroup reads pos[b], counts[b] and flags[b] once, workgroup-uniform, and forms the slot's
// span with sv_span - the host's own function.  Workgroup j owns the ABSOLUTE run r = w0 / R + j, the segments
// [max(w0, r R), min(w1, (r + 1) R)): at most RC new segments touch at most G runs.  It first does its share of the ring copy
// (grid-stride over the slot's workgroups, as CgVoice), then leaves, before any barrier, when its range is empty.  Frame f of
// the range comes from the chunk when f >= p and from the ring otherwise.  The run is transformed in passes of 2048 / (nfft /
// 2) segments; thread k adds bin k's values to float64 registers in ascending t - starting from the stored `partial` when the
// run was begun by an earlier call (j = 0 and w0 % R != 0), from +0.0 otherwise - writes the columns straight to cols (the
// bin on the lane: a wave stores consecutive k of a row) and stores the run's sums to work[b][j].  A segment's arithmetic
// does not depend on its pass, its run or its call: every column is the one-segment call's, bit for bit.
//
// spectrum_voice_finish_kernel, grid (slots), follows on the same stream; the kernel boundary is the ordering between every
// workgroup's read of pos[b] and its update, and between the writes of work and their reads (vnd_voice_core.hpp).  A thread
// per bin (a stride of 256 over F): total = the stored one if w0 >= R else +0.0; the runs this call completed are added to
// it in ascending order; the incomplete one becomes `partial`; the means are (total [+ partial]) / w1, rounded once - the
// operation sequence of cross_finish_kernel.  It is one workgroup a slot, and not voice_advance_kernel's lane a slot,
// because the bins of a slot read pos[b] and one of them writes it: a barrier orders that inside a workgroup.
//
// Ring (vnd_correlogram_voice_stream.hpp's argument, per slot with the slot's own p and n).  cap = W - 1 + M.  Frames read
// from the ring lie in [p - W + 1, p): segment sc(p) was not complete at p.  Frames written lie in [p + n - min(n, W - 1),
// p + n).  A written frame g and a read frame f satisfy 0 < g - f <= W - 2 + n < cap: different ring slots, so no ring slot
// is both read and written in one call although the slot's workgroups are not ordered.  A call with END writes nothing.
//
// Every index that is built from device data:
//   - counts[b] outside [0, M], or pos[b] outside [0, 2^60] without START: the span is not ok and both kernels leave before
//     anything is addressed with it (the finish kernel writes out_counts[b] = -1 only) - so 0 <= p <= 2^60, 0 <= n <= M;
//   - chunk frames: a segment of this call ends at or below p + n, so the chunk is read at [0, n) only; the ring copy reads
//     [n - min(n, W - 1), n);
//   - ring slots: a first slot in [0, cap) walked forward by less than cap with one wrap;
//   - rows: t - w0 < w1 - w0 <= RC; work: j < G by the grid, and in the finish kernel the runs touched are <= G.
#pragma once
#include "../../include/vnd_spectrum_voice_stream.h"

// One slot's side of a call, from the stored position, counts[b] and flags[b] alone.
struct SvSpan : vnd::VoiceHead {
    int64_t w0, w1;                // segments complete before and after the call; !ok: both 0, the slot is left alone
    bool idle;                     // ok, no frame and no flag: only out_counts[b] = 0 is written
};

__host__ __device__ inline int64_t sv_complete(int64_t q, int64_t W, int64_t H) { return q >= W ? (q - W) / H + 1 : 0; }

__host__ __device__ inline SvSpan sv_span(int64_t stored, int32_t count, int32_t flags, int64_t M, int64_t W, int64_t H)
{
    SvSpan v{vnd::voice_head(stored, count, flags, M)};
    if (!v.ok) return v;
    v.idle = count == 0 && !v.start && !v.end;
    v.w0 = sv_complete(v.p, W, H);
    v.w1 = sv_complete(v.p + v.n, W, H);
    return v;
}

template <class T>
struct SvArgs {
    SpectrumArgs<T> sp;               // x, stream_stride, frame_stride: the chunk; win, tw, nperseg, hop, nfft, log_n, detrend,
                                      // run, scale; pxx, pyy, pxy: the pool's means (null: none); the rest is not read
    int64_t *__restrict__ pos;        // [slots]
    const int32_t *__restrict__ counts;
    const int32_t *__restrict__ flags;
    int32_t *__restrict__ out_counts;
    int64_t *__restrict__ segments;   // [slots], null with pxx
    double *__restrict__ sums;        // [slots][F][Q][2] (total, partial)
    double *__restrict__ work;        // [slots][G][F][Q]
    T *__restrict__ ring;             // [slots][cap][channels]
    T *__restrict__ cols;             // [slots][rc][channels][F], or null
    int64_t M, cap, rc;               // max_frames_per_call, W - 1 + M, ceil(M / H)
    int32_t groups;                   // G
};

template <class T>
__device__ __forceinline__ SvSpan sv_view(const SvArgs<T> &a, int64_t b)
{
    return sv_span(vnd::uniform_i64(a.pos[b]), __builtin_amdgcn_readfirstlane(a.counts[b]),
                   __builtin_amdgcn_readfirstlane(a.flags[b]), a.M, a.sp.nperseg, a.sp.hop);
}

// grid = (slots, G); dynamic LDS: the points, (stereo) the left spectra of a pass, the staged frames
template <class T, int CH>
__global__ __launch_bounds__(kSpectrumThreads) void spectrum_voice_kernel(const SvArgs<T> a)
{
    constexpr int Q = CH == 2 ? 4 : 1;
    extern __shared__ __attribute__((aligned(16))) double spectrum_lds[];
    __shared__ double red[kSpectrumThreads];
    const SpectrumArgs<T> &sp = a.sp;
    const int tid = threadIdx.x;
    const int N = 1 << sp.log_n, F = N + 1, G = kSpectrumCap >> sp.log_n;
    const int W = sp.nperseg, H = sp.hop, R = sp.run;
    const int64_t b = blockIdx.x;
    const int j = (int)blockIdx.y;
    const SvSpan s = sv_view(a, b);
    if (!s.ok) return;                                            // (workgroup-uniform, before any barrier)
    const T *__restrict__ chunk = sp.x + b * sp.stream_stride;
    T *__restrict__ ring = a.ring + b * a.cap * CH;
    // the chunk frames later calls read, into the ring: the slot's workgroups share them in grid-stride order
    const int64_t keep = s.end ? 0 : (s.n < W - 1 ? s.n : W - 1);
    if (keep > 0) {
        const int64_t slot0 = (s.p + s.n - keep) % a.cap, rel0 = s.n - keep;
        for (int64_t e = (int64_t)j * kSpectrumThreads + tid; e < keep * CH; e += (int64_t)gridDim.y * kSpectrumThreads) {
            const int64_t i = e / CH;
            const int c = (int)(e - i * CH);
            int64_t slot = slot0 + i;
            if (slot >= a.cap) slot -= a.cap;
            ring[slot * CH + c] = chunk[(rel0 + i) * sp.frame_stride + c];
        }
    }
    const int64_t run = s.w0 / R + j;
    const int64_t lo = s.w0 > run * R ? s.w0 : run * R, hi = s.w1 < (run + 1) * R ? s.w1 : (run + 1) * R;
    if (lo >= hi) return;                                         // (workgroup-uniform, before any barrier)
    const int nseg = (int)(hi - lo);                              // 1 .. R
    T *zre = (T *)spectrum_lds, *zim = zre + kSpectrumZ;
    T *xlr = zim + kSpectrumZ, *xli = xlr + (CH == 2 ? kSpectrumZ : 0);
    T *stage = xli + (CH == 2 ? kSpectrumZ : 0);
    const int room = (R - 1) * H + W;                             // a channel's staged frames
    const int span = (nseg - 1) * H + W;
    const int64_t rel0 = lo * H - s.p;                            // in (-W, n): segment lo was not complete at p
    const int64_t slot0 = rel0 < 0 ? (lo * H) % a.cap : 0;
    for (int e = tid; e < span * CH; e += kSpectrumThreads) {
        const int i = e / CH, c = e - i * CH;
        const int64_t rel = rel0 + i;
        T v;
        if (rel >= 0) {
            v = chunk[rel * sp.frame_stride + c];
        } else {
            int64_t slot = slot0 + i;
            if (slot >= a.cap) slot -= a.cap;
            v = ring[slot * CH + c];
        }
        stage[c * room + i] = v;
    }
    __syncthreads();
    const bool resume = j == 0 && s.w0 % R != 0;                  // the run was begun by an earlier call of this voice
    const double *__restrict__ held = a.sums + b * F * Q * 2;
    double acc[kSpectrumBinsPerThread][Q];
#pragma unroll
    for (int i = 0; i < kSpectrumBinsPerThread; ++i)
#pragma unroll
        for (int q = 0; q < Q; ++q) acc[i][q] = 0.0;
    if (resume) {                                                 // (workgroup-uniform)
#pragma unroll
        for (int i = 0; i < kSpectrumBinsPerThread; ++i) {
            // a lane past the last bin reads the last bin's, and never stores it: no lane mask to keep for the loop below
            const int k = tid + i * kSpectrumThreads < F ? tid + i * kSpectrumThreads : F - 1;
#pragma unroll
            for (int q = 0; q < Q; ++q) acc[i][q] = held[(k * Q + q) * 2 + 1];
        }
    }
    // (the lane's own pointer - bin tid of the call's first row here, of work[b][j] below - is a vector register: the loop
    // is short of scalar ones)
    T *__restrict__ rows = a.cols ? a.cols + ((b * a.rc + (lo - s.w0)) * CH * F + tid) : nullptr;
    for (int gb = 0; gb < nseg; gb += G) {
        const int cnt = nseg - gb < G ? nseg - gb : G;
        spectrum_transform(sp, zre, zim, stage, gb, nseg, red);
        if (CH == 2) {
            for (int e = tid; e < cnt * F; e += kSpectrumThreads) {
                const int g = e / F, k = e - g * F;
                T xr, xi;
                spectrum_bin(sp, zre, zim, g << sp.log_n, k, xr, xi);
                xlr[e] = xr;
                xli[e] = xi;
            }
            __syncthreads();
            spectrum_transform(sp, zre, zim, stage + room, gb, nseg, red);
        }
#pragma unroll
        for (int i = 0; i < kSpectrumBinsPerThread; ++i) {
            const int k = tid + i * kSpectrumThreads;
            if (k >= F) continue;
            for (int g = 0; g < cnt; ++g) {                       // ascending t
                T xr, xi;
                spectrum_bin(sp, zre, zim, g << sp.log_n, k, xr, xi);
                const T m0 = xr * xr, m1 = xi * xi;
                T *__restrict__ row = rows ? rows + (int64_t)(gb + g) * CH * F : nullptr;
                if (CH == 1) {
                    const T pw = spectrum_scaled(sp, m0 + m1, k);
                    acc[i][0] += (double)pw;
                    if (row) row[i * kSpectrumThreads] = pw;
                } else {
                    const T lr = xlr[g * F + k], li = xli[g * F + k];
                    const T l0 = lr * lr, l1 = li * li;
                    const T c0 = lr * xr, c1 = li * xi, c2 = lr * xi, c3 = li * xr;
                    const T pl = spectrum_scaled(sp, l0 + l1, k), pr = spectrum_scaled(sp, m0 + m1, k);
                    acc[i][0] += (double)pl;
                    acc[i][Q > 1 ? 1 : 0] += (double)pr;
                    acc[i][Q > 2 ? 2 : 0] += (double)spectrum_scaled(sp, c0 + c1, k);        // conj(X_L) * X_R
                    acc[i][Q > 3 ? 3 : 0] += (double)spectrum_scaled(sp, c2 - c3, k);
                    if (row) {
                        row[i * kSpectrumThreads] = pl;
                        row[F + i * kSpectrumThreads] = pr;
                    }
                }
            }
        }
        __syncthreads();
    }
    double *__restrict__ w = a.work + ((b * a.groups + j) * F + tid) * Q;
#pragma unroll
    for (int i = 0; i < kSpectrumBinsPerThread; ++i) {
        if (tid + i * kSpectrumThreads >= F) continue;
#pragma unroll
        for (int q = 0; q < Q; ++q) w[i * kSpectrumThreads * Q + q] = acc[i][q];
    }
}

// grid = (slots): the runs this call completed into `total`, the one in progress as `partial`, the means, pos and out_counts
template <class T, int CH>
__global__ __launch_bounds__(kSpectrumThreads) void spectrum_voice_finish_kernel(const SvArgs<T> a)
{
    constexpr int Q = CH == 2 ? 4 : 1;
    const SpectrumArgs<T> &sp = a.sp;
    const int tid = threadIdx.x;
    const int F = (1 << sp.log_n) + 1, R = sp.run;
    const int64_t b = blockIdx.x;
    const SvSpan s = sv_view(a, b);
    if (!s.ok || s.idle) {                                        // (workgroup-uniform, before any barrier)
        if (tid == 0) a.out_counts[b] = s.ok ? 0 : -1;
        return;
    }
    const int64_t r0 = s.w0 / R;
    const int touched = s.w1 > s.w0 ? (int)((s.w1 - 1) / R - r0) + 1 : 0;       // runs with a segment of this call: <= G
    const bool open = s.w1 % R != 0;                                             // the last run is in progress
    const double d = s.w1 > 0 ? (double)s.w1 : 1.0;
    for (int k = tid; k < F; k += kSpectrumThreads) {
        double *__restrict__ sum = a.sums + (b * F + k) * Q * 2;
        const double *__restrict__ w = a.work + (b * a.groups * F + k) * Q;
        double mean[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            double total = s.w0 >= R ? sum[2 * q] : 0.0;
            double partial = 0.0;
            if (touched == 0) {
                if (open) partial = sum[2 * q + 1];
            } else {
                for (int jj = 0; jj < touched; ++jj) {            // ascending runs
                    const double v = w[(int64_t)jj * F * Q + q];
                    if ((r0 + jj + 1) * R <= s.w1) total += v;
                    else partial = v;
                }
                if (!s.end) {
                    sum[2 * q] = total;
                    if (open) sum[2 * q + 1] = partial;
                }
            }
            mean[q] = (open ? total + partial : total) / d;
        }
        if (sp.pxx) {
            const int64_t i = b * F + k;
            sp.pxx[i] = (T)mean[0];
            if (CH == 2) {
                sp.pyy[i] = (T)mean[Q > 1 ? 1 : 0];
                sp.pxy[2 * i] = (T)mean[Q > 2 ? 2 : 0];
                sp.pxy[2 * i + 1] = (T)mean[Q > 3 ? 3 : 0];
            }
        }
    }
    __syncthreads();                                              // every wave has read pos[b]
    if (tid == 0) {
        a.out_counts[b] = (int32_t)(s.w1 - s.w0);
        if (a.segments) a.segments[b] = s.w1;
        a.pos[b] = s.next;
    }
}

// ---- the host side ---------------------------------------------------------------------------------------------------------
// The fixed launch of a pool, and where the parts of its state begin.
struct SvPlan {
    int64_t rc, groups, workgroups, finish_groups, cap, need;
    int64_t sums_at, work_at, ring_at;
    int run, log_n;
};

static int64_t sv_pad16(int64_t bytes) { return (bytes + 15) & ~(int64_t)15; }

// The VND_ERR_INVALID half of the pool's scalar checks.
static vnd_status sv_scalars(int64_t slots, int32_t channels, int32_t nperseg, int32_t hop, int64_t max_frames_per_call)
{
    if (slots < 1 || max_frames_per_call < 1) return fail(VND_ERR_INVALID, "slots and max_frames_per_call must be >= 1");
    if (max_frames_per_call > INT32_MAX)
        return fail(VND_ERR_INVALID, "max_frames_per_call %lld above INT32_MAX: counts are int32", (long long)max_frames_per_call);
    if (channels != 1 && channels != 2) return fail(VND_ERR_INVALID, "channels must be 1 or 2, not %d", channels);
    if (nperseg < 2 || hop < 1) return fail(VND_ERR_INVALID, "nperseg - 1 and hop must be >= 1");
    return VND_OK;
}

// The scalar side of the pool's checks, in the order the entries report them.
static vnd_status sv_plan(int64_t slots, int32_t channels, int32_t nperseg, int32_t hop, int32_t nfft, int64_t max_frames_per_call,
                          int64_t sample_bytes, SvPlan *plan)
{
    vnd_status st = sv_scalars(slots, channels, nperseg, hop, max_frames_per_call);
    if (st != VND_OK) return st;
    if ((st = spectrum_check_transform(nperseg, hop, nfft)) != VND_OK) return st;
    if (slots > VND_MAX_STREAMS) return fail(VND_ERR_UNSUPPORTED, "slots %lld above %d: split the pool", (long long)slots, VND_MAX_STREAMS);
    SvPlan p{};
    const int64_t bins = nfft / 2 + 1, q = channels == 2 ? 4 : 1;
    p.run = spectrum_run(nfft, nperseg, hop, sample_bytes, channels);
    while ((2 << p.log_n) < nfft) ++p.log_n;
    p.rc = (max_frames_per_call + hop - 1) / hop;
    p.groups = (p.rc + p.run - 1) / p.run + 1;
    p.workgroups = slots * p.groups;
    p.finish_groups = slots;
    p.cap = max_frames_per_call + nperseg - 1;
    if (p.groups > 65535)
        return fail(VND_ERR_UNSUPPORTED, "%lld runs per slot and call, above the 65535 of a grid dimension", (long long)p.groups);
    if (p.workgroups > kScopeMaxGroups) return fail(VND_ERR_UNSUPPORTED, "%lld workgroups in one launch, above 2^23", (long long)p.workgroups);
    if (slots * p.rc * channels * bins > ((int64_t)1 << 40))      // < 2^16 * 2^31 * 2 * 2^12
        return fail(VND_ERR_UNSUPPORTED, "cols of %lld x %lld x %d x %lld values, above 2^40", (long long)slots, (long long)p.rc, channels,
                    (long long)bins);
    p.sums_at = voice_position_bytes(slots);
    p.work_at = p.sums_at + slots * bins * q * 16;
    p.ring_at = p.work_at + sv_pad16(p.workgroups * bins * q * 8);                  // < 2^23 * 2^12 * 2^5
    p.need = p.ring_at + sv_pad16(slots * p.cap * channels * sample_bytes);         // < 2^16 * 2^32 * 2^4
    *plan = p;
    return VND_OK;
}

template <class T>
static vnd_status spectrum_voice_stream_dev(vnd_ctx *ctx, void *state, int64_t state_bytes, int64_t max_frames_per_call, const T *x,
                                            int64_t stream_stride, int32_t frame_stride, int32_t channels, const int32_t *counts,
                                            const int32_t *flags, const T *win, const T *tw, int32_t nperseg, int32_t hop,
                                            int32_t nfft, int32_t detrend, double scale, T *cols, int32_t *out_counts, T *pxx,
                                            T *pyy, T *pxy, int64_t *segments, int64_t slots, void *stream_)
{
    if (!state || !x || !counts || !flags || !win || !tw || !out_counts)
        return fail(VND_ERR_INVALID, "null state, frames, counts, flags, window, twiddles or out_counts pointer");
    vnd_status st = sv_scalars(slots, channels, nperseg, hop, max_frames_per_call);
    if (st != VND_OK) return st;
    const bool means = pxx || pyy || pxy || segments;
    if (means && (!pxx || !segments || (channels == 2 && (!pyy || !pxy))))
        return fail(VND_ERR_INVALID, "pxx, pyy, pxy and segments are null as a group, or all given (pyy and pxy may be null with one channel)");
    if (stream_stride < 1 || frame_stride < 1) return fail(VND_ERR_INVALID, "strides must be >= 1");
    if (channels > frame_stride) return fail(VND_ERR_INVALID, "%d channels in a frame stride of %d", channels, frame_stride);
    if (scale != scale) return fail(VND_ERR_INVALID, "scale is NaN");
    if (!(scale > 0.0 && scale <= (double)std::numeric_limits<T>::max() && (T)scale > (T)0))
        return fail(VND_ERR_INVALID, "scale %g is not positive and finite in the sample type", scale);
    SvPlan p{};
    if ((st = sv_plan(slots, channels, nperseg, hop, nfft, max_frames_per_call, (int64_t)sizeof(T), &p)) != VND_OK) return st;
    if ((st = voice_state_check("spectrum voice pool", state, state_bytes, p.need, slots)) != VND_OK) return st;
    int64_t xb = 0;
    if ((st = voice_chunk_bytes(slots, stream_stride, max_frames_per_call, frame_stride, sizeof(T), &xb)) != VND_OK) return st;
    xb += (channels - 1) * (int64_t)sizeof(T);
    const int64_t bins = nfft / 2 + 1, row = slots * bins * (int64_t)sizeof(T);
    const bool stereo = channels == 2;
    const ScopeRegion outs[] = {{state, p.need}, {cols, slots * p.rc * channels * bins * (int64_t)sizeof(T)}, {out_counts, slots * 4},
                                {pxx, row}, {stereo ? pyy : nullptr, row}, {stereo ? pxy : nullptr, 2 * row}, {segments, slots * 8}};
    const ScopeRegion ins[] = {{x, xb}, {win, nperseg * (int64_t)sizeof(T)}, {tw, 2 * (int64_t)nfft * (int64_t)sizeof(T)},
                               {counts, slots * 4}, {flags, slots * 4}};
    constexpr int n_outs = (int)(sizeof(outs) / sizeof(outs[0]));
    for (int i = 0; i < n_outs; ++i) {
        for (const ScopeRegion &in : ins)
            if (scope_overlap(outs[i].p, outs[i].bytes, in.p, in.bytes))
                return fail(VND_ERR_INVALID, "the state and the outputs must not overlap the frames, the window, the twiddles, counts or flags");
        for (int k = i + 1; k < n_outs; ++k)
            if (scope_overlap(outs[i].p, outs[i].bytes, outs[k].p, outs[k].bytes))
                return fail(VND_ERR_INVALID, "the state, cols, out_counts, pxx, pyy, pxy and segments must not overlap one another");
    }
    if (!ctx) return fail(VND_ERR_INVALID, "null context");
    DeviceScope on(ctx->device);
    if (!on.ok) return fail(VND_ERR_HIP, "cannot select device %d", ctx->device);
    hipStream_t stream = (hipStream_t)stream_;

    SvArgs<T> a{};
    a.sp.x = x; a.sp.win = win; a.sp.tw = tw;
    a.sp.stream_stride = stream_stride; a.sp.frame_stride = frame_stride; a.sp.channels = channels;
    a.sp.nperseg = nperseg; a.sp.hop = hop; a.sp.nfft = nfft; a.sp.log_n = p.log_n; a.sp.detrend = detrend != 0; a.sp.run = p.run;
    a.sp.scale = (T)scale; a.sp.batch = slots;
    a.sp.pxx = pxx; a.sp.pyy = pyy; a.sp.pxy = pxy;
    a.pos = (int64_t *)state; a.counts = counts; a.flags = flags; a.out_counts = out_counts; a.segments = segments;
    a.sums = (double *)((char *)state + p.sums_at);
    a.work = (double *)((char *)state + p.work_at);
    a.ring = (T *)((char *)state + p.ring_at);
    a.cols = cols;
    a.M = max_frames_per_call; a.cap = p.cap; a.rc = p.rc; a.groups = (int32_t)p.groups;
    const size_t lds = spectrum_lds_bytes(nfft, nperseg, hop, p.run, (int64_t)sizeof(T), channels);
    const dim3 grid((unsigned)slots, (unsigned)p.groups), finish((unsigned)p.finish_groups);
    if (stereo) {
        if ((st = allow_lds(ctx, (const void *)spectrum_voice_kernel<T, 2>, lds)) != VND_OK) return st;
        hipLaunchKernelGGL((spectrum_voice_kernel<T, 2>), grid, dim3(kSpectrumThreads), lds, stream, a);
        hipLaunchKernelGGL((spectrum_voice_finish_kernel<T, 2>), finish, dim3(kSpectrumThreads), 0, stream, a);
    } else {
        if ((st = allow_lds(ctx, (const void *)spectrum_voice_kernel<T, 1>, lds)) != VND_OK) return st;
        hipLaunchKernelGGL((spectrum_voice_kernel<T, 1>), grid, dim3(kSpectrumThreads), lds, stream, a);
        hipLaunchKernelGGL((spectrum_voice_finish_kernel<T, 1>), finish, dim3(kSpectrumThreads), 0, stream, a);
    }
    HIP_TRY(hipGetLastError());
    return VND_OK;
}

extern "C" {

vnd_status vnd_spectrum_voice_stream_state_bytes(int64_t slots, int32_t channels, int32_t nperseg, int32_t hop, int32_t nfft,
                                                 int64_t max_frames_per_call, int32_t is_float64, int64_t *bytes)
{
    if (!bytes) return fail(VND_ERR_INVALID, "null bytes");
    *bytes = 0;
    SvPlan p{};
    const vnd_status st = sv_plan(slots, channels, nperseg, hop, nfft, max_frames_per_call, is_float64 ? 8 : 4, &p);
    if (st != VND_OK) return st;
    *bytes = p.need;
    return VND_OK;
}

vnd_status vnd_spectrum_voice_stream_reset_dev(vnd_ctx *ctx, void *state, int64_t state_bytes, int64_t slots, int32_t channels,
                                               int32_t nperseg, int32_t hop, int32_t nfft, int64_t max_frames_per_call,
                                               int32_t is_float64, void *stream_)
{
    SvPlan p{};
    vnd_status st = sv_plan(slots, channels, nperseg, hop, nfft, max_frames_per_call, is_float64 ? 8 : 4, &p);
    if (st != VND_OK) return st;
    if ((st = voice_state_check("spectrum voice pool", state, state_bytes, p.need, slots)) != VND_OK) return st;
    if (!ctx) return fail(VND_ERR_INVALID, "null context");
    {   // host side only, nothing enqueued: the compute kernel's LDS limit is raised here, before a first call is captured
        DeviceScope on(ctx->device);
        if (!on.ok) return fail(VND_ERR_HIP, "cannot select device %d", ctx->device);
        const size_t lds = spectrum_lds_bytes(nfft, nperseg, hop, p.run, is_float64 ? 8 : 4, channels);
        const void *kernel = is_float64 ? (channels == 2 ? (const void *)spectrum_voice_kernel<double, 2> : (const void *)spectrum_voice_kernel<double, 1>)
                                        : (channels == 2 ? (const void *)spectrum_voice_kernel<float, 2> : (const void *)spectrum_voice_kernel<float, 1>);
        if ((st = allow_lds(ctx, kernel, lds)) != VND_OK) return st;
    }
    return voice_reset_positions(ctx, state, slots, stream_);
}

vnd_status vnd_spectrum_voice_stream_f32_dev(vnd_ctx *ctx, void *state, int64_t state_bytes, int64_t max_frames_per_call,
                                             const float *frames, int64_t stream_stride, int32_t frame_stride, int32_t channels,
                                             const int32_t *counts, const int32_t *flags, const float *window,
                                             const float *twiddles, int32_t nperseg, int32_t hop, int32_t nfft, int32_t detrend,
                                             double scale, float *cols, int32_t *out_counts, float *pxx, float *pyy, float *pxy,
                                             int64_t *segments, int64_t slots, void *stream)
{
    return spectrum_voice_stream_dev<float>(ctx, state, state_bytes, max_frames_per_call, frames, stream_stride, frame_stride,
                                            channels, counts, flags, window, twiddles, nperseg, hop, nfft, detrend, scale, cols,
                                            out_counts, pxx, pyy, pxy, segments, slots, stream);
}

vnd_status vnd_spectrum_voice_stream_f64_dev(vnd_ctx *ctx, void *state, int64_t state_bytes, int64_t max_frames_per_call,
                                             const double *frames, int64_t stream_stride, int32_t frame_stride, int32_t channels,
                                             const int32_t *counts, const int32_t *flags, const double *window,
                                             const double *twiddles, int32_t nperseg, int32_t hop, int32_t nfft, int32_t detrend,
                                             double scale, double *cols, int32_t *out_counts, double *pxx, double *pyy,
                                             double *pxy, int64_t *segments, int64_t slots, void *stream)
{
    return spectrum_voice_stream_dev<double>(ctx, state, state_bytes, max_frames_per_call, frames, stream_stride, frame_stride,
                                             channels, counts, flags, window, twiddles, nperseg, hop, nfft, detrend, scale, cols,
                                             out_counts, pxx, pyy, pxy, segments, slots, stream);
}

}  // extern "C"

// vnd_level.hpp - the polar level envelope (include/vnd_level.h): np.percentile of the radii of every angular slice of every
// signal of a pool, by an exact radix select on the device.
// (one translation unit: included by vnd_amd.hip after vnd_scope.hpp, whose sample, radius, bin and maximum it reuses)
//
// A cell is one (signal, bin, percentile); its key is the bit pattern of a radius (non-negative: unsigned order is value
// order).  The kernels of one call, all on the caller's stream:
//   scope_max_kernel      (radius_scale <= 0 only) the per-signal maximum, vnd_scope.hpp's first pass
//   level_stage_kernel    grid (ceil(n / span), batch): the sample of every used frame ONCE - its key and its bin (uint16, 0xFFFF:
//                         no bin) into work memory, the frames per bin counted in LDS and added to bin_counts
//   level_init_kernel     a thread per cell: the percentile rule on the bin's count - prev, want-next, gamma; prefix 0, rank prev
//   level_select_kernel   per pass, grid as stage: a workgroup counts, in LDS, the current digit of every key of its span for
//                         every percentile of the key's bin whose prefix the key matches, and adds its non-zero counters to the
//                         global digit histogram
//   level_advance_kernel  per pass, a thread per cell: walks the digit counts to the one that holds the remaining rank, extends
//                         the prefix, reduces the rank, clears the counters.  After the last pass the prefix is sorted[prev] and
//                         the digit's count says how many keys equal it: rank + 1 < count means sorted[next] == sorted[prev];
//                         otherwise the cell asks for ...
//   level_min_kernel      grid as stage: the smallest key above the prefix of every asking cell - atomicMin on the bit
//                         patterns, in LDS, then in global memory
//   level_finish_kernel   a thread per output: NumPy's lerp on the two order statistics
// Everything from level_init_kernel on is "the select over staged keys", level_run_select: the voice pool of
// vnd_level_voice_stream.hpp runs it over its rings, which hold what level_stage_kernel stages (level_frame).
// Digits are d bits, the widest for which a signal's counters and prefixes fit VND_SCOPE_LDS_BYTES (360 bins x 2
// percentiles: d = 5, 7 passes over float32 keys, 13 over float64) - narrower for short signals, level_digit_bits below.
//
// Every index that is built from device data:
//   - n_each[b]: scope_span, as in vnd_scope.hpp;
//   - a bin comes from scope_bin (-1, or in [0, bins - 1]); the staged uint16 is compared with the bin count again where it is
//     read, so a select pass indexes inside its counters whatever the work memory holds;
//   - a digit is masked to its width; the advance walk stays below 2^width and falls back to the last digit.
#pragma once
#include "../../include/vnd_level.h"

constexpr int kLevelThreads = 1024, kLevelCellThreads = 256;
constexpr int kLevelMaxDigitBits = 8;
constexpr unsigned int kLevelNonEmpty = 1u, kLevelWantNext = 2u, kLevelNeedMin = 4u;
constexpr unsigned short kLevelNoBin = 0xFFFFu;

template <class T>
struct LevelArgs {
    using Bits = typename ScopeKind<T>::Bits;
    ScopeArgs<T> s;                         // the pool, n_each, the angle edges (e0, bins0), the maximum (work), scale, span
    Bits *__restrict__ keys;                // [batch][n_frames]
    unsigned short *__restrict__ bins;      // [batch][n_frames]
    unsigned int *__restrict__ bin_counts;  // [batch][num_bins]
    Bits *__restrict__ prefix;              // [batch][num_bins][num_p] from here on: a cell
    Bits *__restrict__ next;
    T *__restrict__ gamma;
    unsigned int *__restrict__ rank;
    unsigned int *__restrict__ flags;
    unsigned int *__restrict__ hist;        // [cell][1 << digit_bits]
    T *__restrict__ levels;                 // [batch][num_p][num_bins]
    T q[VND_LEVEL_MAX_PERCENTILES];         // T(p) / T(100)
    int32_t num_p, digit_bits, shift, width, last;
    int64_t cells_all;                      // batch * num_bins * num_p
};

__device__ __forceinline__ float level_floor(float v) { return floorf(v); }
__device__ __forceinline__ double level_floor(double v) { return floor(v); }

// One count at cnt[idx] (idx < 0: none).  A wave whose active lanes all ask for one counter - a mono signal, equal frames,
// the top digits of a quiet one - adds their number once instead of serialising on the address.
__device__ __forceinline__ void level_count(unsigned int *cnt, int idx)
{
    const unsigned long long act = __ballot(1);
    const int first = __builtin_amdgcn_readfirstlane(idx);
    if (__ballot(idx == first) == act) {
        if (first >= 0 && (int)__lane_id() == __ffsll((unsigned long long)act) - 1) atomicAdd(cnt + first, (unsigned int)__popcll(act));
    } else if (idx >= 0) {
        atomicAdd(cnt + idx, 1u);
    }
}

// What is staged for one frame: its slice on the edges e (staged in LDS; inv = bins / (e[bins] - e[0])), -1 for none, and
// its key, the bit pattern of radius / den.  level_stage_kernel and the voice pool's push (vnd_level_voice_stream.hpp) both
// stage through this function, so a ring entry of the pool is what the one-shot entry writes for the frame.
template <class T>
__device__ __forceinline__ int level_frame(T l, T r, bool ms, bool fold, T den, const double *e, int bins, double inv,
                                           typename ScopeKind<T>::Bits &key)
{
    using K = ScopeKind<T>;
    T th, rad;
    K::sample(l, r, ms, fold, th, rad);
    const double deg = (double)K::degrees(th);
    int k = scope_bin(e, bins, inv, deg);
    if (deg == e[bins]) k = -1;                                   // the reference's mask: `<` on the last edge too
    key = K::bits(scope_radius(rad, den));
    return k;
}

// grid = (ceil(n_frames / span), batch); dynamic LDS: the edges, then the bins' counters
template <class T>
__global__ __launch_bounds__(kLevelThreads) void level_stage_kernel(const LevelArgs<T> a)
{
    using K = ScopeKind<T>;
    extern __shared__ __attribute__((aligned(16))) double level_lds[];
    const int64_t b = blockIdx.y;
    int64_t j0, j1;
    if (!scope_span(a.s, b, a.s.span, j0, j1)) return;            // (workgroup-uniform, before any barrier)
    const int bins = a.s.bins0;
    double *e = level_lds;
    unsigned int *cnt = (unsigned int *)(e + (bins + 1));
    for (int i = threadIdx.x; i <= bins; i += kLevelThreads) e[i] = a.s.e0[i];
    for (int i = threadIdx.x; i < bins; i += kLevelThreads) cnt[i] = 0u;
    __syncthreads();
    const double inv = (double)bins / (e[bins] - e[0]);
    const T *__restrict__ pl = a.s.l + b * a.s.stream_stride;
    const T *__restrict__ pr = a.s.r + b * a.s.stream_stride;
    const T den = scope_denominator(a.s, b);
    typename K::Bits *__restrict__ keys = a.keys + b * a.s.n_frames;
    unsigned short *__restrict__ kb = a.bins + b * a.s.n_frames;
    for (int64_t j = j0 + threadIdx.x; j < j1; j += kLevelThreads) {
        T l, r;
        scope_load(a.s, pl, pr, j, l, r);
        typename K::Bits key;
        const int k = level_frame(l, r, a.s.ms != 0, a.s.fold != 0, den, e, bins, inv, key);
        keys[j] = key;
        kb[j] = k < 0 ? kLevelNoBin : (unsigned short)k;
        level_count(cnt, k);
    }
    __syncthreads();
    unsigned int *__restrict__ out = a.bin_counts + b * (int64_t)bins;
    for (int i = threadIdx.x; i < bins; i += kLevelThreads) {
        const unsigned int v = cnt[i];
        if (v) atomicAdd(out + i, v);
    }
}

// a thread per cell: the percentile rule of include/vnd_level.h on the count of the cell's bin
template <class T>
__global__ __launch_bounds__(kLevelCellThreads) void level_init_kernel(const LevelArgs<T> a)
{
    using Bits = typename ScopeKind<T>::Bits;
    const int64_t i = (int64_t)blockIdx.x * kLevelCellThreads + threadIdx.x;
    if (i >= a.cells_all) return;
    const int p = (int)(i % a.num_p);
    const unsigned int m = a.bin_counts[i / a.num_p];
    unsigned int prev = 0, flags = 0;
    T g = (T)0;
    if (m) {
        const T top = (T)(m - 1);                                 // rounded to nearest
        const T v = top * a.q[p];
        flags = kLevelNonEmpty;
        if (v >= top) {
            prev = m - 1;
        } else {
            const T fl = level_floor(v);
            prev = (unsigned int)fl;
            g = v - fl;
            if (prev >= m - 1) prev = m - 1;                      // (cannot happen: v < T(m - 1))
            else flags |= kLevelWantNext;
        }
    }
    a.prefix[i] = (Bits)0;
    a.next[i] = ~(Bits)0;
    a.gamma[i] = g;
    a.rank[i] = prev;
    a.flags[i] = flags;
}

// grid = (ceil(n_frames / span), batch); dynamic LDS: the signal's prefixes, then its digit counters
template <class T>
__global__ __launch_bounds__(kLevelThreads) void level_select_kernel(const LevelArgs<T> a)
{
    using Bits = typename ScopeKind<T>::Bits;
    constexpr int kKeyBits = 8 * (int)sizeof(Bits);
    extern __shared__ __attribute__((aligned(16))) double level_lds[];
    const int64_t b = blockIdx.y;
    int64_t j0, j1;
    if (!scope_span(a.s, b, a.s.span, j0, j1)) return;
    const int bins = a.s.bins0, np = a.num_p, cells = bins * np, total = cells << a.digit_bits;
    Bits *pre = (Bits *)level_lds;
    unsigned int *cnt = (unsigned int *)(pre + cells);
    for (int i = threadIdx.x; i < cells; i += kLevelThreads) pre[i] = a.prefix[b * cells + i];
    for (int i = threadIdx.x; i < total; i += kLevelThreads) cnt[i] = 0u;
    __syncthreads();
    const int hi = a.shift + a.width;                             // the bits from here up are the prefix
    const bool whole = hi >= kKeyBits;
    const int up = whole ? 0 : hi;
    const Bits mask = (Bits)((1u << a.width) - 1u);
    const Bits *__restrict__ keys = a.keys + b * a.s.n_frames;
    const unsigned short *__restrict__ kb = a.bins + b * a.s.n_frames;
    for (int64_t j = j0 + threadIdx.x; j < j1; j += kLevelThreads) {
        const int k = kb[j];
        const Bits key = keys[j];
        const int digit = (int)((key >> a.shift) & mask);
        for (int p = 0; p < np; ++p) {
            int idx = -1;
            if (k < bins) {
                const int c = k * np + p;
                if (whole || ((key ^ pre[c]) >> up) == 0) idx = (c << a.digit_bits) + digit;
            }
            level_count(cnt, idx);
        }
    }
    __syncthreads();
    unsigned int *__restrict__ out = a.hist + b * (int64_t)total;
    for (int i = threadIdx.x; i < total; i += kLevelThreads) {
        const unsigned int v = cnt[i];
        if (v) atomicAdd(out + i, v);
    }
}

// a thread per cell, after a select pass
template <class T>
__global__ __launch_bounds__(kLevelCellThreads) void level_advance_kernel(const LevelArgs<T> a)
{
    using Bits = typename ScopeKind<T>::Bits;
    const int64_t i = (int64_t)blockIdx.x * kLevelCellThreads + threadIdx.x;
    if (i >= a.cells_all) return;
    unsigned int *__restrict__ h = a.hist + (i << a.digit_bits);
    const unsigned int flags = a.flags[i];
    const int digits = 1 << a.width;
    if (flags & kLevelNonEmpty) {
        unsigned int rank = a.rank[i], c = 0;
        int t = 0;
        for (; t < digits; ++t) {
            c = h[t];
            if (rank < c) break;
            rank -= c;
        }
        if (t == digits) { t = digits - 1; rank = 0; c = 1; }     // (cannot happen: the rank is below the bin's count)
        const Bits pre = a.prefix[i] | ((Bits)t << a.shift);
        a.prefix[i] = pre;
        a.rank[i] = rank;
        if (a.last) {                                             // c keys equal sorted[prev]; it is number `rank` of them
            if ((flags & kLevelWantNext) && rank + 1 == c) a.flags[i] = flags | kLevelNeedMin;
            else a.next[i] = pre;
        }
    }
    for (int t = 0; t < digits; ++t) h[t] = 0u;
}

// grid = (ceil(n_frames / span), batch); dynamic LDS: the signal's prefixes, its minima, its flags
template <class T>
__global__ __launch_bounds__(kLevelThreads) void level_min_kernel(const LevelArgs<T> a)
{
    using Bits = typename ScopeKind<T>::Bits;
    extern __shared__ __attribute__((aligned(16))) double level_lds[];
    const int64_t b = blockIdx.y;
    int64_t j0, j1;
    if (!scope_span(a.s, b, a.s.span, j0, j1)) return;
    const int bins = a.s.bins0, np = a.num_p, cells = bins * np;
    Bits *pre = (Bits *)level_lds;
    Bits *mn = pre + cells;
    unsigned int *fl = (unsigned int *)(mn + cells);
    int any = 0;
    for (int i = threadIdx.x; i < cells; i += kLevelThreads) {
        pre[i] = a.prefix[b * cells + i];
        mn[i] = ~(Bits)0;
        const unsigned int f = a.flags[b * cells + i];
        fl[i] = f;
        any |= (f & kLevelNeedMin) != 0;
    }
    if (!__syncthreads_or(any)) return;                           // no cell of this signal asks (workgroup-uniform)
    const Bits *__restrict__ keys = a.keys + b * a.s.n_frames;
    const unsigned short *__restrict__ kb = a.bins + b * a.s.n_frames;
    for (int64_t j = j0 + threadIdx.x; j < j1; j += kLevelThreads) {
        const int k = kb[j];
        if (k >= bins) continue;
        const Bits key = keys[j];
        for (int p = 0; p < np; ++p) {
            const int c = k * np + p;
            if ((fl[c] & kLevelNeedMin) && key > pre[c] && key < mn[c]) atomicMin(mn + c, key);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < cells; i += kLevelThreads)
        if (mn[i] != ~(Bits)0) atomicMin(a.next + b * cells + i, mn[i]);
}

// a thread per output: levels[b][p][bin]
template <class T>
__global__ __launch_bounds__(kLevelCellThreads) void level_finish_kernel(const LevelArgs<T> a)
{
    using K = ScopeKind<T>;
    const int64_t i = (int64_t)blockIdx.x * kLevelCellThreads + threadIdx.x;
    if (i >= a.cells_all) return;
    const int bins = a.s.bins0;
    const int64_t bin = i % bins, p = (i / bins) % a.num_p, b = i / ((int64_t)bins * a.num_p);
    const int64_t cell = (b * bins + bin) * a.num_p + p;
    T out = (T)0;
    if (a.flags[cell] & kLevelNonEmpty) {
        const T lo = K::value(a.prefix[cell]), up = K::value(a.next[cell]), g = a.gamma[cell];
        const T d = up - lo;
        const T w = d * g, w1 = d * ((T)1 - g);                   // every operation rounded on its own (-ffp-contract=off)
        out = g >= (T)0.5 ? up - w1 : lo + w;
    }
    a.levels[i] = out;
}

// The digit width of a call: the widest whose counters and prefixes of one signal fit the LDS budget, but no more counters
// a signal than kLevelCountersPerFrame for each frame a workgroup brings - every pass clears, flushes and walks all of them,
// and at 480 frames a signal that, not the frames, is the traffic: d = 5 measured 1.9 ms on 2048 x 480
// where the frames alone are 6 MB a pass.
constexpr int64_t kLevelCountersPerFrame = 8;

static int level_digit_bits(int64_t n_frames, int32_t bins, int32_t num_p, int64_t key_bytes)
{
    const int64_t cells = (int64_t)bins * num_p;
    const int64_t frames = std::min<int64_t>(n_frames, VND_LEVEL_SPAN_FRAMES);
    int d = 1;                                                    // d = 1 fits within the header's limits
    while (d < kLevelMaxDigitBits && cells * (((int64_t)4 << (d + 1)) + key_bytes) <= VND_SCOPE_LDS_BYTES &&
           (cells << (d + 1)) <= kLevelCountersPerFrame * frames)
        ++d;
    return d;
}

struct LevelLayout {
    int64_t prefix, next, gamma, rank, flags, hist, hist_bytes, keys, bins, total;      // byte offsets; the maximum at 0
    int digit_bits;
};

static int64_t level_align8(int64_t v) { return (v + 7) & ~(int64_t)7; }

// The select's part of the work memory from byte `at` on - the cell state and the digit histograms; `keys` is where it ends.
// (the shape is inside the header's limits: nothing overflows)
static LevelLayout level_select_layout(int64_t at, int64_t batch, int64_t n_frames, int32_t bins, int32_t num_p, int64_t key_bytes)
{
    LevelLayout w{};
    const int64_t cells = batch * bins * num_p;
    w.digit_bits = level_digit_bits(n_frames, bins, num_p, key_bytes);
    w.prefix = at; at += cells * 8;
    w.next = at; at += cells * 8;
    w.gamma = at; at += cells * 8;
    w.rank = at; at += level_align8(cells * 4);
    w.flags = at; at += level_align8(cells * 4);
    w.hist = at; w.hist_bytes = level_align8((cells << w.digit_bits) * 4); at += w.hist_bytes;
    w.keys = w.bins = w.total = at;
    return w;
}

// The one-shot entry's work memory: the per-signal maximum, the select's part, then the staged keys and bins.
static LevelLayout level_layout(int64_t batch, int64_t n_frames, int32_t bins, int32_t num_p, int64_t key_bytes)
{
    LevelLayout w = level_select_layout(batch * 8, batch, n_frames, bins, num_p, key_bytes);
    int64_t at = w.keys;
    at += level_align8(batch * n_frames * key_bytes);
    w.bins = at; at += level_align8(batch * n_frames * 2);
    w.total = at;
    return w;
}

static vnd_status level_check_shape(int64_t batch, int64_t n_frames, int32_t bins, int32_t num_p)
{
    vnd_status st = scope_check_limits(batch, n_frames);
    if (st != VND_OK) return st;
    if (bins > VND_LEVEL_MAX_BINS) return fail(VND_ERR_UNSUPPORTED, "%d bins, above %d", bins, VND_LEVEL_MAX_BINS);
    if (num_p > VND_LEVEL_MAX_PERCENTILES)
        return fail(VND_ERR_UNSUPPORTED, "%d percentiles, above %d", num_p, VND_LEVEL_MAX_PERCENTILES);
    return scope_check_groups(batch, n_frames, VND_LEVEL_SPAN_FRAMES);
}

// The select over staged keys, for both callers (level_dev below; the voice pool's levels entry over its rings,
// vnd_level_voice_stream.hpp).  `a` has keys, bins, bin_counts (counted), s.n_frames, s.step, s.n_each, s.bins0 and s.span, the
// cell state and hist at `w`'s offsets of `base`, levels, num_p and q.  level_select_allow comes before anything is enqueued.
struct LevelSelectLds { size_t select, min; };

template <class T>
static vnd_status level_select_allow(vnd_ctx *ctx, int32_t bins, int32_t num_p, int digit_bits, LevelSelectLds *lds)
{
    using Bits = typename ScopeKind<T>::Bits;
    const int cells = bins * num_p;
    lds->select = (size_t)cells * sizeof(Bits) + ((size_t)cells << digit_bits) * 4;
    lds->min = (size_t)cells * (2 * sizeof(Bits) + 4);
    vnd_status st = allow_lds(ctx, (const void *)level_select_kernel<T>, lds->select);
    if (st != VND_OK) return st;
    return allow_lds(ctx, (const void *)level_min_kernel<T>, lds->min);
}

template <class T>
static void level_fill_select(LevelArgs<T> &a, char *base, const LevelLayout &w, int64_t batch, int32_t bins, const double *percentiles,
                              int32_t num_p)
{
    using Bits = typename ScopeKind<T>::Bits;
    a.prefix = (Bits *)(base + w.prefix); a.next = (Bits *)(base + w.next); a.gamma = (T *)(base + w.gamma);
    a.rank = (unsigned int *)(base + w.rank); a.flags = (unsigned int *)(base + w.flags); a.hist = (unsigned int *)(base + w.hist);
    a.num_p = num_p; a.digit_bits = w.digit_bits; a.cells_all = batch * bins * num_p;
    for (int32_t p = 0; p < num_p; ++p) a.q[p] = (T)percentiles[p] / (T)100;
}

template <class T>
static vnd_status level_run_select(LevelArgs<T> a, const LevelLayout &w, const LevelSelectLds &lds, int64_t batch, hipStream_t stream)
{
    using Bits = typename ScopeKind<T>::Bits;
    HIP_TRY(hipMemsetAsync(a.hist, 0, (size_t)w.hist_bytes, stream));
    const dim3 frames_grid((unsigned)((a.s.n_frames + a.s.span - 1) / a.s.span), (unsigned)batch);
    const dim3 cells_grid((unsigned)((a.cells_all + kLevelCellThreads - 1) / kLevelCellThreads));
    hipLaunchKernelGGL(level_init_kernel<T>, cells_grid, dim3(kLevelCellThreads), 0, stream, a);
    constexpr int kKeyBits = 8 * (int)sizeof(Bits);
    for (int hi = kKeyBits; hi > 0; hi -= w.digit_bits) {
        a.shift = hi > w.digit_bits ? hi - w.digit_bits : 0;
        a.width = hi - a.shift;
        a.last = a.shift == 0;
        hipLaunchKernelGGL(level_select_kernel<T>, frames_grid, dim3(kLevelThreads), lds.select, stream, a);
        hipLaunchKernelGGL(level_advance_kernel<T>, cells_grid, dim3(kLevelCellThreads), 0, stream, a);
    }
    hipLaunchKernelGGL(level_min_kernel<T>, frames_grid, dim3(kLevelThreads), lds.min, stream, a);
    hipLaunchKernelGGL(level_finish_kernel<T>, cells_grid, dim3(kLevelCellThreads), 0, stream, a);
    HIP_TRY(hipGetLastError());
    return VND_OK;
}

template <class T>
static vnd_status level_dev(vnd_ctx *ctx, const T *l, const T *r, int64_t batch, int64_t n_frames, int64_t stream_stride,
                            int32_t frame_stride, int32_t ms_mode, int32_t semicircular, double radius_scale, const double *edges,
                            int32_t bins, const double *percentiles, int32_t num_p, const int32_t *n_each, T *levels,
                            uint32_t *bin_counts, void *work, int64_t work_bytes, void *stream_)
{
    using Bits = typename ScopeKind<T>::Bits;
    int64_t fb = 0;
    vnd_status st = scope_check_pool(l, r, batch, n_frames, stream_stride, frame_stride, (int64_t)sizeof(T), &fb);
    if (st != VND_OK) return st;
    if (!edges || !percentiles || !levels || !bin_counts) return fail(VND_ERR_INVALID, "null edges, percentiles, levels or bin_counts pointer");
    if (bins < 1 || num_p < 1) return fail(VND_ERR_INVALID, "num_bins and num_percentiles must be >= 1");
    for (int32_t p = 0; p < num_p; ++p)
        if (!(percentiles[p] >= 0.0 && percentiles[p] <= 100.0))
            return fail(VND_ERR_INVALID, "percentile %g is not in [0, 100]", percentiles[p]);
    const bool by_max = !(radius_scale > 0.0);
    if (radius_scale != radius_scale) return fail(VND_ERR_INVALID, "radius_scale is NaN");
    if (!by_max && !(radius_scale <= (double)std::numeric_limits<T>::max() && (T)radius_scale > (T)0))
        return fail(VND_ERR_INVALID, "radius_scale %g is zero or infinite in the sample type", radius_scale);
    if (!work) return fail(VND_ERR_INVALID, "null work pointer: the select needs vnd_polar_level_work_bytes of memory");
    if ((uintptr_t)work % 8 != 0) return fail(VND_ERR_INVALID, "the work memory is not 8-byte aligned");
    // What the work memory must hold, and what overlaps, is defined for a supported shape only; an unsupported one is refused
    // right after (g_err keeps the first message).
    const vnd_status shape = level_check_shape(batch, n_frames, bins, num_p);
    if (shape != VND_OK) return shape;
    const LevelLayout w = level_layout(batch, n_frames, bins, num_p, (int64_t)sizeof(Bits));
    if (work_bytes < w.total)
        return fail(VND_ERR_INVALID, "work of %lld bytes, the call needs %lld", (long long)work_bytes, (long long)w.total);
    const int64_t cells_all = batch * bins * num_p;
    const ScopeRegion outs[] = {{levels, cells_all * (int64_t)sizeof(T)}, {bin_counts, batch * bins * 4}, {work, w.total}};
    const ScopeRegion ins[] = {{l, fb}, {r, fb}, {edges, ((int64_t)bins + 1) * 8}, {n_each, batch * 4}};
    for (int i = 0; i < 3; ++i) {
        for (const ScopeRegion &in : ins)
            if (scope_overlap(outs[i].p, outs[i].bytes, in.p, in.bytes))
                return fail(VND_ERR_INVALID, "levels, bin_counts and work must not overlap the frames, the edges or n_each");
        for (int k = i + 1; k < 3; ++k)
            if (scope_overlap(outs[i].p, outs[i].bytes, outs[k].p, outs[k].bytes))
                return fail(VND_ERR_INVALID, "levels, bin_counts and work must not overlap one another");
    }
    if (!ctx) return fail(VND_ERR_INVALID, "null context");
    DeviceScope on(ctx->device);
    if (!on.ok) return fail(VND_ERR_HIP, "cannot select device %d", ctx->device);
    hipStream_t stream = (hipStream_t)stream_;

    char *base = (char *)work;
    LevelArgs<T> a{};
    scope_fill_pool(a.s, l, r, n_frames, stream_stride, frame_stride, 1);
    a.s.n_each = n_each; a.s.e0 = edges; a.s.e1 = edges; a.s.bins0 = bins; a.s.bins1 = 1;
    a.s.work = (unsigned long long *)work; a.s.scale = by_max ? (T)0 : (T)radius_scale; a.s.normalize = by_max;
    a.s.ms = ms_mode != 0; a.s.fold = semicircular != 0; a.s.span = VND_LEVEL_SPAN_FRAMES;
    a.keys = (Bits *)(base + w.keys); a.bins = (unsigned short *)(base + w.bins); a.bin_counts = bin_counts;
    a.levels = levels;
    level_fill_select(a, base, w, batch, bins, percentiles, num_p);

    const size_t stage_lds = (size_t)(bins + 1) * 8 + (size_t)bins * 4;
    LevelSelectLds lds{};
    if ((st = level_select_allow<T>(ctx, bins, num_p, w.digit_bits, &lds)) != VND_OK) return st;

    if (by_max && (st = scope_launch_max(a.s, batch, stream)) != VND_OK) return st;
    HIP_TRY(hipMemsetAsync(bin_counts, 0, (size_t)batch * bins * 4, stream));
    const dim3 frames_grid((unsigned)((n_frames + VND_LEVEL_SPAN_FRAMES - 1) / VND_LEVEL_SPAN_FRAMES), (unsigned)batch);
    hipLaunchKernelGGL(level_stage_kernel<T>, frames_grid, dim3(kLevelThreads), stage_lds, stream, a);
    return level_run_select(a, w, lds, batch, stream);
}

extern "C" {

vnd_status vnd_polar_level_work_bytes(int64_t batch, int64_t n_frames, int32_t num_bins, int32_t num_percentiles,
                                      int32_t is_float64, int64_t *bytes)
{
    if (!bytes) return fail(VND_ERR_INVALID, "null bytes");
    *bytes = 0;
    if (batch < 1 || n_frames < 1 || num_bins < 1 || num_percentiles < 1)
        return fail(VND_ERR_INVALID, "batch, n_frames, num_bins and num_percentiles must be >= 1");
    const vnd_status st = level_check_shape(batch, n_frames, num_bins, num_percentiles);
    if (st != VND_OK) return st;
    *bytes = level_layout(batch, n_frames, num_bins, num_percentiles, is_float64 ? 8 : 4).total;
    return VND_OK;
}

vnd_status vnd_polar_level_f32_dev(vnd_ctx *ctx, const float *l, const float *r, int64_t batch, int64_t n_frames,
                                   int64_t stream_stride, int32_t frame_stride, int32_t ms_mode, int32_t semicircular,
                                   double radius_scale, const double *angle_edges, int32_t num_bins, const double *percentiles,
                                   int32_t num_percentiles, const int32_t *n_each, float *levels, uint32_t *bin_counts, void *work,
                                   int64_t work_bytes, void *stream)
{
    return level_dev<float>(ctx, l, r, batch, n_frames, stream_stride, frame_stride, ms_mode, semicircular, radius_scale, angle_edges,
                            num_bins, percentiles, num_percentiles, n_each, levels, bin_counts, work, work_bytes, stream);
}

vnd_status vnd_polar_level_f64_dev(vnd_ctx *ctx, const double *l, const double *r, int64_t batch, int64_t n_frames,
                                   int64_t stream_stride, int32_t frame_stride, int32_t ms_mode, int32_t semicircular,
                                   double radius_scale, const double *angle_edges, int32_t num_bins, const double *percentiles,
                                   int32_t num_percentiles, const int32_t *n_each, double *levels, uint32_t *bin_counts, void *work,
                                   int64_t work_bytes, void *stream)
{
    return level_dev<double>(ctx, l, r, batch, n_frames, stream_stride, frame_stride, ms_mode, semicircular, radius_scale,
                             angle_edges, num_bins, percentiles, num_percentiles, n_each, levels, bin_counts, work, work_bytes, stream);
}

}  // extern "C"

// vnd_scope.hpp - the vectorscope's data (include/vnd_scope.h): the polar sample of every frame of a pool, and the polar and
// Lissajous count grids, binned on the device.
// (one translation unit: included by vnd_amd.hip after vnd_stage.hpp and vnd_voice_stream.hpp)
//
// The sample of a frame is vnd::polar_sample / polar_sample64 (vnd_polar.hpp) for every kernel here, and the radius
// coordinate is scope_radius below for both the coordinates kernel and the polar histogram: a count grid is the grid of the
// thetas and radii the coordinates kernel writes, cell for cell.
//
// scope_max_kernel, grid (ceil(n / 8192), batch): the per-signal maximum radius as a maximum over bit patterns (radii are
// non-negative, so unsigned order is value order) - a wave's maximum by shuffles, one atomicMax per wave into work[b], which
// the entry cleared on the same stream.  Order-free and exact.
// scope_coords_kernel, grid (ceil(n / 2048), batch): radii and thetas of every frame.
// scope_hist_kernel<T, POLAR, LDS>, grid (ceil(used / span), batch): a workgroup takes `span` consecutive used frames of one
// signal.  It stages both edge arrays in LDS; on the LDS-private route (1024 threads, span VND_SCOPE_SPAN_FRAMES) it clears a
// private grid behind them, bins with LDS atomics and adds its non-zero cells to the global grid; on the direct route (256
// threads, span VND_SCOPE_DIRECT_SPAN_FRAMES) every frame is one atomicAdd(unsigned *) to global memory.  Counts are
// integers: arrival order cannot show.
//
// Every index that is built from device data:
//   - n_each[b] outside [0, n_frames] becomes 0 frames before anything is addressed with it (workgroup-uniform: the
//     workgroup leaves before its first barrier);
//   - a bin comes from scope_bin, which returns -1 or a value in [0, bins - 1] whatever the edges hold: the arithmetic guess
//     is clamped as a double before it becomes an int, the walk of one step either way stays inside because the value was
//     first held to [edges[0], edges[bins]), and the bisection keeps 0 <= lo < hi <= bins.
#pragma once
#include "../../include/vnd_scope.h"

constexpr int kScopeLdsThreads = 1024, kScopeDirectThreads = 256, kScopeThreads = 256;
constexpr int64_t kScopeMaxSpan = 8192, kScopeCoordsSpan = 2048;
constexpr int64_t kScopeMaxGroups = (int64_t)1 << 23;
// The auto choice: LDS-private where the grid fits and a workgroup has at least one frame for every 40
// cells it has to clear and flush - 900 frames a signal on the default polar grid; measured, profiles/scope_hist_rate.json:
// at 36 000 cells direct is ahead at 480 frames a signal (x 1.04 - 1.26) and LDS-private from 1200 on (x 0.91 and falling).
constexpr int64_t kScopeLdsCellsPerFrame = 40;

template <class T> struct ScopeKind;
template <> struct ScopeKind<float> {
    using Bits = unsigned int;
    using Pair = float2;
    __device__ static __forceinline__ void sample(float l, float r, bool ms, bool fold, float &th, float &rad) { vnd::polar_sample(l, r, ms, fold, th, rad); }
    __device__ static __forceinline__ Bits bits(float v) { return __float_as_uint(v); }
    __device__ static __forceinline__ float value(Bits b) { return __uint_as_float(b); }
    __device__ static __forceinline__ float div(float a, float b) { return __fdiv_rn(a, b); }
    __device__ static __forceinline__ float eps() { return 1e-10f; }                                   // float32(EPSILON)
    __device__ static __forceinline__ float degrees(float th) { return th * 57.2957763671875f; }       // float32(180) / float32(pi)
};
template <> struct ScopeKind<double> {
    using Bits = unsigned long long;
    using Pair = double2;
    __device__ static __forceinline__ void sample(double l, double r, bool ms, bool fold, double &th, double &rad) { vnd::polar_sample64(l, r, ms, fold, th, rad); }
    __device__ static __forceinline__ Bits bits(double v) { return (Bits)__double_as_longlong(v); }
    __device__ static __forceinline__ double value(Bits b) { return __longlong_as_double((long long)b); }
    __device__ static __forceinline__ double div(double a, double b) { return a / b; }
    __device__ static __forceinline__ double eps() { return 1e-10; }
    __device__ static __forceinline__ double degrees(double th) { return th * (180.0 / 3.141592653589793); }
};

template <class T>
struct ScopeArgs {
    const T *__restrict__ l;            // used frame j of signal b at b * stream_stride + j * frame_stride (the step folded in)
    const T *__restrict__ r;
    int64_t stream_stride, frame_stride;
    int64_t n_frames, step;             // frames of a signal, and every step-th of them is used
    const int32_t *__restrict__ n_each; // or null
    const double *__restrict__ e0;      // bins0 + 1 edges of coordinate 0
    const double *__restrict__ e1;
    int32_t bins0, bins1;
    unsigned int *__restrict__ counts;  // [batch][bins0][bins1]
    T *__restrict__ radii;              // coordinates kernel: [batch][n_frames]
    T *__restrict__ thetas;
    unsigned long long *__restrict__ work;      // [batch]: the bit pattern of the largest radius (low word for float32)
    T scale;                            // > 0: radius / scale;  otherwise the per-signal maximum, if `normalize`
    int32_t normalize, ms, fold, packed;        // packed: r == l + 1 on even strides, 2-element aligned - one load a frame
    int64_t span;                       // used frames per workgroup
};

// The used frames [j0, j1) of this workgroup; false when there are none (workgroup-uniform).
template <class T>
__device__ __forceinline__ bool scope_span(const ScopeArgs<T> &a, int64_t b, int64_t span, int64_t &j0, int64_t &j1)
{
    int64_t n = a.n_frames;
    if (a.n_each) {
        const int32_t v = __builtin_amdgcn_readfirstlane(a.n_each[b]);
        n = (v >= 0 && (int64_t)v <= a.n_frames) ? (int64_t)v : 0;
    }
    const int64_t used = (n + a.step - 1) / a.step;
    j0 = (int64_t)blockIdx.x * span;
    j1 = j0 + span < used ? j0 + span : used;
    return j0 < j1;
}

template <class T>
__device__ __forceinline__ void scope_load(const ScopeArgs<T> &a, const T *pl, const T *pr, int64_t j, T &l, T &r)
{
    const int64_t i = j * a.frame_stride;
    if (a.packed) {
        const typename ScopeKind<T>::Pair v = *(const typename ScopeKind<T>::Pair *)(pl + i);
        l = v.x; r = v.y;
    } else {
        l = pl[i]; r = pr[i];
    }
}

// What a radius is divided by for signal b: the caller's scale, or max_b + eps; 0 when it is not divided at all.
template <class T>
__device__ __forceinline__ T scope_denominator(const ScopeArgs<T> &a, int64_t b)
{
    using K = ScopeKind<T>;
    if (a.scale > (T)0) return a.scale;
    if (!a.normalize) return (T)0;
    const unsigned long long w = a.work[b];
    return K::value((typename K::Bits)w) + K::eps();
}

template <class T>
__device__ __forceinline__ T scope_radius(T rad, T den) { return den > (T)0 ? ScopeKind<T>::div(rad, den) : rad; }

// np.histogramdd's bin of v on `bins + 1` ascending edges e: -1 when the frame is dropped.  inv = bins / (e[bins] - e[0]).
__device__ __forceinline__ int scope_bin(const double *e, int bins, double inv, double v)
{
    if (!(v >= e[0] && v <= e[bins])) return -1;                  // outside, NaN
    if (v == e[bins]) return bins - 1;
    const double g = (v - e[0]) * inv;                            // the guess of evenly spaced edges; the edges decide
    int k = g >= (double)(bins - 1) ? bins - 1 : (g > 0.0 ? (int)g : 0);
    if (v < e[k]) {                                               // e[0] <= v: k >= 1 here
        --k;
        if (v >= e[k]) return k;
    } else {
        if (v < e[k + 1]) return k;
        ++k;                                                      // v < e[bins]: k <= bins - 1 here
        if (v < e[k + 1]) return k;
    }
    int lo = 0, hi = bins;                                        // uneven edges: e[lo] <= v < e[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (v >= e[mid]) lo = mid; else hi = mid;
    }
    return lo;
}

// grid = (ceil(n_frames / kScopeMaxSpan), batch); work cleared before it on the same stream
template <class T>
__global__ __launch_bounds__(kScopeThreads) void scope_max_kernel(const ScopeArgs<T> a)
{
    using K = ScopeKind<T>;
    const int64_t b = blockIdx.y;
    int64_t j0, j1;
    if (!scope_span(a, b, kScopeMaxSpan, j0, j1)) return;
    const T *__restrict__ pl = a.l + b * a.stream_stride;
    const T *__restrict__ pr = a.r + b * a.stream_stride;
    typename K::Bits m = 0;
    for (int64_t j = j0 + threadIdx.x; j < j1; j += kScopeThreads) {
        T l, r, th, rad;
        scope_load(a, pl, pr, j, l, r);
        K::sample(l, r, a.ms != 0, a.fold != 0, th, rad);
        const typename K::Bits v = K::bits(rad);
        m = v > m ? v : m;
    }
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) {
        const typename K::Bits o = __shfl_xor(m, sh);
        m = o > m ? o : m;
    }
    if ((threadIdx.x & 63) == 0 && m != 0) atomicMax((typename K::Bits *)(a.work + b), m);      // little-endian: the low word
}

// grid = (ceil(n_frames / kScopeCoordsSpan), batch)
template <class T>
__global__ __launch_bounds__(kScopeThreads) void scope_coords_kernel(const ScopeArgs<T> a)
{
    using K = ScopeKind<T>;
    const int64_t b = blockIdx.y;
    int64_t j0, j1;
    if (!scope_span(a, b, kScopeCoordsSpan, j0, j1)) return;
    const T *__restrict__ pl = a.l + b * a.stream_stride;
    const T *__restrict__ pr = a.r + b * a.stream_stride;
    const T den = scope_denominator(a, b);
    for (int64_t j = j0 + threadIdx.x; j < j1; j += kScopeThreads) {
        T l, r, th, rad;
        scope_load(a, pl, pr, j, l, r);
        K::sample(l, r, a.ms != 0, a.fold != 0, th, rad);
        a.radii[b * a.n_frames + j] = scope_radius(rad, den);
        a.thetas[b * a.n_frames + j] = th;
    }
}

// grid = (ceil(used / span), batch); dynamic LDS: the edges, then (LDS) the private grid
template <class T, bool POLAR, bool LDS>
__global__ __launch_bounds__(LDS ? kScopeLdsThreads : kScopeDirectThreads) void scope_hist_kernel(const ScopeArgs<T> a)
{
    using K = ScopeKind<T>;
    constexpr int kThreads = LDS ? kScopeLdsThreads : kScopeDirectThreads;
    extern __shared__ __attribute__((aligned(16))) double scope_lds[];
    const int64_t b = blockIdx.y;
    int64_t j0, j1;
    if (!scope_span(a, b, a.span, j0, j1)) return;                // (workgroup-uniform, before any barrier)
    double *e0 = scope_lds, *e1 = scope_lds + (a.bins0 + 1);
    unsigned int *grid = (unsigned int *)(e1 + (a.bins1 + 1));
    const int cells = a.bins0 * a.bins1;
    for (int i = threadIdx.x; i <= a.bins0; i += kThreads) e0[i] = a.e0[i];
    for (int i = threadIdx.x; i <= a.bins1; i += kThreads) e1[i] = a.e1[i];
    if (LDS)
        for (int c = threadIdx.x; c < cells; c += kThreads) grid[c] = 0u;
    __syncthreads();
    const double inv0 = (double)a.bins0 / (e0[a.bins0] - e0[0]), inv1 = (double)a.bins1 / (e1[a.bins1] - e1[0]);
    const T *__restrict__ pl = a.l + b * a.stream_stride;
    const T *__restrict__ pr = a.r + b * a.stream_stride;
    unsigned int *__restrict__ out = a.counts + b * (int64_t)cells;
    const T den = POLAR ? scope_denominator(a, b) : (T)0;
    for (int64_t j = j0 + threadIdx.x; j < j1; j += kThreads) {
        T l, r;
        scope_load(a, pl, pr, j, l, r);
        double v0, v1;
        if (POLAR) {
            T th, rad;
            K::sample(l, r, a.ms != 0, a.fold != 0, th, rad);
            v0 = (double)K::degrees(th);
            v1 = (double)scope_radius(rad, den);
        } else {
            v0 = (double)l;
            v1 = (double)r;
        }
        const int k0 = scope_bin(e0, a.bins0, inv0, v0);
        if (k0 < 0) continue;
        const int k1 = scope_bin(e1, a.bins1, inv1, v1);
        if (k1 < 0) continue;
        const int c = k0 * a.bins1 + k1;
        if (LDS) atomicAdd(grid + c, 1u);
        else atomicAdd(out + c, 1u);
    }
    if (LDS) {
        __syncthreads();
        for (int c = threadIdx.x; c < cells; c += kThreads) {
            const unsigned int v = grid[c];
            if (v) atomicAdd(out + c, v);
        }
    }
}

static int64_t scope_edge_bytes(int32_t bins0, int32_t bins1) { return ((int64_t)bins0 + bins1 + 2) * (int64_t)sizeof(double); }

static bool scope_fits_lds(int32_t bins0, int32_t bins1)
{
    return (int64_t)bins0 * bins1 * 4 + scope_edge_bytes(bins0, bins1) <= VND_SCOPE_LDS_BYTES;
}

// VND_SCOPE_ROUTE of a tuning session, read at the call (vnd_spec.hpp: the registry of tuning variables)
static int scope_route_setting()
{
    for (const TuningName &v : kTuningNames)
        if (v.field == &Tuning::scope_route) return tuning_value(v, 0);
    return 0;
}

static int scope_pick_route(int32_t bins0, int32_t bins1, int64_t used)
{
    const bool fits = scope_fits_lds(bins0, bins1);
    const int setting = scope_route_setting();
    if (setting == VND_SCOPE_ROUTE_DIRECT || !fits) return VND_SCOPE_ROUTE_DIRECT;
    if (setting == VND_SCOPE_ROUTE_LDS) return VND_SCOPE_ROUTE_LDS;
    const int64_t per_group = std::min<int64_t>(used, VND_SCOPE_SPAN_FRAMES);
    return per_group * kScopeLdsCellsPerFrame >= (int64_t)bins0 * bins1 ? VND_SCOPE_ROUTE_LDS : VND_SCOPE_ROUTE_DIRECT;
}

static bool scope_overlap(const void *u, int64_t ub, const void *v, int64_t vb)
{
    const char *u0 = (const char *)u, *v0 = (const char *)v;
    return u && v && u0 < v0 + vb && v0 < u0 + ub;
}

struct ScopeRegion { const void *p; int64_t bytes; };

// "These outputs overlap none of these inputs, nor one another": 0, or 1 for an output on an input and 2 for two outputs - the
// caller has a message for each.  by_output: output i is held against the inputs and against the outputs after it before
// output i + 1 is looked at; else every output against the inputs first.  (The order decides which message a call gets.)
static int scope_clash(const ScopeRegion *outs, int n_out, const ScopeRegion *ins, int n_in, bool by_output)
{
    for (int pass = 0; pass < 2; ++pass)
        for (int i = 0; i < n_out; ++i) {
            for (int k = 0; pass == 0 && k < n_in; ++k)
                if (scope_overlap(outs[i].p, outs[i].bytes, ins[k].p, ins[k].bytes)) return 1;
            for (int k = i + 1; pass == (by_output ? 0 : 1) && k < n_out; ++k)
                if (scope_overlap(outs[i].p, outs[i].bytes, outs[k].p, outs[k].bytes)) return 2;
        }
    return 0;
}

// The checks every entry shares: the pool's shape and extent (frame_bytes: what l and r each span), then the limits.
static vnd_status scope_check_pool(const void *l, const void *r, int64_t batch, int64_t n_frames, int64_t stream_stride,
                                   int32_t frame_stride, int64_t sample_bytes, int64_t *frame_bytes)
{
    if (!l || !r) return fail(VND_ERR_INVALID, "null frame pointer");
    if (batch < 1 || n_frames < 1) return fail(VND_ERR_INVALID, "batch and n_frames must be >= 1");
    if (stream_stride < 1 || frame_stride < 1) return fail(VND_ERR_INVALID, "strides must be >= 1");
    int64_t span, last;
    if (__builtin_mul_overflow(batch - 1, stream_stride, &span) ||
        __builtin_mul_overflow(n_frames - 1, (int64_t)frame_stride, &last) ||
        __builtin_add_overflow(span, last, &span) || span > INT64_MAX / 16)
        return fail(VND_ERR_INVALID, "buffer extents overflow");
    *frame_bytes = (span + 1) * sample_bytes;
    return VND_OK;
}

static vnd_status scope_check_limits(int64_t batch, int64_t n_frames)
{
    if (n_frames > (int64_t)UINT32_MAX)
        return fail(VND_ERR_UNSUPPORTED, "n_frames %lld above 2^32 - 1: counts are uint32", (long long)n_frames);
    if (batch > VND_MAX_STREAMS) return fail(VND_ERR_UNSUPPORTED, "batch %lld above %d: split the pool", (long long)batch, VND_MAX_STREAMS);
    return VND_OK;
}

static vnd_status scope_check_groups(int64_t batch, int64_t used, int64_t span)
{
    const int64_t groups = (used + span - 1) / span;
    if (groups * batch > kScopeMaxGroups)
        return fail(VND_ERR_UNSUPPORTED, "%lld workgroups in one launch, above 2^23: split the pool", (long long)(groups * batch));
    return VND_OK;
}

static vnd_status scope_check_work(const void *work, int64_t work_bytes, int64_t batch)
{
    if (!work) return fail(VND_ERR_INVALID, "null work pointer: the per-signal maximum needs vnd_scope_work_bytes of memory");
    if (work_bytes < batch * 8)
        return fail(VND_ERR_INVALID, "work of %lld bytes, the pool needs %lld", (long long)work_bytes, (long long)(batch * 8));
    if ((uintptr_t)work % 8 != 0) return fail(VND_ERR_INVALID, "the work memory is not 8-byte aligned");
    return VND_OK;
}

template <class T>
static void scope_fill_pool(ScopeArgs<T> &a, const T *l, const T *r, int64_t n_frames, int64_t stream_stride, int64_t frame_stride,
                            int64_t step)
{
    a.l = l; a.r = r; a.n_frames = n_frames; a.stream_stride = stream_stride; a.step = step;
    a.frame_stride = frame_stride * step;
    a.packed = r == l + 1 && stream_stride % 2 == 0 && a.frame_stride % 2 == 0 && (uintptr_t)l % (2 * sizeof(T)) == 0;
}

template <class T>
static vnd_status scope_launch_max(const ScopeArgs<T> &a, int64_t batch, hipStream_t stream)
{
    HIP_TRY(hipMemsetAsync(a.work, 0, (size_t)batch * 8, stream));
    const int64_t groups = (a.n_frames + kScopeMaxSpan - 1) / kScopeMaxSpan;
    hipLaunchKernelGGL(scope_max_kernel<T>, dim3((unsigned)groups, (unsigned)batch), dim3(kScopeThreads), 0, stream, a);
    HIP_TRY(hipGetLastError());
    return VND_OK;
}

template <class T>
static vnd_status scope_coords_dev(vnd_ctx *ctx, const T *l, const T *r, int64_t batch, int64_t n_frames, int64_t stream_stride,
                                   int32_t frame_stride, int32_t ms_mode, int32_t semicircular, int32_t normalize, T *radii,
                                   T *thetas, void *work, int64_t work_bytes, void *stream_)
{
    int64_t fb = 0;
    vnd_status st = scope_check_pool(l, r, batch, n_frames, stream_stride, frame_stride, (int64_t)sizeof(T), &fb);
    if (st != VND_OK) return st;
    if (!radii || !thetas) return fail(VND_ERR_INVALID, "null radii or thetas pointer");
    if (normalize && (st = scope_check_work(work, work_bytes, batch)) != VND_OK) return st;
    if (batch > INT64_MAX / 16 / n_frames) return fail(VND_ERR_INVALID, "buffer extents overflow");
    const int64_t ob = batch * n_frames * (int64_t)sizeof(T), wb = normalize ? batch * 8 : 0;
    const ScopeRegion outs[] = {{radii, ob}, {thetas, ob}, {normalize ? work : nullptr, wb}}, ins[] = {{l, fb}, {r, fb}};
    if (const int hit = scope_clash(outs, 3, ins, 2, true))
        return fail(VND_ERR_INVALID, "radii, thetas and work must not overlap %s", hit == 1 ? "the frames" : "one another");
    if ((st = scope_check_limits(batch, n_frames)) != VND_OK) return st;
    if ((st = scope_check_groups(batch, n_frames, kScopeCoordsSpan)) != VND_OK) return st;
    if (!ctx) return fail(VND_ERR_INVALID, "null context");
    DeviceScope on(ctx->device);
    if (!on.ok) return fail(VND_ERR_HIP, "cannot select device %d", ctx->device);
    hipStream_t stream = (hipStream_t)stream_;

    ScopeArgs<T> a{};
    scope_fill_pool(a, l, r, n_frames, stream_stride, frame_stride, 1);
    a.radii = radii; a.thetas = thetas; a.work = (unsigned long long *)work;
    a.normalize = normalize != 0; a.ms = ms_mode != 0; a.fold = semicircular != 0;
    if (a.normalize && (st = scope_launch_max(a, batch, stream)) != VND_OK) return st;
    const int64_t groups = (n_frames + kScopeCoordsSpan - 1) / kScopeCoordsSpan;
    hipLaunchKernelGGL(scope_coords_kernel<T>, dim3((unsigned)groups, (unsigned)batch), dim3(kScopeThreads), 0, stream, a);
    HIP_TRY(hipGetLastError());
    return VND_OK;
}

// Both histograms.  POLAR: radius_scale > 0 a fixed scale, otherwise the per-signal maximum through `work`.
template <class T, bool POLAR>
static vnd_status scope_hist_dev(vnd_ctx *ctx, const T *l, const T *r, int64_t batch, int64_t n_frames, int64_t stream_stride,
                                 int32_t frame_stride, int64_t frame_step, int32_t ms_mode, int32_t semicircular,
                                 double radius_scale, const double *e0, int32_t bins0, const double *e1, int32_t bins1,
                                 const int32_t *n_each, uint32_t *counts, int32_t accumulate, void *work, int64_t work_bytes,
                                 void *stream_)
{
    int64_t fb = 0;
    vnd_status st = scope_check_pool(l, r, batch, n_frames, stream_stride, frame_stride, (int64_t)sizeof(T), &fb);
    if (st != VND_OK) return st;
    if (!e0 || !e1 || !counts) return fail(VND_ERR_INVALID, "null edges or counts pointer");
    if (bins0 < 1 || bins1 < 1) return fail(VND_ERR_INVALID, "bin counts must be >= 1");
    if (frame_step < 1) return fail(VND_ERR_INVALID, "frame_step must be >= 1");
    const bool by_max = POLAR && !(radius_scale > 0.0);
    if (POLAR) {
        if (radius_scale != radius_scale) return fail(VND_ERR_INVALID, "radius_scale is NaN");
        if (!by_max && !(radius_scale <= (double)std::numeric_limits<T>::max() && (T)radius_scale > (T)0))
            return fail(VND_ERR_INVALID, "radius_scale %g is zero or infinite in the sample type", radius_scale);
        if (by_max && accumulate)
            return fail(VND_ERR_INVALID, "accumulate with the per-signal maximum (radius_scale <= 0): a later block's maximum would "
                                         "rescale the earlier frames");
        if (by_max && (st = scope_check_work(work, work_bytes, batch)) != VND_OK) return st;
    }
    const bool bins_ok = bins0 <= VND_SCOPE_MAX_BINS && bins1 <= VND_SCOPE_MAX_BINS;
    // (bin counts above the limit are refused below; here they only must not overflow)
    const int64_t cells = (int64_t)bins0 * bins1;
    if (batch > INT64_MAX / 16 / cells) return fail(VND_ERR_INVALID, "buffer extents overflow");
    const int64_t cb = batch * cells * 4, wb = by_max ? batch * 8 : 0;
    const ScopeRegion outs[] = {{counts, cb}, {by_max ? work : nullptr, wb}};
    const ScopeRegion ins[] = {{l, fb}, {r, fb}, {e0, ((int64_t)bins0 + 1) * 8}, {e1, ((int64_t)bins1 + 1) * 8},
                               {n_each, batch * 4}};
    if (const int hit = scope_clash(outs, 2, ins, 5, false))
        return fail(VND_ERR_INVALID, "counts and work must not overlap %s", hit == 1 ? "the frames, the edges or n_each" : "one another");
    if ((st = scope_check_limits(batch, n_frames)) != VND_OK) return st;
    if (!bins_ok) return fail(VND_ERR_UNSUPPORTED, "%d x %d bins, above %d an axis", bins0, bins1, VND_SCOPE_MAX_BINS);
    if (frame_step > n_frames) frame_step = n_frames;             // frame 0 alone either way, and no product can overflow
    const int64_t used = (n_frames + frame_step - 1) / frame_step;
    const int route = scope_pick_route(bins0, bins1, used);
    const bool lds = route == VND_SCOPE_ROUTE_LDS;
    const int64_t span = lds ? VND_SCOPE_SPAN_FRAMES : VND_SCOPE_DIRECT_SPAN_FRAMES;
    if ((st = scope_check_groups(batch, used, span)) != VND_OK) return st;
    if (!ctx) return fail(VND_ERR_INVALID, "null context");
    DeviceScope on(ctx->device);
    if (!on.ok) return fail(VND_ERR_HIP, "cannot select device %d", ctx->device);
    hipStream_t stream = (hipStream_t)stream_;

    ScopeArgs<T> a{};
    scope_fill_pool(a, l, r, n_frames, stream_stride, frame_stride, frame_step);
    a.n_each = n_each; a.e0 = e0; a.e1 = e1; a.bins0 = bins0; a.bins1 = bins1; a.counts = counts;
    a.work = (unsigned long long *)work; a.scale = by_max || !POLAR ? (T)0 : (T)radius_scale; a.normalize = by_max;
    a.ms = ms_mode != 0; a.fold = semicircular != 0; a.span = span;
    if (by_max && (st = scope_launch_max(a, batch, stream)) != VND_OK) return st;
    if (!accumulate) HIP_TRY(hipMemsetAsync(counts, 0, (size_t)cb, stream));
    const size_t lds_bytes = (size_t)scope_edge_bytes(bins0, bins1) + (lds ? (size_t)cells * 4 : 0);
    const dim3 grid((unsigned)((used + span - 1) / span), (unsigned)batch);
    if (lds) {
        const void *kernel = (const void *)scope_hist_kernel<T, POLAR, true>;
        if ((st = allow_lds(ctx, kernel, lds_bytes)) != VND_OK) return st;
        hipLaunchKernelGGL((scope_hist_kernel<T, POLAR, true>), grid, dim3(kScopeLdsThreads), lds_bytes, stream, a);
    } else {
        const void *kernel = (const void *)scope_hist_kernel<T, POLAR, false>;
        if ((st = allow_lds(ctx, kernel, lds_bytes)) != VND_OK) return st;
        hipLaunchKernelGGL((scope_hist_kernel<T, POLAR, false>), grid, dim3(kScopeDirectThreads), lds_bytes, stream, a);
    }
    HIP_TRY(hipGetLastError());
    return VND_OK;
}

extern "C" {

vnd_status vnd_scope_work_bytes(int64_t batch, int64_t *bytes)
{
    if (!bytes) return fail(VND_ERR_INVALID, "null bytes");
    *bytes = 0;
    if (batch < 1) return fail(VND_ERR_INVALID, "batch must be >= 1");
    if (batch > VND_MAX_STREAMS) return fail(VND_ERR_UNSUPPORTED, "batch %lld above %d: split the pool", (long long)batch, VND_MAX_STREAMS);
    *bytes = batch * 8;
    return VND_OK;
}

vnd_status vnd_scope_route(int32_t bins0, int32_t bins1, int64_t used_frames, int32_t *route)
{
    if (!route) return fail(VND_ERR_INVALID, "null route");
    *route = 0;
    if (bins0 < 1 || bins1 < 1 || used_frames < 1) return fail(VND_ERR_INVALID, "bin counts and used_frames must be >= 1");
    if (bins0 > VND_SCOPE_MAX_BINS || bins1 > VND_SCOPE_MAX_BINS)
        return fail(VND_ERR_UNSUPPORTED, "%d x %d bins, above %d an axis", bins0, bins1, VND_SCOPE_MAX_BINS);
    *route = scope_pick_route(bins0, bins1, used_frames);
    return VND_OK;
}

vnd_status vnd_polar_coords_f32_dev(vnd_ctx *ctx, const float *l, const float *r, int64_t batch, int64_t n_frames,
                                    int64_t stream_stride, int32_t frame_stride, int32_t ms_mode, int32_t semicircular,
                                    int32_t normalize, float *radii, float *thetas, void *work, int64_t work_bytes, void *stream)
{
    return scope_coords_dev<float>(ctx, l, r, batch, n_frames, stream_stride, frame_stride, ms_mode, semicircular, normalize, radii,
                                   thetas, work, work_bytes, stream);
}

vnd_status vnd_polar_coords_f64_dev(vnd_ctx *ctx, const double *l, const double *r, int64_t batch, int64_t n_frames,
                                    int64_t stream_stride, int32_t frame_stride, int32_t ms_mode, int32_t semicircular,
                                    int32_t normalize, double *radii, double *thetas, void *work, int64_t work_bytes, void *stream)
{
    return scope_coords_dev<double>(ctx, l, r, batch, n_frames, stream_stride, frame_stride, ms_mode, semicircular, normalize, radii,
                                    thetas, work, work_bytes, stream);
}

vnd_status vnd_polar_hist_f32_dev(vnd_ctx *ctx, const float *l, const float *r, int64_t batch, int64_t n_frames,
                                  int64_t stream_stride, int32_t frame_stride, int32_t ms_mode, int32_t semicircular,
                                  double radius_scale, const double *angle_edges, int32_t num_angle_bins,
                                  const double *radius_edges, int32_t num_radius_bins, const int32_t *n_each, uint32_t *counts,
                                  int32_t accumulate, void *work, int64_t work_bytes, void *stream)
{
    return scope_hist_dev<float, true>(ctx, l, r, batch, n_frames, stream_stride, frame_stride, 1, ms_mode, semicircular, radius_scale,
                                       angle_edges, num_angle_bins, radius_edges, num_radius_bins, n_each, counts, accumulate, work,
                                       work_bytes, stream);
}

vnd_status vnd_polar_hist_f64_dev(vnd_ctx *ctx, const double *l, const double *r, int64_t batch, int64_t n_frames,
                                  int64_t stream_stride, int32_t frame_stride, int32_t ms_mode, int32_t semicircular,
                                  double radius_scale, const double *angle_edges, int32_t num_angle_bins,
                                  const double *radius_edges, int32_t num_radius_bins, const int32_t *n_each, uint32_t *counts,
                                  int32_t accumulate, void *work, int64_t work_bytes, void *stream)
{
    return scope_hist_dev<double, true>(ctx, l, r, batch, n_frames, stream_stride, frame_stride, 1, ms_mode, semicircular, radius_scale,
                                        angle_edges, num_angle_bins, radius_edges, num_radius_bins, n_each, counts, accumulate, work,
                                        work_bytes, stream);
}

vnd_status vnd_lissajous_hist_f32_dev(vnd_ctx *ctx, const float *l, const float *r, int64_t batch, int64_t n_frames,
                                      int64_t stream_stride, int32_t frame_stride, int64_t frame_step, const double *x_edges,
                                      int32_t x_bins, const double *y_edges, int32_t y_bins, const int32_t *n_each, uint32_t *counts,
                                      int32_t accumulate, void *stream)
{
    return scope_hist_dev<float, false>(ctx, l, r, batch, n_frames, stream_stride, frame_stride, frame_step, 0, 0, 0.0, x_edges, x_bins,
                                        y_edges, y_bins, n_each, counts, accumulate, nullptr, 0, stream);
}

vnd_status vnd_lissajous_hist_f64_dev(vnd_ctx *ctx, const double *l, const double *r, int64_t batch, int64_t n_frames,
                                      int64_t stream_stride, int32_t frame_stride, int64_t frame_step, const double *x_edges,
                                      int32_t x_bins, const double *y_edges, int32_t y_bins, const int32_t *n_each, uint32_t *counts,
                                      int32_t accumulate, void *stream)
{
    return scope_hist_dev<double, false>(ctx, l, r, batch, n_frames, stream_stride, frame_stride, frame_step, 0, 0, 0.0, x_edges, x_bins,
                                         y_edges, y_bins, n_each, counts, accumulate, nullptr, 0, stream);
}

}  // extern "C"

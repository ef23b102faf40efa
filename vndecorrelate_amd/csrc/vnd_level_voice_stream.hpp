// vnd_level_voice_stream.hpp - the polar level envelope of a voice pool (include/vnd_polar_level_voice_stream.h): the per-slice
// percentiles of vnd_level.hpp over the last W frames of every voice, the signal arriving block by block, the position per
// slot in the device state and a count and start / end flags per slot and call.
// (one translation unit: included by vnd_amd.hip after vnd_level.hpp, vnd_voice_core.hpp and vnd_voice_window.hpp)
//
// Percentiles of blocks do not add up, so the state keeps the window itself: per slot a ring of keys and a ring of slices,
// entry g mod W what level_stage_kernel would stage for the voice's frame g - through level_frame, the one function both
// kernels call.  An order statistic does not depend on the order of its multiset: the select runs over the ring as it lies.
//
// PUSH, two launches on the caller's stream, grids fixed by (slots, M):
//   level_voice_stage_kernel, the walk of vnd_voice_window.hpp: idle slots, bad slots and workgroups past n leave before the
//     edges are staged.  Frame j of the chunk is the voice's frame g = p + j; the lane writes its key and slice to entry
//     g mod W.  It reads nothing of the rings.
//   voice_advance_kernel<LevelVoiceArgs<T>> (vnd_voice_core.hpp) writes valid[b] and pos[b]; the slot's advance() also writes
//     fill[b] = min(p + n, W), by the same lane, for a slot that answers 1.
// The slot rule is scope_voice_span's (vnd_voice_window.hpp) as it stands; its `clear` is not used: nothing is cleared.
//
// LEVELS, a pure function of the state: a memset of bin_counts, level_voice_count_kernel (grid (ceil(W / span), slots): the
// slices of ring entries [0, fill) counted in LDS through level_count and added to bin_counts), then level_run_select of
// vnd_level.hpp with LevelArgs pointing keys / bins at the rings, n_frames = W and n_each = fill - scope_span's rule for
// n_each makes a fill outside [0, W] no frames at all.
//
// Ring: the argument of vnd_voice_window.hpp, with the slot rule and the indices built from device data.  What is this pool's:
// fill is a prefix length - a voice that has pushed q < W frames owns [0, q), one that has pushed more owns the whole ring;
// what lies beyond fill is a previous voice's and is never read - and fill[b] and the staged slices meet, in the levels
// kernels, scope_span and the `k < bins` compare of vnd_level.hpp.
#pragma once
#include "../../include/vnd_polar_level_voice_stream.h"

template <class T>
struct LevelVoiceArgs {
    using Bits = typename ScopeKind<T>::Bits;
    ScopeArgs<T> s;                     // the chunk (l, r, strides, packed), the angle edges (e0, bins0), scale, ms, fold
    Bits *__restrict__ keys;            // [slots][W]: the key of frame g at g mod W
    unsigned short *__restrict__ bins;  // [slots][W]: its slice, kLevelNoBin for none
    int64_t *__restrict__ pos;          // [slots]
    int32_t *__restrict__ fill;         // [slots]: ring entries [0, fill) are the voice's
    const int32_t *__restrict__ counts;
    const int32_t *__restrict__ flags;
    int32_t *__restrict__ out_counts;   // valid [slots]
    int64_t slots, M, W;
    __device__ vnd::VoiceAnswer advance(int64_t b) const
    {
        const ScopeVoiceSpan v = scope_voice_span(pos[b], counts[b], flags[b], M);
        if (v.valid == 1) fill[b] = (int32_t)(v.p + v.n < W ? v.p + v.n : W);     // (the lane that moves pos[b] on)
        return {v.valid, v.valid == 1, v.next};
    }
};

// grid = (ceil(M / kScopeVoiceSpan), slots); dynamic LDS: the edges
template <class T>
__global__ __launch_bounds__(kScopeVoiceThreads) void level_voice_stage_kernel(const LevelVoiceArgs<T> a)
{
    extern __shared__ __attribute__((aligned(16))) double level_voice_lds[];
    const int64_t b = blockIdx.y;
    VoiceWindowWalk w;
    if (!w.open(a.pos, a.counts, a.flags, a.M, b, blockIdx.x)) return;
    const int bins = a.s.bins0;
    double *e = level_voice_lds;
    for (int i = threadIdx.x; i <= bins; i += kScopeVoiceThreads) e[i] = a.s.e0[i];
    __syncthreads();
    const double inv = (double)bins / (e[bins] - e[0]);
    const T *__restrict__ pl = a.s.l + b * a.s.stream_stride;
    const T *__restrict__ pr = a.s.r + b * a.s.stream_stride;
    typename ScopeKind<T>::Bits *__restrict__ keys = a.keys + b * a.W;
    unsigned short *__restrict__ kb = a.bins + b * a.W;
    w.enter(a.W);
    for (int64_t j = w.j0 + threadIdx.x; j < w.j1; j += kScopeVoiceThreads) {
        T l, r;
        scope_load(a.s, pl, pr, j, l, r);
        typename ScopeKind<T>::Bits key;
        const int k = level_frame(l, r, a.s.ms != 0, a.s.fold != 0, a.s.scale, e, bins, inv, key);
        const int64_t slot = w.entry(j);
        keys[slot] = key;
        kb[slot] = k < 0 ? kLevelNoBin : (unsigned short)k;
    }
}

// grid = (ceil(W / span), slots); dynamic LDS: the slices' counters.  bin_counts is zero before.
template <class T>
__global__ __launch_bounds__(kLevelThreads) void level_voice_count_kernel(const LevelArgs<T> a)
{
    extern __shared__ __attribute__((aligned(16))) double level_voice_lds[];
    const int64_t b = blockIdx.y;
    int64_t j0, j1;
    if (!scope_span(a.s, b, a.s.span, j0, j1)) return;            // (workgroup-uniform, before any barrier)
    const int bins = a.s.bins0;
    unsigned int *cnt = (unsigned int *)level_voice_lds;
    for (int i = threadIdx.x; i < bins; i += kLevelThreads) cnt[i] = 0u;
    __syncthreads();
    const unsigned short *__restrict__ kb = a.bins + b * a.s.n_frames;
    for (int64_t j = j0 + threadIdx.x; j < j1; j += kLevelThreads) {
        const int k = kb[j];
        level_count(cnt, k < bins ? k : -1);
    }
    __syncthreads();
    unsigned int *__restrict__ out = a.bin_counts + b * (int64_t)bins;
    for (int i = threadIdx.x; i < bins; i += kLevelThreads) {
        const unsigned int v = cnt[i];
        if (v) atomicAdd(out + i, v);
    }
}

// ---- the host side ---------------------------------------------------------------------------------------------------------
static int64_t level_voice_pad16(int64_t v) { return (v + 15) & ~(int64_t)15; }

// The fixed launch of a push, and where the parts of the state begin.
struct LevelVoicePlan {
    int64_t stage_groups, fill_at, keys_at, bins_at, need;
};

// voice_window_plan's checks (there is no whole-voice form), then the state: the positions, the fills, the two rings.
static vnd_status level_voice_plan(int64_t slots, int64_t max_frames_per_call, int64_t window_frames, int64_t key_bytes,
                                   LevelVoicePlan *plan)
{
    LevelVoicePlan p{};
    const vnd_status st = voice_window_plan(slots, max_frames_per_call, window_frames, false, &p.stage_groups);
    if (st != VND_OK) return st;
    p.fill_at = voice_position_bytes(slots);
    p.keys_at = p.fill_at + level_voice_pad16(slots * (int64_t)sizeof(int32_t));
    p.bins_at = p.keys_at + level_voice_pad16(slots * window_frames * key_bytes);
    p.need = p.bins_at + level_voice_pad16(slots * window_frames * 2);
    *plan = p;
    return VND_OK;
}

template <class T>
static vnd_status level_voice_push_dev(vnd_ctx *ctx, void *state, int64_t state_bytes, int64_t max_frames_per_call,
                                       int64_t window_frames, const T *l, const T *r, int64_t stream_stride, int32_t frame_stride,
                                       const int32_t *counts, const int32_t *flags, int32_t ms_mode, int32_t semicircular,
                                       double radius_scale, const double *edges, int32_t bins, int32_t *valid, int64_t slots,
                                       void *stream_)
{
    using Bits = typename ScopeKind<T>::Bits;
    if (!state || !l || !r || !counts || !flags || !edges || !valid)
        return fail(VND_ERR_INVALID, "null state, chunk, counts, flags, edges or valid pointer");
    if (stream_stride < 1 || frame_stride < 1) return fail(VND_ERR_INVALID, "strides must be >= 1");
    if (bins < 1) return fail(VND_ERR_INVALID, "num_bins must be >= 1");
    vnd_status st = voice_window_scale<T>(radius_scale);
    if (st != VND_OK) return st;
    LevelVoicePlan p{};
    if ((st = level_voice_plan(slots, max_frames_per_call, window_frames, (int64_t)sizeof(Bits), &p)) != VND_OK) return st;
    if ((st = voice_state_check("level voice pool", state, state_bytes, p.need, slots)) != VND_OK) return st;
    int64_t xb = 0;
    if ((st = voice_chunk_bytes(slots, stream_stride, max_frames_per_call, frame_stride, sizeof(T), &xb)) != VND_OK) return st;
    // (a bin count above the limit is refused below; here it only must not overflow)
    const ScopeRegion outs[] = {{valid, slots * 4}, {state, p.need}};
    const ScopeRegion ins[] = {{l, xb}, {r, xb}, {edges, ((int64_t)bins + 1) * 8}, {counts, slots * 4}, {flags, slots * 4}};
    if (const int hit = scope_clash(outs, 2, ins, 5, false))
        return fail(VND_ERR_INVALID, "valid and the state must not overlap %s",
                    hit == 1 ? "the chunk, the edges, counts or flags" : "one another");
    if (bins > VND_LEVEL_MAX_BINS) return fail(VND_ERR_UNSUPPORTED, "%d bins, above %d", bins, VND_LEVEL_MAX_BINS);
    if (!ctx) return fail(VND_ERR_INVALID, "null context");
    DeviceScope on(ctx->device);
    if (!on.ok) return fail(VND_ERR_HIP, "cannot select device %d", ctx->device);
    hipStream_t stream = (hipStream_t)stream_;

    LevelVoiceArgs<T> a{};
    scope_fill_pool(a.s, l, r, max_frames_per_call, stream_stride, frame_stride, 1);
    a.s.e0 = edges; a.s.e1 = edges; a.s.bins0 = bins; a.s.bins1 = 1;
    a.s.scale = (T)radius_scale; a.s.ms = ms_mode != 0; a.s.fold = semicircular != 0;
    char *base = (char *)state;
    a.pos = (int64_t *)base; a.fill = (int32_t *)(base + p.fill_at);
    a.keys = (Bits *)(base + p.keys_at); a.bins = (unsigned short *)(base + p.bins_at);
    a.counts = counts; a.flags = flags; a.out_counts = valid;
    a.slots = slots; a.M = max_frames_per_call; a.W = window_frames;
    const size_t lds_bytes = (size_t)(bins + 1) * 8;              // at most 8200 bytes
    hipLaunchKernelGGL(level_voice_stage_kernel<T>, dim3((unsigned)p.stage_groups, (unsigned)slots), dim3(kScopeVoiceThreads),
                       lds_bytes, stream, a);
    HIP_TRY(hipGetLastError());
    launch_voice_advance(a, slots, stream);
    HIP_TRY(hipGetLastError());
    return VND_OK;
}

template <class T>
static vnd_status level_voice_levels_dev(vnd_ctx *ctx, const void *state, int64_t state_bytes, int64_t max_frames_per_call,
                                         int64_t window_frames, int32_t bins, const double *percentiles, int32_t num_p, T *levels,
                                         uint32_t *bin_counts, void *work, int64_t work_bytes, int64_t slots, void *stream_)
{
    using Bits = typename ScopeKind<T>::Bits;
    if (!state || !percentiles || !levels || !bin_counts)
        return fail(VND_ERR_INVALID, "null state, percentiles, levels or bin_counts pointer");
    if (bins < 1 || num_p < 1) return fail(VND_ERR_INVALID, "num_bins and num_percentiles must be >= 1");
    for (int32_t p = 0; p < num_p; ++p)
        if (!(percentiles[p] >= 0.0 && percentiles[p] <= 100.0))
            return fail(VND_ERR_INVALID, "percentile %g is not in [0, 100]", percentiles[p]);
    if (!work) return fail(VND_ERR_INVALID, "null work pointer: the select needs vnd_polar_level_voice_stream_work_bytes of memory");
    if ((uintptr_t)work % 8 != 0) return fail(VND_ERR_INVALID, "the work memory is not 8-byte aligned");
    LevelVoicePlan p{};
    vnd_status st = level_voice_plan(slots, max_frames_per_call, window_frames, (int64_t)sizeof(Bits), &p);
    if (st != VND_OK) return st;
    if ((st = voice_state_check("level voice pool", state, state_bytes, p.need, slots)) != VND_OK) return st;
    // What the work memory must hold, and what overlaps, is defined for a supported shape only (as in vnd_level.hpp).
    if ((st = level_check_shape(slots, window_frames, bins, num_p)) != VND_OK) return st;
    const LevelLayout w = level_select_layout(0, slots, window_frames, bins, num_p, (int64_t)sizeof(Bits));
    if (work_bytes < w.total)
        return fail(VND_ERR_INVALID, "work of %lld bytes, the call needs %lld", (long long)work_bytes, (long long)w.total);
    const int64_t cells_all = slots * bins * num_p;
    const ScopeRegion regions[] = {{levels, cells_all * (int64_t)sizeof(T)}, {bin_counts, slots * bins * 4}, {work, w.total},
                                   {state, p.need}};
    if (scope_clash(regions, 4, nullptr, 0, true))
        return fail(VND_ERR_INVALID, "levels, bin_counts, work and the state must not overlap one another");
    if (!ctx) return fail(VND_ERR_INVALID, "null context");
    DeviceScope on(ctx->device);
    if (!on.ok) return fail(VND_ERR_HIP, "cannot select device %d", ctx->device);
    hipStream_t stream = (hipStream_t)stream_;

    char *ring = (char *)const_cast<void *>(state);               // (read only: LevelArgs is the one-shot's, which stages)
    LevelArgs<T> a{};
    a.s.n_frames = window_frames; a.s.step = 1; a.s.n_each = (const int32_t *)(ring + p.fill_at);
    a.s.bins0 = bins; a.s.bins1 = 1; a.s.span = VND_LEVEL_SPAN_FRAMES;
    a.keys = (Bits *)(ring + p.keys_at); a.bins = (unsigned short *)(ring + p.bins_at); a.bin_counts = bin_counts;
    a.levels = levels;
    level_fill_select(a, (char *)work, w, slots, bins, percentiles, num_p);
    LevelSelectLds lds{};
    if ((st = level_select_allow<T>(ctx, bins, num_p, w.digit_bits, &lds)) != VND_OK) return st;

    HIP_TRY(hipMemsetAsync(bin_counts, 0, (size_t)slots * bins * 4, stream));
    const dim3 frames_grid((unsigned)((window_frames + VND_LEVEL_SPAN_FRAMES - 1) / VND_LEVEL_SPAN_FRAMES), (unsigned)slots);
    hipLaunchKernelGGL(level_voice_count_kernel<T>, frames_grid, dim3(kLevelThreads), (size_t)bins * 4, stream, a);
    return level_run_select(a, w, lds, slots, stream);
}

extern "C" {

vnd_status vnd_polar_level_voice_stream_state_bytes(int64_t slots, int64_t max_frames_per_call, int64_t window_frames,
                                                    int32_t is_float64, int64_t *bytes)
{
    if (!bytes) return fail(VND_ERR_INVALID, "null bytes");
    *bytes = 0;
    LevelVoicePlan p{};
    const vnd_status st = level_voice_plan(slots, max_frames_per_call, window_frames, is_float64 ? 8 : 4, &p);
    if (st != VND_OK) return st;
    *bytes = p.need;
    return VND_OK;
}

vnd_status vnd_polar_level_voice_stream_reset_dev(vnd_ctx *ctx, void *state, int64_t state_bytes, int64_t slots,
                                                  int64_t max_frames_per_call, int64_t window_frames, int32_t is_float64,
                                                  void *stream_)
{
    LevelVoicePlan p{};
    vnd_status st = level_voice_plan(slots, max_frames_per_call, window_frames, is_float64 ? 8 : 4, &p);
    if (st != VND_OK) return st;
    if ((st = voice_state_check("level voice pool", state, state_bytes, p.need, slots)) != VND_OK) return st;
    if (!ctx) return fail(VND_ERR_INVALID, "null context");
    DeviceScope on(ctx->device);
    if (!on.ok) return fail(VND_ERR_HIP, "cannot select device %d", ctx->device);
    HIP_TRY(hipMemsetAsync(state, 0, (size_t)p.keys_at, (hipStream_t)stream_));        // the positions and the fills
    return VND_OK;
}

vnd_status vnd_polar_level_voice_stream_push_f32_dev(vnd_ctx *ctx, void *state, int64_t state_bytes, int64_t max_frames_per_call,
                                                     int64_t window_frames, const float *l, const float *r, int64_t stream_stride,
                                                     int32_t frame_stride, const int32_t *counts, const int32_t *flags,
                                                     int32_t ms_mode, int32_t semicircular, double radius_scale,
                                                     const double *angle_edges, int32_t num_bins, int32_t *valid, int64_t slots,
                                                     void *stream)
{
    return level_voice_push_dev<float>(ctx, state, state_bytes, max_frames_per_call, window_frames, l, r, stream_stride,
                                       frame_stride, counts, flags, ms_mode, semicircular, radius_scale, angle_edges, num_bins,
                                       valid, slots, stream);
}

vnd_status vnd_polar_level_voice_stream_push_f64_dev(vnd_ctx *ctx, void *state, int64_t state_bytes, int64_t max_frames_per_call,
                                                     int64_t window_frames, const double *l, const double *r,
                                                     int64_t stream_stride, int32_t frame_stride, const int32_t *counts,
                                                     const int32_t *flags, int32_t ms_mode, int32_t semicircular,
                                                     double radius_scale, const double *angle_edges, int32_t num_bins,
                                                     int32_t *valid, int64_t slots, void *stream)
{
    return level_voice_push_dev<double>(ctx, state, state_bytes, max_frames_per_call, window_frames, l, r, stream_stride,
                                        frame_stride, counts, flags, ms_mode, semicircular, radius_scale, angle_edges, num_bins,
                                        valid, slots, stream);
}

vnd_status vnd_polar_level_voice_stream_work_bytes(int64_t slots, int64_t window_frames, int32_t num_bins, int32_t num_percentiles,
                                                   int32_t is_float64, int64_t *bytes)
{
    if (!bytes) return fail(VND_ERR_INVALID, "null bytes");
    *bytes = 0;
    if (slots < 1 || window_frames < 1 || num_bins < 1 || num_percentiles < 1)
        return fail(VND_ERR_INVALID, "slots, window_frames, num_bins and num_percentiles must be >= 1");
    if (window_frames > INT32_MAX) return fail(VND_ERR_UNSUPPORTED, "window_frames %lld above INT32_MAX", (long long)window_frames);
    const vnd_status st = level_check_shape(slots, window_frames, num_bins, num_percentiles);
    if (st != VND_OK) return st;
    *bytes = level_select_layout(0, slots, window_frames, num_bins, num_percentiles, is_float64 ? 8 : 4).total;
    return VND_OK;
}

vnd_status vnd_polar_level_voice_stream_levels_f32_dev(vnd_ctx *ctx, const void *state, int64_t state_bytes,
                                                       int64_t max_frames_per_call, int64_t window_frames, int32_t num_bins,
                                                       const double *percentiles, int32_t num_percentiles, float *levels,
                                                       uint32_t *bin_counts, void *work, int64_t work_bytes, int64_t slots,
                                                       void *stream)
{
    return level_voice_levels_dev<float>(ctx, state, state_bytes, max_frames_per_call, window_frames, num_bins, percentiles,
                                         num_percentiles, levels, bin_counts, work, work_bytes, slots, stream);
}

vnd_status vnd_polar_level_voice_stream_levels_f64_dev(vnd_ctx *ctx, const void *state, int64_t state_bytes,
                                                       int64_t max_frames_per_call, int64_t window_frames, int32_t num_bins,
                                                       const double *percentiles, int32_t num_percentiles, double *levels,
                                                       uint32_t *bin_counts, void *work, int64_t work_bytes, int64_t slots,
                                                       void *stream)
{
    return level_voice_levels_dev<double>(ctx, state, state_bytes, max_frames_per_call, window_frames, num_bins, percentiles,
                                          num_percentiles, levels, bin_counts, work, work_bytes, slots, stream);
}

}  // extern "C"

// vnd_scope_voice_stream.hpp - the vectorscope of a voice pool (include/vnd_scope_voice_stream.h): the polar and Lissajous
// count grids of vnd_scope.hpp with the signal arriving block by block, the position per slot in the device state and a count
// and start / end flags per slot and call - whole-voice, or over the last W frames of each voice (a sliding window).
// (one translation unit: included by vnd_amd.hip after vnd_scope.hpp and vnd_voice_window.hpp)
//
// The cell of a frame is formed by scope_hist_kernel's own functions - ScopeKind<T>::sample / degrees, scope_radius, scope_bin
// on edges staged in LDS - so a grid row is the one-shot entry's, cell for cell.  What is new is the life cycle of a row and
// the window.  Counts are integers: the frame that leaves the window takes its count out of the cell it was put in, which
// the ring remembers, and the row is exact.
//
// Three launches on the caller's stream, with grids fixed by (slots, M, cells):
//   scope_voice_clear_kernel, grid (ceil(4 cells / 16 KiB), slots): a workgroup leaves at once unless its slot answers 1 from
//     position 0 - a START, or a voice that begins at 0 after an END or a reset; otherwise it zeroes its 16 KiB of the row with
//     16-byte stores (4-byte stores for a head and a tail that are not 16-byte aligned).
//   scope_voice_bin_kernel, the walk of vnd_voice_window.hpp: idle slots, bad slots and workgroups past n leave before the
//     edges are staged.  Frame j of the chunk is the voice's frame g = p + j.  With W > 0 the lane reads ring[g mod W] when
//     g >= W - the cell of frame g - W - and takes one count out of it when it lies in [0, cells); then it adds one count
//     to the new cell, if the frame has one, and stores the new cell or -1 in ring[g mod W].  Global integer atomics: the
//     direct route of vnd_scope.hpp (DESIGN.md 3.25 says why not the LDS-private one).
//   voice_advance_kernel<ScopeVoiceArgs<T>> (vnd_voice_core.hpp) writes valid[b] and pos[b].
// The kernel boundaries are the ordering clear -> bin -> advance: every read of pos[b] comes before its update, and every
// count of a call lands on a cleared row (vnd_voice_core.hpp, ORDERING).
//
// Ring: the argument of vnd_voice_window.hpp, with the slot rule and the indices built from device data.  What is this pool's:
// an entry is read only for g >= W, when frame g - W of THIS voice wrote it, so the ring is never cleared; a new cell is
// k0 * bins1 + k1 with both bins from scope_bin, in [0, cells); a cell READ from the ring is used only when it lies in
// [0, cells), whatever the state holds.
#pragma once
#include "../../include/vnd_scope_voice_stream.h"

constexpr int64_t kScopeVoiceClearBytes = 16384;      // bytes of one row per workgroup of the clear kernel

template <class T>
struct ScopeVoiceArgs {
    // The chunk fields of ScopeArgs<T> in this struct's own text, and the packed load below in the kernel's: with ScopeArgs<T>
    // embedded, as LevelVoiceArgs<T> has it, the whole-voice form measured 0.2 - 1.6 % slower at 256 slots x 4800 frames
    // (profiles/voice_window_core_rates.json); registers, LDS and occupancy were the same either way.
    const T *__restrict__ l;            // the chunk: frame t of slot b at b * stream_stride + t * frame_stride
    const T *__restrict__ r;
    int64_t stream_stride, frame_stride;
    const double *__restrict__ e0;      // bins0 + 1 edges of coordinate 0
    const double *__restrict__ e1;
    int32_t bins0, bins1;
    unsigned int *__restrict__ grid;    // [slots][bins0][bins1]
    int32_t *__restrict__ ring;         // [slots][W]: the cell of frame g at g mod W, -1 for a dropped frame; null with W = 0
    int64_t *__restrict__ pos;          // [slots]
    const int32_t *__restrict__ counts;
    const int32_t *__restrict__ flags;
    int32_t *__restrict__ out_counts;   // valid [slots]
    int64_t slots, M, W;
    T scale;                            // polar: radius / scale
    int32_t ms, fold, packed;           // packed: r == l + 1 on even strides, 2-element aligned - one load a frame
    __device__ vnd::VoiceAnswer advance(int64_t b) const
    {
        const ScopeVoiceSpan v = scope_voice_span(pos[b], counts[b], flags[b], M);
        return {v.valid, v.valid == 1, v.next};
    }
};

// grid = (ceil(4 cells / kScopeVoiceClearBytes), slots)
template <class T>
__global__ __launch_bounds__(kScopeVoiceThreads) void scope_voice_clear_kernel(const ScopeVoiceArgs<T> a)
{
    const int64_t b = blockIdx.y;
    const ScopeVoiceSpan s = scope_voice_view(a.pos, a.counts, a.flags, a.M, b);
    if (s.valid != 1 || !s.clear) return;                         // (workgroup-uniform)
    constexpr int64_t kPer = kScopeVoiceClearBytes / 4;
    const int64_t cells = (int64_t)a.bins0 * a.bins1;
    const int64_t lo = (int64_t)blockIdx.x * kPer, hi = lo + kPer < cells ? lo + kPer : cells;    // lo < cells by the grid
    unsigned int *row = a.grid + b * cells;
    // [lo, hi) = a head up to the first 16-byte boundary, whole uint4s, a tail
    int64_t head = (int64_t)((16 - ((uintptr_t)(row + lo) & 15)) & 15) / 4;
    if (head > hi - lo) head = hi - lo;
    const int64_t quads = (hi - lo - head) / 4, tail0 = lo + head + 4 * quads;
    if ((int64_t)threadIdx.x < head) row[lo + threadIdx.x] = 0u;
    uint4 *body = (uint4 *)(row + lo + head);
    for (int64_t i = threadIdx.x; i < quads; i += kScopeVoiceThreads) body[i] = make_uint4(0u, 0u, 0u, 0u);
    if ((int64_t)threadIdx.x < hi - tail0) row[tail0 + threadIdx.x] = 0u;
}

// grid = (ceil(M / kScopeVoiceSpan), slots); dynamic LDS: the edges
template <class T, bool POLAR>
__global__ __launch_bounds__(kScopeVoiceThreads) void scope_voice_bin_kernel(const ScopeVoiceArgs<T> a)
{
    using K = ScopeKind<T>;
    extern __shared__ __attribute__((aligned(16))) double scope_voice_lds[];
    const int64_t b = blockIdx.y;
    VoiceWindowWalk w;
    if (!w.open(a.pos, a.counts, a.flags, a.M, b, blockIdx.x)) return;
    const int bins0 = a.bins0, bins1 = a.bins1;
    double *e0 = scope_voice_lds, *e1 = scope_voice_lds + (bins0 + 1);
    for (int i = threadIdx.x; i <= bins0; i += kScopeVoiceThreads) e0[i] = a.e0[i];
    for (int i = threadIdx.x; i <= bins1; i += kScopeVoiceThreads) e1[i] = a.e1[i];
    __syncthreads();
    const double inv0 = (double)bins0 / (e0[bins0] - e0[0]), inv1 = (double)bins1 / (e1[bins1] - e1[0]);
    const int cells = bins0 * bins1;
    const T *__restrict__ pl = a.l + b * a.stream_stride;
    const T *__restrict__ pr = a.r + b * a.stream_stride;
    unsigned int *__restrict__ out = a.grid + b * (int64_t)cells;
    int32_t *__restrict__ ring = a.W > 0 ? a.ring + b * a.W : nullptr;
    if (ring) w.enter(a.W);
    for (int64_t j = w.j0 + threadIdx.x; j < w.j1; j += kScopeVoiceThreads) {
        const int64_t i = j * a.frame_stride;
        T l, r;
        if (a.packed) {
            const typename K::Pair v = *(const typename K::Pair *)(pl + i);
            l = v.x; r = v.y;
        } else {
            l = pl[i]; r = pr[i];
        }
        double v0, v1;
        if (POLAR) {
            T th, rad;
            K::sample(l, r, a.ms != 0, a.fold != 0, th, rad);
            v0 = (double)K::degrees(th);
            v1 = (double)scope_radius(rad, a.scale);
        } else {
            v0 = (double)l;
            v1 = (double)r;
        }
        int c = -1;
        const int k0 = scope_bin(e0, bins0, inv0, v0);
        if (k0 >= 0) {
            const int k1 = scope_bin(e1, bins1, inv1, v1);
            if (k1 >= 0) c = k0 * bins1 + k1;
        }
        if (ring) {
            const int64_t slot = w.entry(j);
            if (w.s.p + j >= a.W) {                               // frame g - W of this voice leaves the window
                const int32_t old = ring[slot];
                if (old >= 0 && old < cells) atomicSub(out + old, 1u);
            }
            ring[slot] = c;
        }
        if (c >= 0) atomicAdd(out + c, 1u);
    }
}

// ---- the host side ---------------------------------------------------------------------------------------------------------
// The fixed launch of a pool, and where the ring begins.
struct ScopeVoicePlan {
    int64_t bin_groups, ring_at, need;
};

// voice_window_plan's checks (window_frames = 0: whole-voice), then the state: the positions, the ring.
static vnd_status scope_voice_plan(int64_t slots, int64_t max_frames_per_call, int64_t window_frames, ScopeVoicePlan *plan)
{
    ScopeVoicePlan p{};
    const vnd_status st = voice_window_plan(slots, max_frames_per_call, window_frames, true, &p.bin_groups);
    if (st != VND_OK) return st;
    p.ring_at = voice_position_bytes(slots);
    p.need = p.ring_at + ((slots * window_frames * (int64_t)sizeof(int32_t) + 15) & ~(int64_t)15);
    *plan = p;
    return VND_OK;
}

template <class T, bool POLAR>
static vnd_status scope_voice_stream_dev(vnd_ctx *ctx, void *state, int64_t state_bytes, int64_t max_frames_per_call,
                                         int64_t window_frames, const T *l, const T *r, int64_t stream_stride, int32_t frame_stride,
                                         const int32_t *counts, const int32_t *flags, int32_t ms_mode, int32_t semicircular,
                                         double radius_scale, const double *e0, int32_t bins0, const double *e1, int32_t bins1,
                                         uint32_t *grid, int32_t *valid, int64_t slots, void *stream_)
{
    if (!state || !l || !r || !counts || !flags || !e0 || !e1 || !grid || !valid)
        return fail(VND_ERR_INVALID, "null state, chunk, counts, flags, edges, grid or valid pointer");
    if (stream_stride < 1 || frame_stride < 1) return fail(VND_ERR_INVALID, "strides must be >= 1");
    if (bins0 < 1 || bins1 < 1) return fail(VND_ERR_INVALID, "bin counts must be >= 1");
    vnd_status st = VND_OK;
    if (POLAR && (st = voice_window_scale<T>(radius_scale)) != VND_OK) return st;
    ScopeVoicePlan p{};
    if ((st = scope_voice_plan(slots, max_frames_per_call, window_frames, &p)) != VND_OK) return st;
    if ((st = voice_state_check("scope voice pool", state, state_bytes, p.need, slots)) != VND_OK) return st;
    if ((uintptr_t)grid % 4 != 0) return fail(VND_ERR_INVALID, "the grid is not 4-byte aligned");
    int64_t xb = 0;
    if ((st = voice_chunk_bytes(slots, stream_stride, max_frames_per_call, frame_stride, sizeof(T), &xb)) != VND_OK) return st;
    const bool bins_ok = bins0 <= VND_SCOPE_MAX_BINS && bins1 <= VND_SCOPE_MAX_BINS;
    // (bin counts above the limit are refused below; here they only must not overflow)
    const int64_t cells = (int64_t)bins0 * bins1;
    if (slots > INT64_MAX / 16 / cells) return fail(VND_ERR_INVALID, "buffer extents overflow");
    const ScopeRegion outs[] = {{grid, slots * cells * 4}, {valid, slots * 4}, {state, p.need}};
    const ScopeRegion ins[] = {{l, xb}, {r, xb}, {e0, ((int64_t)bins0 + 1) * 8}, {e1, ((int64_t)bins1 + 1) * 8}, {counts, slots * 4},
                               {flags, slots * 4}};
    if (const int hit = scope_clash(outs, 3, ins, 6, true))
        return fail(VND_ERR_INVALID, "grid, valid and the state must not overlap %s",
                    hit == 1 ? "the chunk, the edges, counts or flags" : "one another");
    if (!bins_ok) return fail(VND_ERR_UNSUPPORTED, "%d x %d bins, above %d an axis", bins0, bins1, VND_SCOPE_MAX_BINS);
    const int64_t clear_groups = (cells * 4 + kScopeVoiceClearBytes - 1) / kScopeVoiceClearBytes;
    if (clear_groups * slots > kScopeMaxGroups)
        return fail(VND_ERR_UNSUPPORTED, "%lld workgroups in one launch, above 2^23: split the pool", (long long)(clear_groups * slots));
    if (!ctx) return fail(VND_ERR_INVALID, "null context");
    DeviceScope on(ctx->device);
    if (!on.ok) return fail(VND_ERR_HIP, "cannot select device %d", ctx->device);
    hipStream_t stream = (hipStream_t)stream_;

    ScopeVoiceArgs<T> a{};
    a.l = l; a.r = r; a.stream_stride = stream_stride; a.frame_stride = frame_stride;
    a.packed = r == l + 1 && stream_stride % 2 == 0 && frame_stride % 2 == 0 && (uintptr_t)l % (2 * sizeof(T)) == 0;
    a.e0 = e0; a.e1 = e1; a.bins0 = bins0; a.bins1 = bins1; a.grid = grid;
    a.ring = window_frames > 0 ? (int32_t *)((char *)state + p.ring_at) : nullptr;
    a.pos = (int64_t *)state; a.counts = counts; a.flags = flags; a.out_counts = valid;
    a.slots = slots; a.M = max_frames_per_call; a.W = window_frames;
    a.scale = POLAR ? (T)radius_scale : (T)0; a.ms = ms_mode != 0; a.fold = semicircular != 0;
    const size_t lds_bytes = (size_t)scope_edge_bytes(bins0, bins1);
    const void *kernel = (const void *)scope_voice_bin_kernel<T, POLAR>;
    if ((st = allow_lds(ctx, kernel, lds_bytes)) != VND_OK) return st;
    hipLaunchKernelGGL(scope_voice_clear_kernel<T>, dim3((unsigned)clear_groups, (unsigned)slots), dim3(kScopeVoiceThreads), 0, stream, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL((scope_voice_bin_kernel<T, POLAR>), dim3((unsigned)p.bin_groups, (unsigned)slots), dim3(kScopeVoiceThreads),
                       lds_bytes, stream, a);
    HIP_TRY(hipGetLastError());
    launch_voice_advance(a, slots, stream);
    HIP_TRY(hipGetLastError());
    return VND_OK;
}

extern "C" {

vnd_status vnd_scope_voice_stream_state_bytes(int64_t slots, int64_t max_frames_per_call, int64_t window_frames, int64_t *bytes)
{
    if (!bytes) return fail(VND_ERR_INVALID, "null bytes");
    *bytes = 0;
    ScopeVoicePlan p{};
    const vnd_status st = scope_voice_plan(slots, max_frames_per_call, window_frames, &p);
    if (st != VND_OK) return st;
    *bytes = p.need;
    return VND_OK;
}

vnd_status vnd_scope_voice_stream_reset_dev(vnd_ctx *ctx, void *state, int64_t state_bytes, int64_t slots, int64_t max_frames_per_call,
                                            int64_t window_frames, void *stream_)
{
    ScopeVoicePlan p{};
    vnd_status st = scope_voice_plan(slots, max_frames_per_call, window_frames, &p);
    if (st != VND_OK) return st;
    if ((st = voice_state_check("scope voice pool", state, state_bytes, p.need, slots)) != VND_OK) return st;
    if (!ctx) return fail(VND_ERR_INVALID, "null context");
    return voice_reset_positions(ctx, state, slots, stream_);
}

vnd_status vnd_polar_hist_voice_stream_f32_dev(vnd_ctx *ctx, void *state, int64_t state_bytes, int64_t max_frames_per_call,
                                               int64_t window_frames, const float *l, const float *r, int64_t stream_stride,
                                               int32_t frame_stride, const int32_t *counts, const int32_t *flags, int32_t ms_mode,
                                               int32_t semicircular, double radius_scale, const double *angle_edges,
                                               int32_t num_angle_bins, const double *radius_edges, int32_t num_radius_bins,
                                               uint32_t *grid, int32_t *valid, int64_t slots, void *stream)
{
    return scope_voice_stream_dev<float, true>(ctx, state, state_bytes, max_frames_per_call, window_frames, l, r, stream_stride,
                                               frame_stride, counts, flags, ms_mode, semicircular, radius_scale, angle_edges,
                                               num_angle_bins, radius_edges, num_radius_bins, grid, valid, slots, stream);
}

vnd_status vnd_polar_hist_voice_stream_f64_dev(vnd_ctx *ctx, void *state, int64_t state_bytes, int64_t max_frames_per_call,
                                               int64_t window_frames, const double *l, const double *r, int64_t stream_stride,
                                               int32_t frame_stride, const int32_t *counts, const int32_t *flags, int32_t ms_mode,
                                               int32_t semicircular, double radius_scale, const double *angle_edges,
                                               int32_t num_angle_bins, const double *radius_edges, int32_t num_radius_bins,
                                               uint32_t *grid, int32_t *valid, int64_t slots, void *stream)
{
    return scope_voice_stream_dev<double, true>(ctx, state, state_bytes, max_frames_per_call, window_frames, l, r, stream_stride,
                                                frame_stride, counts, flags, ms_mode, semicircular, radius_scale, angle_edges,
                                                num_angle_bins, radius_edges, num_radius_bins, grid, valid, slots, stream);
}

vnd_status vnd_lissajous_hist_voice_stream_f32_dev(vnd_ctx *ctx, void *state, int64_t state_bytes, int64_t max_frames_per_call,
                                                   int64_t window_frames, const float *l, const float *r, int64_t stream_stride,
                                                   int32_t frame_stride, const int32_t *counts, const int32_t *flags,
                                                   const double *x_edges, int32_t x_bins, const double *y_edges, int32_t y_bins,
                                                   uint32_t *grid, int32_t *valid, int64_t slots, void *stream)
{
    return scope_voice_stream_dev<float, false>(ctx, state, state_bytes, max_frames_per_call, window_frames, l, r, stream_stride,
                                                frame_stride, counts, flags, 0, 0, 0.0, x_edges, x_bins, y_edges, y_bins, grid, valid,
                                                slots, stream);
}

vnd_status vnd_lissajous_hist_voice_stream_f64_dev(vnd_ctx *ctx, void *state, int64_t state_bytes, int64_t max_frames_per_call,
                                                   int64_t window_frames, const double *l, const double *r, int64_t stream_stride,
                                                   int32_t frame_stride, const int32_t *counts, const int32_t *flags,
                                                   const double *x_edges, int32_t x_bins, const double *y_edges, int32_t y_bins,
                                                   uint32_t *grid, int32_t *valid, int64_t slots, void *stream)
{
    return scope_voice_stream_dev<double, false>(ctx, state, state_bytes, max_frames_per_call, window_frames, l, r, stream_stride,
                                                 frame_stride, counts, flags, 0, 0, 0.0, x_edges, x_bins, y_edges, y_bins, grid, valid,
                                                 slots, stream);
}

}  // extern "C"

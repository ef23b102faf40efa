/* vnd_level.h - the polar level envelope on the device, exported by libvnd_amd.so: for every signal of a pool, every angular
 * slice and every requested percentile, np.percentile of the radii whose angle falls in the slice - the first two steps of
 * utils/plot.py _build_pseudo_hull (:688-699), which plot_polar_level draws its outline (p = 95) and its median overlay
 * (p = 50) from.  It is bin_percentile_radii of _build_pseudo_hull(..., smoothing_sigma=0, use_convex_hull=False); the
 * smoothing, the convex hull and the drawing work on num_bins numbers a signal and are not here.
 *
 * Same conventions as vnd_scope.h (plain C99, vnd_status, vnd_last_error, "*_dev" = device pointers and a hipStream_t passed
 * as void*).  The entry enqueues on hip_stream only: it allocates nothing, reads no device memory from the host, synchronises
 * nothing, is graph-capturable and thread-safe.  Every argument is checked before anything is enqueued, with nothing
 * written: first the arguments (VND_ERR_INVALID, then VND_ERR_UNSUPPORTED), last the context (a null ctx is VND_ERR_INVALID
 * "null context").
 *
 * ---- the sample of a frame ----------------------------------------------------------------------------------------------
 * vnd_scope.h's, from the same device function: pool layout, ms_mode, semicircular, the degrees (one multiply by
 * 57.2957763671875f; float64: 180.0 / pi) and the radius coordinate - radius_scale <= 0: the radius divided by the signal's
 * own maximum plus eps, by vnd_scope.h's first pass; radius_scale > 0: divided by sample_type(radius_scale).  n_each_dev: null,
 * or int32 [batch] in device memory: signal b is its first n_each[b] frames; a value outside [0, n_frames] contributes no
 * frame, and nothing is indexed with it.
 *
 * ---- the bin of a frame -------------------------------------------------------------------------------------------------
 * The reference's mask, not np.histogramdd's rule: the degrees are widened to float64 and compared with num_bins + 1 ascending
 * float64 edges in device memory (the caller's np.linspace(-90, 90, num_bins + 1)); bin k holds edges[k] <= deg < edges[k + 1],
 * the last bin included: a frame whose angle equals the last edge (an anti-phase frame R = -L, L > 0: exactly 90.0 degrees)
 * belongs to no bin, as does a NaN angle or one outside the edges.  -90.0 lands in bin 0.  Non-finite radii are outside the
 * contract, but no index leaves its array whatever the frames hold.
 *
 * ---- the percentile of a bin --------------------------------------------------------------------------------------------
 * NumPy 2's np.percentile(radii_of_bin, p), method 'linear', on an array of the sample type T, bit for bit:
 *     q = T(p) / T(100);  v = T(m - 1) * q          m frames in the bin, T(m - 1) rounded to nearest
 *     v >= T(m - 1): prev = next = m - 1;   otherwise prev = floor(v), next = prev + 1
 *     g = v - T(prev);  a, b = sorted[prev], sorted[next];  d = b - a
 *     result = g >= 0.5 ? b - d * (1 - g) : a + d * g              every operation rounded on its own in T, nothing fused
 * An empty bin gives T(0).  The selection is exact: sorted[prev] and sorted[next] are order statistics of the bit patterns of
 * the radii (non-negative, so they order as unsigned integers), found by a most-significant-digit-first radix select whose
 * number of passes is fixed by the key width, never by the data; counts are integers added with integer atomics.  The result
 * does not depend on arrival order, block scheduling or run, for any distribution of the data.
 *
 * ---- outputs ------------------------------------------------------------------------------------------------------------
 * levels_dev: [batch][num_percentiles][num_bins] of the sample type.  bin_counts_dev: uint32 [batch][num_bins], the frames
 * of every bin.  Both are fully written by every successful call.  There is no `accumulate`: percentiles of blocks do not
 * add up to the percentile of the whole.
 *
 * ---- work ---------------------------------------------------------------------------------------------------------------
 * work_dev: caller-owned, 8-byte aligned, at least vnd_polar_level_work_bytes(...) bytes.  It holds the per-signal maximum,
 * the staged key (the radius's bit pattern) and bin (uint16) of every frame, and the select's state and digit histograms.
 * The entry clears what it needs cleared on hip_stream itself: what the memory held does not matter.
 *
 * ---- refusals -----------------------------------------------------------------------------------------------------------
 * VND_ERR_INVALID: a null pointer (n_each_dev may be null); batch, n_frames, a stride, num_bins or num_percentiles below 1; a
 * percentile outside [0, 100] or NaN; a radius_scale that is NaN, or positive with a sample-type value that is zero or
 * infinite; work_bytes below the query's answer or work_dev not 8-byte aligned; outputs (levels, bin_counts, work) overlapping
 * one another or any input (frames, edges, n_each); extents that overflow.
 * VND_ERR_UNSUPPORTED: n_frames above 2^32 - 1; batch above VND_MAX_STREAMS; num_bins above VND_LEVEL_MAX_BINS;
 * num_percentiles above VND_LEVEL_MAX_PERCENTILES; more than 2^23 workgroups in a launch (batch * ceil(n_frames /
 * VND_LEVEL_SPAN_FRAMES)).  What the work memory must hold, and which buffers overlap, is defined for a supported shape only: of
 * the VND_ERR_INVALID checks, work_bytes and the overlaps come after the VND_ERR_UNSUPPORTED ones.                         */
#ifndef VND_LEVEL_H
#define VND_LEVEL_H

#include "vnd_scope.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VND_LEVEL_MAX_PERCENTILES 4
#define VND_LEVEL_MAX_BINS 1024            /* the select's digit counters and prefixes of one signal stay in LDS */
#define VND_LEVEL_SPAN_FRAMES 32768        /* frames of one signal per workgroup, every per-frame kernel */

/* Bytes of work memory for a call of this shape.  No context. */
vnd_status vnd_polar_level_work_bytes(int64_t batch, int64_t n_frames, int32_t num_bins, int32_t num_percentiles,
                                      int32_t is_float64, int64_t *bytes);

/* percentiles: num_percentiles values in HOST memory, read at the call. */
vnd_status vnd_polar_level_f32_dev(vnd_ctx *ctx, const float *l_dev, const float *r_dev, int64_t batch, int64_t n_frames,
                                   int64_t stream_stride, int32_t frame_stride, int32_t ms_mode, int32_t semicircular,
                                   double radius_scale, const double *angle_edges_dev, int32_t num_bins,
                                   const double *percentiles, int32_t num_percentiles, const int32_t *n_each_dev,
                                   float *levels_dev, uint32_t *bin_counts_dev, void *work_dev, int64_t work_bytes,
                                   void *hip_stream);
vnd_status vnd_polar_level_f64_dev(vnd_ctx *ctx, const double *l_dev, const double *r_dev, int64_t batch, int64_t n_frames,
                                   int64_t stream_stride, int32_t frame_stride, int32_t ms_mode, int32_t semicircular,
                                   double radius_scale, const double *angle_edges_dev, int32_t num_bins,
                                   const double *percentiles, int32_t num_percentiles, const int32_t *n_each_dev,
                                   double *levels_dev, uint32_t *bin_counts_dev, void *work_dev, int64_t work_bytes,
                                   void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* VND_LEVEL_H */

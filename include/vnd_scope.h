/* vnd_scope.h - the vectorscope's data on the device, exported by libvnd_amd.so: the polar sample of every frame of a pool
 * (utils/dsp.py:374-422 polar_coordinates, compute_weights=False) and the two count grids utils/plot.py draws from - the
 * polar density of plot_polar_sample and the L/R density of plot_lissajous(color_mode='density').  Drawing is not here.
 *
 * Same conventions as vnd_analysis.h (plain C99, vnd_status, vnd_last_error, "*_dev" = device pointers and a hipStream_t
 * passed as void*), and kept out of vnd_amd.h so that it keeps its fixed set of functions.  Every *_dev entry enqueues on
 * hip_stream only: it allocates nothing, reads no device memory from the host, synchronises nothing, is graph-capturable
 * and thread-safe.  Every argument is checked before anything is enqueued, with nothing written: first the arguments
 * (VND_ERR_INVALID, then VND_ERR_UNSUPPORTED), last the context (a null ctx is VND_ERR_INVALID "null context").
 *
 * ---- pool ---------------------------------------------------------------------------------------------------------------
 * Frame t (0 <= t < n_frames) of signal b (0 <= b < batch): L at l_dev[b * stream_stride + t * frame_stride], R at r_dev
 * likewise, in elements; the two may be columns 0 and 1 of one (batch, n_frames, 2) block (stream_stride 2 n_frames,
 * frame_stride 2).  *_f32_dev takes float32 frames, *_f64_dev float64 frames (a Haas or chain pool's output).
 *
 * ---- the polar sample of a frame ----------------------------------------------------------------------------------------
 *     theta  = atan2(l - r, l + r) with ms_mode, atan2(l, r) without           (LayoutMode.MS / LayoutMode.LR)
 *     theta  = theta + pi if theta < -pi/2, theta - pi if theta > pi/2         with semicircular only
 *     radius = sqrt(l * l + r * r)                                             every operation rounded on its own
 * in the sample type, as NumPy 2 computes them on arrays of that type: float32 pi/2 and pi are float32(pi / 2) and
 * float32(pi), atan2 is atan2f.  It is the sample of vnd_polar_moments_f32_dev.  Normalised (vnd_polar_coords_*_dev with
 * `normalize`, vnd_polar_hist_*_dev with radius_scale <= 0) the radius is divided by max_b + eps: max_b the largest radius of
 * signal b ALONE, eps = float32(1e-10) added in float32 (float64: 1e-10 in float64), the division correctly rounded - NumPy's
 * `radii /= radii.max() + EPSILON`.  The maximum is taken over the bit patterns of the radii, which are non-negative: it
 * is exact and does not depend on the order.  Non-finite frames are outside the contract of the normalised forms (NumPy's
 * max of a signal with a NaN radius is NaN); the histograms drop them (below).
 *
 * ---- work ---------------------------------------------------------------------------------------------------------------
 * The per-signal maximum is a first pass into caller-owned memory: work_dev, 8-byte aligned, of at least
 * vnd_scope_work_bytes(batch) bytes.  The entry clears it on hip_stream itself: what it held does not matter.  An entry
 * that does not normalise (normalize == 0, radius_scale > 0) takes no work memory: work_dev may be null.
 *
 * ---- binning ------------------------------------------------------------------------------------------------------------
 * np.histogramdd's rule against two device arrays of float64 edges, bins + 1 strictly ascending finite values each (the
 * caller's np.linspace: the device never reproduces its rounding).  A coordinate v is widened to float64; its bin is k with
 * edges[k] <= v < edges[k + 1]; v == edges[bins] goes to bin bins - 1; every other value - outside the range, NaN, +-inf -
 * drops the frame.  A frame counts once, in cell [k0][k1], when both coordinates have a bin.  Edges that are not ascending
 * give unspecified counts, but no index leaves the grid.
 *   polar grid:      coordinate 0 = theta in degrees: theta * (float32(180) / float32(pi)) = theta * 57.2957763671875f, one
 *                    float32 multiply, which is np.degrees on float32 (float64: theta * (180.0 / pi));
 *                    coordinate 1 = the normalised radius, or with radius_scale > 0 radius / sample_type(radius_scale),
 *                    correctly rounded.  No theta or radius is written to memory.
 *   Lissajous grid:  coordinate 0 = l, coordinate 1 = r (np.histogram2d(left, right, ...)), of the frames 0, frame_step,
 *                    2 frame_step, ... (the reference's left[::step]).
 * counts_dev: uint32 [batch][bins0][bins1], C-contiguous.  accumulate == 0: the entry clears the grid on hip_stream first.
 * accumulate != 0: the counts are added to what the grid holds (modulo 2^32).  accumulate with the per-signal maximum
 * (radius_scale <= 0) is VND_ERR_INVALID: the maximum of a later block would rescale the earlier frames.
 * n_each_dev: null, or int32 [batch] in device memory: signal b is its first n_each[b] frames (the Lissajous grid takes every
 * frame_step-th of those).  A value outside [0, n_frames] contributes no frame, and nothing is indexed with it.  It is the
 * out_counts of a voice pool or a block stream, handed on without a host read.
 * Counts are integers added with integer atomics: a grid does not depend on the order of arrival, on the route or on the
 * run, bit for bit.
 *
 * ---- routes -------------------------------------------------------------------------------------------------------------
 * LDS-private (route 1): a workgroup owns VND_SCOPE_SPAN_FRAMES consecutive (used) frames of one signal, bins them into a
 * private grid in LDS and adds its non-zero cells to counts_dev at the end.  For grids with
 * 4 bins0 bins1 + 8 (bins0 + bins1 + 2) <= VND_SCOPE_LDS_BYTES (the default 240 x 150 polar grid: 147136).
 * Direct (route 2): every frame is one atomic add to counts_dev.  Every grid the entry accepts.
 * The entry chooses by grid and frames per signal; the tuning variable VND_SCOPE_ROUTE (read at the call in
 * a VND_TUNING=1 process: 1 LDS-private where the grid fits, 2 direct, anything else the entry's choice) pins it.
 * vnd_scope_route answers which route a call of a shape takes now.
 *
 * ---- refusals -----------------------------------------------------------------------------------------------------------
 * VND_ERR_INVALID: a null pointer (n_each_dev may be null; work_dev as above); batch, n_frames, a stride, a bin count or
 * frame_step below 1; work_bytes below the query's answer or work_dev not 8-byte aligned; a radius_scale that is NaN, or
 * positive with a sample-type value that is zero or infinite; accumulate with radius_scale <= 0; outputs (counts, radii,
 * thetas, work) overlapping one another or any input (frames, edges, n_each); extents that overflow.
 * VND_ERR_UNSUPPORTED: n_frames above 2^32 - 1 (counts are uint32); batch above VND_MAX_STREAMS; a bin count above
 * VND_SCOPE_MAX_BINS (the edges of both axes are staged in LDS); more than 2^23 workgroups in the launch (batch *
 * ceil(used frames / VND_SCOPE_DIRECT_SPAN_FRAMES) on the direct route).                                                */
#ifndef VND_SCOPE_H
#define VND_SCOPE_H

#include "vnd_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VND_SCOPE_MAX_BINS 4096            /* bins per axis */
#define VND_SCOPE_LDS_BYTES 163840         /* the LDS-private route's budget: the grid and both edge arrays */
#define VND_SCOPE_SPAN_FRAMES 32768        /* frames of one signal per workgroup, LDS-private route */
#define VND_SCOPE_DIRECT_SPAN_FRAMES 4096  /* ... direct route */
#define VND_SCOPE_ROUTE_LDS 1
#define VND_SCOPE_ROUTE_DIRECT 2

/* Bytes of work memory for a pool of `batch` signals.  No context. */
vnd_status vnd_scope_work_bytes(int64_t batch, int64_t *bytes);
/* The route (VND_SCOPE_ROUTE_*) a histogram of bins0 x bins1 cells over used_frames frames per signal takes now: the
 * entry's choice, or what VND_SCOPE_ROUTE pins.  No context. */
vnd_status vnd_scope_route(int32_t bins0, int32_t bins1, int64_t used_frames, int32_t *route);

/* radii_dev, thetas_dev: [batch][n_frames] of the sample type, C-contiguous. */
vnd_status vnd_polar_coords_f32_dev(vnd_ctx *ctx, const float *l_dev, const float *r_dev, int64_t batch, int64_t n_frames,
                                    int64_t stream_stride, int32_t frame_stride, int32_t ms_mode, int32_t semicircular,
                                    int32_t normalize, float *radii_dev, float *thetas_dev, void *work_dev,
                                    int64_t work_bytes, void *hip_stream);
vnd_status vnd_polar_coords_f64_dev(vnd_ctx *ctx, const double *l_dev, const double *r_dev, int64_t batch, int64_t n_frames,
                                    int64_t stream_stride, int32_t frame_stride, int32_t ms_mode, int32_t semicircular,
                                    int32_t normalize, double *radii_dev, double *thetas_dev, void *work_dev,
                                    int64_t work_bytes, void *hip_stream);

/* counts_dev: uint32 [batch][num_angle_bins][num_radius_bins]. */
vnd_status vnd_polar_hist_f32_dev(vnd_ctx *ctx, const float *l_dev, const float *r_dev, int64_t batch, int64_t n_frames,
                                  int64_t stream_stride, int32_t frame_stride, int32_t ms_mode, int32_t semicircular,
                                  double radius_scale, const double *angle_edges_dev, int32_t num_angle_bins,
                                  const double *radius_edges_dev, int32_t num_radius_bins, const int32_t *n_each_dev,
                                  uint32_t *counts_dev, int32_t accumulate, void *work_dev, int64_t work_bytes,
                                  void *hip_stream);
vnd_status vnd_polar_hist_f64_dev(vnd_ctx *ctx, const double *l_dev, const double *r_dev, int64_t batch, int64_t n_frames,
                                  int64_t stream_stride, int32_t frame_stride, int32_t ms_mode, int32_t semicircular,
                                  double radius_scale, const double *angle_edges_dev, int32_t num_angle_bins,
                                  const double *radius_edges_dev, int32_t num_radius_bins, const int32_t *n_each_dev,
                                  uint32_t *counts_dev, int32_t accumulate, void *work_dev, int64_t work_bytes,
                                  void *hip_stream);

/* counts_dev: uint32 [batch][x_bins][y_bins]; L on the first axis. */
vnd_status vnd_lissajous_hist_f32_dev(vnd_ctx *ctx, const float *l_dev, const float *r_dev, int64_t batch, int64_t n_frames,
                                      int64_t stream_stride, int32_t frame_stride, int64_t frame_step,
                                      const double *x_edges_dev, int32_t x_bins, const double *y_edges_dev, int32_t y_bins,
                                      const int32_t *n_each_dev, uint32_t *counts_dev, int32_t accumulate, void *hip_stream);
vnd_status vnd_lissajous_hist_f64_dev(vnd_ctx *ctx, const double *l_dev, const double *r_dev, int64_t batch, int64_t n_frames,
                                      int64_t stream_stride, int32_t frame_stride, int64_t frame_step,
                                      const double *x_edges_dev, int32_t x_bins, const double *y_edges_dev, int32_t y_bins,
                                      const int32_t *n_each_dev, uint32_t *counts_dev, int32_t accumulate, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* VND_SCOPE_H */

/* vnd_scope_voice_stream.h - the vectorscope of a VOICE POOL, exported by libvnd_amd.so: the polar and Lissajous count grids
 * of vnd_scope.h for a meter whose slots are voices and whose positions live in device memory, as
 * vnd_polar_voice_stream.h is for the polar moments.  Two forms: whole-voice (window_frames = 0: after every call a slot's
 * grid is the histogram of that voice's whole signal so far) and sliding-window (window_frames = W > 0: the histogram of the
 * voice's last W frames).  Counts are integers, so the window slides exactly: the frame that leaves it takes its count out of
 * the cell it was put in.  It reads the rows and the out_counts of a decorrelating pool (vnd_voice_stream.h,
 * vnd_haas_voice_stream.h) straight from device memory.  A call is a pure function of device memory - no argument depends on
 * the call's history - so it can be captured in a graph and replayed.
 *
 * Same conventions as vnd_polar_voice_stream.h (plain C99, vnd_status, vnd_last_error, "*_dev" = device pointers and a
 * hipStream_t passed as void*), and kept out of vnd_amd.h so that it keeps its fixed set of functions.
 *
 * ---- one call, per slot b ---------------------------------------------------------------------------------------------
 * Read on the device: pos[b] from the state, counts[b] (int32, frames pushed for this slot in this call, 0..M, M =
 * max_frames_per_call) and flags[b] (int32, VND_VOICE_START and VND_VOICE_END of vnd_voice_stream.h; other bits are
 * ignored).  With cells = bins0 * bins1:
 *     p = START ? 0 : pos[b]                  START: whatever the slot held is dropped
 *     n = counts[b]
 *     if p == 0: grid[b][..] = 0              a START, or a voice that begins at 0 after an END or a reset
 *     for every frame g in [p, p + n), c(g) = its cell k0 * bins1 + k1, or -1 when the binning rule drops it:
 *         W > 0 and g >= W:  o = ring[b][g mod W];  if 0 <= o < cells: grid[b][o] -= 1         frame g - W leaves
 *         if c(g) >= 0: grid[b][c(g)] += 1
 *         W > 0:             ring[b][g mod W] = c(g)
 *     valid[b] = 1
 *     pos[b]   = END ? 0 : p + n              after the call; END leaves the grid as it is: the final picture stays
 *                                             readable until the slot's next voice
 * A slot with n = 0 and neither flag is idle: valid[b] = 0 and nothing of its row or its state is touched.  START and END in
 * one call are a whole voice in one block.
 *
 * Contract.  After every call that answers 1, grid[b] equals BYTE FOR BYTE what vnd_polar_hist_*_dev /
 * vnd_lissajous_hist_*_dev (vnd_scope.h) write with the same edges, mode and radius_scale, accumulate = 0, frame_step = 1 and
 * no n_each, for the frames [max(0, p + n - W), p + n) of the voice - [0, p + n) with W = 0 - for every schedule of counts,
 * idle calls, restarts and neighbours.  (No frames at all: a row of zeros.)  The cell of a frame is formed by the very
 * functions of those entries: the polar sample, the degrees, radius / sample_type(radius_scale) and the binning rule of
 * vnd_scope.h.  Increments and decrements are integer atomics modulo 2^32 and the true count of a cell lies in [0, W], so a
 * row does not depend on the order of arrival or on the run.  With W = 0 the counts are modulo 2^32, as for `accumulate`.
 * Only radius_scale > 0 is accepted: a per-voice maximum cannot stream (a later block's maximum would rescale the earlier
 * frames), as for `accumulate` in vnd_scope.h.
 *
 * Bad per-slot values (the other slots are unaffected): counts[b] outside [0, M], or - without START - a stored position
 * outside [0, 2^60] (a state that was never reset): valid[b] = -1; the grid row, the ring and the position of the slot are
 * untouched and nothing is indexed with the bad value.  It is the rule of vnd_voice_stream.h, so a -1 from a decorrelating
 * pool, handed on as a count, passes through the meter as -1.
 *
 * ---- chunk ------------------------------------------------------------------------------------------------------------
 * Frame t (0 <= t < counts[b]) of slot b: L at l_dev[b * stream_stride + t * frame_stride], R at r_dev likewise, in
 * elements (l_dev and r_dev may be channels 0 and 1 of one (slots, M, 2) block: stream_stride 2 M, frame_stride 2).  Only
 * the first counts[b] frames of row b are read.  *_f32_dev takes float32, *_f64_dev float64.
 *
 * ---- grid -------------------------------------------------------------------------------------------------------------
 * grid_dev: uint32 [slots][bins0][bins1], C-contiguous, 4-byte aligned, CALLER-OWNED memory that BELONGS TO THE POOL BETWEEN
 * CALLS: it is as much the pool's state as state_dev is.  The caller hands the same memory to every call and does not write
 * it in between (reading it, on the call's stream or after it, is what it is for).  A row is first written when its slot
 * first answers 1 - and cleared then, since the position is 0 - so the memory needs no initialisation.
 * Edges: float64, bins + 1 strictly ascending finite values an axis, in device memory, the same for every call of a pool
 * (the ring holds cells of THIS grid).
 *
 * ---- state ------------------------------------------------------------------------------------------------------------
 * `state_bytes` at least what vnd_scope_voice_stream_state_bytes returns, state_dev 16-byte aligned.  In this order:
 *     positions  int64 [slots], padded to a multiple of 16 bytes
 *     ring       int32 [slots][W], padded to a multiple of 16 bytes; absent with W = 0.  Entry g mod W holds the cell that
 *                the voice's absolute frame g was counted in, or -1 if the binning rule dropped it.
 * Why no lane races another on the ring: max_frames_per_call <= W is required, so the frames [p, p + n) of one call have
 * n <= W distinct residues mod W - every entry a call touches is read and written by the one lane that owns its frame,
 * although the workgroups of a slot are not ordered.  An entry is read only for g >= W, when frame g - W of this voice wrote
 * it, so the ring is never cleared; and a value read from it is used only when it lies in [0, cells): nothing the state
 * holds can index outside the grid.
 * The positions must start at 0: vnd_scope_voice_stream_reset_dev enqueues one hipMemsetAsync over the positions ONLY (it
 * ends every voice; every row is cleared when its next voice begins).  A call reads and writes the state and the grid on the
 * call's stream: calls of one pool run in order on one hipStream_t (or are ordered by the caller).
 *
 * *_dev: every array is device memory; valid_dev int32 [slots].  Enqueues three kernels on hip_stream only - a clear kernel
 * (ceil(4 cells / 16 KiB) workgroups a slot, which leave at once unless the slot clears), the bin kernel (ceil(M / 1024)
 * workgroups a slot; idle and bad slots and workgroups past n leave at once) and one lane per slot that writes valid and
 * pos - with grids fixed by (slots, M, cells): no allocation, no synchronisation, no read of device memory by the host, no
 * other stream.  Capturable.
 * Checked before anything is enqueued, with nothing written, first the arguments and last the context (a null ctx is
 * VND_ERR_INVALID): VND_ERR_INVALID for a null pointer; slots, strides, bin counts or max_frames_per_call below 1 (or
 * max_frames_per_call above INT32_MAX: counts are int32); window_frames below 0, or above 0 and below max_frames_per_call; a
 * radius_scale that is NaN, <= 0, or zero or infinite in the sample type; a state_bytes below the query's answer, a state not
 * 16-byte aligned or a grid not 4-byte aligned; grid, valid and the state overlapping one another or the chunk, the edges,
 * counts or flags; extents that overflow.  VND_ERR_UNSUPPORTED for slots above VND_MAX_STREAMS, window_frames above
 * INT32_MAX, a bin count above VND_SCOPE_MAX_BINS, or a launch above 2^23 workgroups (slots * ceil(M / 1024), or slots *
 * ceil(4 cells / 16 KiB)).                                                                                              */
#ifndef VND_SCOPE_VOICE_STREAM_H
#define VND_SCOPE_VOICE_STREAM_H

#include "vnd_amd.h"
#include "vnd_scope.h"
#include "vnd_voice_stream.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The state of a pool, in bytes (see "state" above); window_frames 0 for the whole-voice form.  No context. */
vnd_status vnd_scope_voice_stream_state_bytes(int64_t slots, int64_t max_frames_per_call, int64_t window_frames,
                                              int64_t *bytes);
/* Every position to 0, with the pool's own checks.  The ring and the grid are left alone. */
vnd_status vnd_scope_voice_stream_reset_dev(vnd_ctx *ctx, void *state_dev, int64_t state_bytes, int64_t slots,
                                            int64_t max_frames_per_call, int64_t window_frames, void *hip_stream);

/* grid_dev: uint32 [slots][num_angle_bins][num_radius_bins]. */
vnd_status vnd_polar_hist_voice_stream_f32_dev(vnd_ctx *ctx, void *state_dev, int64_t state_bytes,
                                               int64_t max_frames_per_call, int64_t window_frames, const float *l_dev,
                                               const float *r_dev, int64_t stream_stride, int32_t frame_stride,
                                               const int32_t *counts_dev, const int32_t *flags_dev, int32_t ms_mode,
                                               int32_t semicircular, double radius_scale, const double *angle_edges_dev,
                                               int32_t num_angle_bins, const double *radius_edges_dev,
                                               int32_t num_radius_bins, uint32_t *grid_dev, int32_t *valid_dev,
                                               int64_t slots, void *hip_stream);
vnd_status vnd_polar_hist_voice_stream_f64_dev(vnd_ctx *ctx, void *state_dev, int64_t state_bytes,
                                               int64_t max_frames_per_call, int64_t window_frames, const double *l_dev,
                                               const double *r_dev, int64_t stream_stride, int32_t frame_stride,
                                               const int32_t *counts_dev, const int32_t *flags_dev, int32_t ms_mode,
                                               int32_t semicircular, double radius_scale, const double *angle_edges_dev,
                                               int32_t num_angle_bins, const double *radius_edges_dev,
                                               int32_t num_radius_bins, uint32_t *grid_dev, int32_t *valid_dev,
                                               int64_t slots, void *hip_stream);

/* grid_dev: uint32 [slots][x_bins][y_bins]; L on the first axis. */
vnd_status vnd_lissajous_hist_voice_stream_f32_dev(vnd_ctx *ctx, void *state_dev, int64_t state_bytes,
                                                   int64_t max_frames_per_call, int64_t window_frames, const float *l_dev,
                                                   const float *r_dev, int64_t stream_stride, int32_t frame_stride,
                                                   const int32_t *counts_dev, const int32_t *flags_dev,
                                                   const double *x_edges_dev, int32_t x_bins, const double *y_edges_dev,
                                                   int32_t y_bins, uint32_t *grid_dev, int32_t *valid_dev, int64_t slots,
                                                   void *hip_stream);
vnd_status vnd_lissajous_hist_voice_stream_f64_dev(vnd_ctx *ctx, void *state_dev, int64_t state_bytes,
                                                   int64_t max_frames_per_call, int64_t window_frames, const double *l_dev,
                                                   const double *r_dev, int64_t stream_stride, int32_t frame_stride,
                                                   const int32_t *counts_dev, const int32_t *flags_dev,
                                                   const double *x_edges_dev, int32_t x_bins, const double *y_edges_dev,
                                                   int32_t y_bins, uint32_t *grid_dev, int32_t *valid_dev, int64_t slots,
                                                   void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* VND_SCOPE_VOICE_STREAM_H */

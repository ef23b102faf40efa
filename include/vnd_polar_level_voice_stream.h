/* vnd_polar_level_voice_stream.h - the polar level envelope of a VOICE POOL, exported by libvnd_amd.so: the per-slice
 * percentiles of vnd_level.h for a meter whose slots are voices and whose positions live in device memory, over the last
 * W = window_frames frames of each voice - the outline plot_polar_level draws over the count grid that
 * vnd_scope_voice_stream.h keeps.  Percentiles of blocks do not add up, so the pool keeps the window, not a sum: a ring per
 * slot remembers, for each of the voice's last W frames, exactly what the one-shot entry's stage kernel writes to its work
 * memory - the key (the bit pattern of the radius) and the slice (uint16).  A percentile is an order statistic of a multiset:
 * the order of the ring's entries does not matter, the ring is never unrolled, and vnd_level.h's radix select runs over it as
 * it lies.  It reads the rows and the out_counts of a decorrelating pool (vnd_voice_stream.h, vnd_haas_voice_stream.h)
 * straight from device memory.  A call is a pure function of device memory - no argument depends on the call's history - so
 * it can be captured in a graph and replayed.
 *
 * Same conventions as vnd_scope_voice_stream.h (plain C99, vnd_status, vnd_last_error, "*_dev" = device pointers and a
 * hipStream_t passed as void*), and kept out of vnd_amd.h so that it keeps its fixed set of functions.  Every *_dev entry
 * enqueues on hip_stream only: no allocation, no synchronisation, no read of device memory by the host, no other stream;
 * capturable and thread-safe.  Two entries: the PUSH takes a call's frames into the rings; LEVELS computes the envelope of
 * every slot from the state alone.  Blocks arrive a hundred times a second and a display redraws thirty times: push every
 * block, read when the picture is drawn.
 *
 * ---- push: one call, per slot b -----------------------------------------------------------------------------------------
 * The slot rule of vnd_scope_voice_stream.h.  Read on the device: pos[b] from the state, counts[b] (int32, frames pushed for
 * this slot in this call, 0..M, M = max_frames_per_call) and flags[b] (int32, VND_VOICE_START and VND_VOICE_END of
 * vnd_voice_stream.h; other bits are ignored):
 *     p = START ? 0 : pos[b]                  START: whatever the slot held is dropped
 *     n = counts[b]
 *     for every frame g in [p, p + n):  keys[b][g mod W] = the key of frame g;  bins[b][g mod W] = the slice of frame g
 *     valid[b] = 1
 *     fill[b]  = min(p + n, W)                the ring entries [0, fill[b]) are the voice's
 *     pos[b]   = END ? 0 : p + n              after the call; END leaves fill and the ring as they are: the final envelope
 *                                             stays readable until the slot's next voice
 * A slot with n = 0 and neither flag is idle: valid[b] = 0 and nothing of its state is touched.  START and END in one call
 * are a whole voice in one block.
 * fill is a prefix length.  While a voice has pushed fewer than W frames its entries are [0, p + n) of the ring; from W
 * frames on, every entry is the voice's.  After a START over a full ring the stale entries of the previous voice lie beyond
 * fill and are never read.
 * Why no lane races another on the ring: max_frames_per_call <= W is required, so the frames [p, p + n) of one call have
 * n <= W distinct residues mod W - every entry a call touches is written by the one lane that owns its frame, although the
 * workgroups of a slot are not ordered.  The ring is never cleared and never read by the push.
 *
 * Bad per-slot values (the other slots are unaffected): counts[b] outside [0, M], or - without START - a stored position
 * outside [0, 2^60] (a state that was never reset): valid[b] = -1; the rings, fill and the position of the slot are
 * untouched and nothing is indexed with the bad value.  It is the rule of vnd_voice_stream.h, so a -1 from a decorrelating
 * pool, handed on as a count, passes through the meter as -1.
 *
 * The key and the slice of a frame are formed by the very device function vnd_polar_level_*_dev stages with: the polar
 * sample, the degrees, the reference's mask on float64 edges (a frame at exactly the last edge belongs to no slice: 0xFFFF)
 * and radius / sample_type(radius_scale).  Only radius_scale > 0 is accepted: a per-voice maximum cannot stream (a later
 * block's maximum would rescale the earlier frames).  The edges are the same for every call of a pool (the ring holds slices
 * of THESE edges), num_bins + 1 ascending float64 values in device memory.
 *
 * Chunk: frame t (0 <= t < counts[b]) of slot b: L at l_dev[b * stream_stride + t * frame_stride], R at r_dev likewise, in
 * elements (l_dev and r_dev may be channels 0 and 1 of one (slots, M, 2) block: stream_stride 2 M, frame_stride 2).  Only
 * the first counts[b] frames of row b are read.  *_f32_dev takes float32, *_f64_dev float64.  valid_dev: int32 [slots].
 * Two kernels: the stage kernel (ceil(M / 1024) workgroups a slot; idle and bad slots and workgroups past n leave at once)
 * and one lane per slot that writes valid, fill and pos.
 *
 * ---- levels -------------------------------------------------------------------------------------------------------------
 * A pure function of the state.  levels_dev: [slots][num_percentiles][num_bins] of the sample type; bin_counts_dev: uint32
 * [slots][num_bins]; both fully written by every successful call.
 * Contract.  Slot b's rows equal BYTE FOR BYTE what vnd_polar_level_*_dev (vnd_level.h) writes, with the same edges, mode,
 * radius_scale and percentiles, for the fill[b] frames the ring holds: the frames [max(0, q - W), q) of the slot's current or
 * last voice, q its position after its last answered push - for every schedule of counts, idle calls, restarts and
 * neighbours.  A slot that never started, or one whose fill lies outside [0, W] (a state that was never reset), contributes
 * no frame: levels 0, counts 0.  A slice read from the ring is compared with num_bins where it is read: nothing the state
 * holds can index outside an array.
 * The slice counts are recounted from the ring on every call (2 bytes a frame beside a select that reads 6 or 10 bytes a
 * frame on every pass), then vnd_level.h's init, select, advance, min and finish kernels run as they are with the rings as
 * their staged keys and bins and fill as n_each.  percentiles: num_percentiles values in HOST memory, read at the call.
 * work_dev: caller-owned, 8-byte aligned, at least vnd_polar_level_voice_stream_work_bytes(...) bytes: the select's cell state
 * and digit histograms only - the keys are in the state.  The entry clears what it needs cleared on hip_stream itself.
 *
 * ---- state --------------------------------------------------------------------------------------------------------------
 * `state_bytes` at least what vnd_polar_level_voice_stream_state_bytes returns, state_dev 16-byte aligned.  In this order,
 * each part padded to a multiple of 16 bytes:
 *     positions  int64 [slots]
 *     fill       int32 [slots]
 *     keys       [slots][W]: uint32 for float32 frames, uint64 for float64
 *     bins       uint16 [slots][W]; 0xFFFF: the frame falls in no slice
 * Positions and fills must start at 0: vnd_polar_level_voice_stream_reset_dev enqueues one hipMemsetAsync over those two
 * (and their padding) ONLY (it ends every voice; the rings are never cleared).  Push and levels read and write the state on
 * the call's stream: calls of one pool run in order on one hipStream_t (or are ordered by the caller).
 *
 * ---- refusals -----------------------------------------------------------------------------------------------------------
 * Checked before anything is enqueued, with nothing written, first the arguments and last the context (a null ctx is
 * VND_ERR_INVALID).  VND_ERR_INVALID: a null pointer; slots, a stride, num_bins, num_percentiles or max_frames_per_call below
 * 1 (or max_frames_per_call above INT32_MAX: counts are int32); window_frames below max_frames_per_call; a percentile outside
 * [0, 100] or NaN; a radius_scale that is NaN, <= 0, or zero or infinite in the sample type; state_bytes or work_bytes below
 * the query's answer; a state not 16-byte aligned or work not 8-byte aligned; outputs (valid; levels, bin_counts, work) and
 * the state overlapping one another or any input (the chunk, the edges, counts, flags); extents that overflow.
 * VND_ERR_UNSUPPORTED: slots above VND_MAX_STREAMS; window_frames above INT32_MAX; num_bins above VND_LEVEL_MAX_BINS;
 * num_percentiles above VND_LEVEL_MAX_PERCENTILES; more than 2^23 workgroups in a launch (slots * ceil(M / 1024) for the push,
 * slots * ceil(W / VND_LEVEL_SPAN_FRAMES) for the levels).                                                                  */
#ifndef VND_POLAR_LEVEL_VOICE_STREAM_H
#define VND_POLAR_LEVEL_VOICE_STREAM_H

#include "vnd_amd.h"
#include "vnd_level.h"
#include "vnd_voice_stream.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The state of a pool, in bytes (see "state" above).  No context. */
vnd_status vnd_polar_level_voice_stream_state_bytes(int64_t slots, int64_t max_frames_per_call, int64_t window_frames,
                                                    int32_t is_float64, int64_t *bytes);
/* Every position and every fill to 0, with the pool's own checks.  The rings are left alone. */
vnd_status vnd_polar_level_voice_stream_reset_dev(vnd_ctx *ctx, void *state_dev, int64_t state_bytes, int64_t slots,
                                                  int64_t max_frames_per_call, int64_t window_frames, int32_t is_float64,
                                                  void *hip_stream);

vnd_status vnd_polar_level_voice_stream_push_f32_dev(vnd_ctx *ctx, void *state_dev, int64_t state_bytes,
                                                     int64_t max_frames_per_call, int64_t window_frames, const float *l_dev,
                                                     const float *r_dev, int64_t stream_stride, int32_t frame_stride,
                                                     const int32_t *counts_dev, const int32_t *flags_dev, int32_t ms_mode,
                                                     int32_t semicircular, double radius_scale,
                                                     const double *angle_edges_dev, int32_t num_bins, int32_t *valid_dev,
                                                     int64_t slots, void *hip_stream);
vnd_status vnd_polar_level_voice_stream_push_f64_dev(vnd_ctx *ctx, void *state_dev, int64_t state_bytes,
                                                     int64_t max_frames_per_call, int64_t window_frames, const double *l_dev,
                                                     const double *r_dev, int64_t stream_stride, int32_t frame_stride,
                                                     const int32_t *counts_dev, const int32_t *flags_dev, int32_t ms_mode,
                                                     int32_t semicircular, double radius_scale,
                                                     const double *angle_edges_dev, int32_t num_bins, int32_t *valid_dev,
                                                     int64_t slots, void *hip_stream);

/* Bytes of work memory for a levels call of this shape.  No context. */
vnd_status vnd_polar_level_voice_stream_work_bytes(int64_t slots, int64_t window_frames, int32_t num_bins,
                                                   int32_t num_percentiles, int32_t is_float64, int64_t *bytes);

/* levels_dev: [slots][num_percentiles][num_bins]; bin_counts_dev: uint32 [slots][num_bins].  percentiles: HOST memory. */
vnd_status vnd_polar_level_voice_stream_levels_f32_dev(vnd_ctx *ctx, const void *state_dev, int64_t state_bytes,
                                                       int64_t max_frames_per_call, int64_t window_frames, int32_t num_bins,
                                                       const double *percentiles, int32_t num_percentiles, float *levels_dev,
                                                       uint32_t *bin_counts_dev, void *work_dev, int64_t work_bytes,
                                                       int64_t slots, void *hip_stream);
vnd_status vnd_polar_level_voice_stream_levels_f64_dev(vnd_ctx *ctx, const void *state_dev, int64_t state_bytes,
                                                       int64_t max_frames_per_call, int64_t window_frames, int32_t num_bins,
                                                       const double *percentiles, int32_t num_percentiles, double *levels_dev,
                                                       uint32_t *bin_counts_dev, void *work_dev, int64_t work_bytes,
                                                       int64_t slots, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* VND_POLAR_LEVEL_VOICE_STREAM_H */

/* vnd_polar_voice_stream.h - the eight polar moments of vnd_polar_moments_f32_dev (vnd_amd.h) for a VOICE POOL, exported
 * by libvnd_amd.so: a meter whose slots are voices and whose positions live in device memory, as
 * vnd_correlogram_voice_stream.h is for the correlogram.  After every call each slot's moments are those of that voice's
 * whole output so far, so the symmetry-aware objective of a live voice is one row of 64 bytes away.  It reads the rows and
 * the out_counts of a decorrelating pool (vnd_voice_stream.h, vnd_haas_voice_stream.h) straight from device memory.  A
 * call is a pure function of device memory - no argument depends on the call's history - so it can be captured in a graph
 * and replayed.
 *
 * Same conventions as vnd_correlogram_voice_stream.h (plain C99, vnd_status, vnd_last_error, "*_dev" = device pointers and
 * a hipStream_t passed as void*), and kept out of vnd_amd.h so that it keeps its fixed set of functions.
 *
 * ---- one call, per slot b ---------------------------------------------------------------------------------------------
 * Read on the device: pos[b] from the state, counts[b] (int32, frames pushed for this slot in this call, 0..M, M =
 * max_frames_per_call) and flags[b] (int32, VND_VOICE_START and VND_VOICE_END of vnd_voice_stream.h; other bits are
 * ignored).
 *     p = START ? 0 : pos[b]                  START: whatever the slot held is dropped
 *     n = counts[b]
 *     moments[b][0..7] = the eight moments of frames [0, p + n) of the voice
 *         { sum r, sum r theta, sum r theta^2, sum r theta^3, max |theta|, sum L R, sum L^2, sum R^2 }
 *     valid[b] = 1
 *     pos[b]   = END ? 0 : p + n              after the call
 * A slot with n = 0 and neither flag is idle: valid[b] = 0, its moments row is left untouched and nothing of its state
 * changes.  START and END in one call are a whole voice in one block.  END with n = 0 reports the voice's final moments;
 * a voice of no frames has eight zeros.
 *
 * Contract, float32 (*_f32_dev).  Take one voice: the calls from a START - or from position 0 after an END or a reset - up
 * to the current one.  After each of them moments[b] equals vnd_polar_moments_f32_dev(y, n, n_pairs = 1, ...) on the
 * concatenation of the frames it has pushed so far, BIT FOR BIT, for every schedule of counts, idle calls and neighbours.
 * That call sums in a fixed order that depends on absolute frame positions only - chunk c is frames [512 c, 512 c + 512);
 * lane t of 256 adds frames 512 c + t and 512 c + 256 + t; a shuffle tree 32..1 per wave; the four waves in order; reduce
 * lane t adds the chunk partials c = t (mod 256) in ascending c from +0.0; the same tree again; max |theta| through fmax
 * along the same path - and this meter keeps exactly that order: it carries the 256 reduce-lane sums of the completed
 * chunks and the frames of the chunk still incomplete.
 * Contract, float64 (*_f64_dev): theta, r and the products in float64, as NumPy computes them on float64 arrays (no cast
 * to float32), in the same summation order.  The moments do not depend on the schedule, bit for bit.
 *
 * Bad per-slot values (the other slots are unaffected): counts[b] outside [0, M], or - without START - a stored position
 * outside [0, 2^60] (a state that was never reset): valid[b] = -1; the moments row, the position, the sums and the ring of
 * the slot are untouched and nothing is indexed with the bad value.  It is the rule of vnd_voice_stream.h, so a -1 from a
 * decorrelating pool, handed on as a count, passes through the meter as -1.
 *
 * ---- chunk ------------------------------------------------------------------------------------------------------------
 * Frame t (0 <= t < counts[b]) of slot b: L at l_dev[b * stream_stride + t * frame_stride], R at r_dev likewise, in
 * elements (l_dev and r_dev may be channels 0 and 1 of one (slots, M, 2) block: stream_stride 2 M, frame_stride 2).  Only
 * the first counts[b] frames of row b are read.  *_f32_dev takes float32, *_f64_dev float64.
 *
 * ---- state ------------------------------------------------------------------------------------------------------------
 * `state_bytes` at least what vnd_polar_voice_stream_state_bytes returns for the sample size (4: float32, 8: float64),
 * state_dev 16-byte aligned.  With G = ceil(M / 512) + 1 and cap = 511 + M, in this order:
 *     positions  int64 [slots], padded to a multiple of 16 bytes
 *     sums       float64 [slots][256][8]: reduce lane t's running sums over the completed chunks c = t (mod 256).  Lane t
 *                is read only when t < floor(p / 512), so the sums are logically zero at START and are never cleared
 *     partials   float64 [slots][G][8]: scratch of one call, the chunk partials between its two kernels
 *     ring       [slots][cap] (L, R) pairs of the sample type: the frames of the chunk still incomplete, ring slot = the
 *                voice's absolute frame mod cap.  A call reads frames in [p - 511, p) and writes frames in [p, p + n):
 *                a written frame g and a read frame f have 0 < g - f <= 510 + n < cap, so no slot is both read and
 *                written in one call.  A call with END writes nothing to it.  The ring is never cleared
 * The positions must start at 0: vnd_polar_voice_stream_reset_dev enqueues one hipMemsetAsync over the positions ONLY (it
 * ends every voice).  A call reads and writes the state on the call's stream: calls of one pool run in order on one
 * hipStream_t (or are ordered by the caller).
 *
 * *_dev: every array is device memory; moments_dev is float64 [slots][8], valid_dev int32 [slots].  Enqueues two kernels
 * on hip_stream only - G workgroups per slot that form the partials of the chunks the call touches and keep the incomplete
 * chunk's frames, then one workgroup per slot that folds them into the lane sums and writes moments, valid and pos - with
 * a grid fixed by (slots, M): no allocation, no synchronisation, no read of device memory by the host, no other stream.
 * Capturable.
 * Checked before anything is enqueued, with nothing written: VND_ERR_INVALID for a null pointer; slots, strides or
 * max_frames_per_call below 1 (or max_frames_per_call above INT32_MAX: counts are int32); a sample size other than 4 or
 * 8; a state_bytes below the query's answer or a state not 16-byte aligned; moments, valid, the state and the chunk
 * overlapping one another; extents that overflow.  VND_ERR_UNSUPPORTED for slots above VND_MAX_STREAMS, G above 65535 or
 * slots * G above 2^23.                                                                                                 */
#ifndef VND_POLAR_VOICE_STREAM_H
#define VND_POLAR_VOICE_STREAM_H

#include "vnd_amd.h"
#include "vnd_voice_stream.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The state of a pool, in bytes (see "state" above); sample_bytes 4 for *_f32_dev, 8 for *_f64_dev.  No context. */
vnd_status vnd_polar_voice_stream_state_bytes(int64_t slots, int64_t max_frames_per_call, int32_t sample_bytes,
                                              int64_t *bytes);
/* Every position to 0, with the pool's own checks: state_bytes is held to the size for sample_bytes. */
vnd_status vnd_polar_voice_stream_reset_dev(vnd_ctx *ctx, void *state_dev, int64_t state_bytes, int64_t slots,
                                            int64_t max_frames_per_call, int32_t sample_bytes, void *hip_stream);
vnd_status vnd_polar_voice_stream_f32_dev(vnd_ctx *ctx, void *state_dev, int64_t state_bytes, int64_t max_frames_per_call,
                                          const float *l_dev, const float *r_dev, int64_t stream_stride,
                                          int32_t frame_stride, const int32_t *counts_dev, const int32_t *flags_dev,
                                          double *moments_dev, int32_t *valid_dev, int64_t slots, void *hip_stream);
vnd_status vnd_polar_voice_stream_f64_dev(vnd_ctx *ctx, void *state_dev, int64_t state_bytes, int64_t max_frames_per_call,
                                          const double *l_dev, const double *r_dev, int64_t stream_stride,
                                          int32_t frame_stride, const int32_t *counts_dev, const int32_t *flags_dev,
                                          double *moments_dev, int32_t *valid_dev, int64_t slots, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* VND_POLAR_VOICE_STREAM_H */

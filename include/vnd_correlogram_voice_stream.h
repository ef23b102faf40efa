/* vnd_correlogram_voice_stream.h - the cross-correlogram of vnd_correlogram_f32_dev (vnd_analysis.h) for a VOICE POOL,
 * exported by libvnd_amd.so: vnd_correlogram_stream_f32_dev (vnd_correlogram_stream.h) with the stream position moved
 * from the caller into the device state, one per slot, and with a frame count and start / end flags per slot and call,
 * as vnd_voice_stream.h does it for the decorrelating pools.  It reads the rows and the out_counts of such a pool straight
 * from device memory, so "decorrelate, then meter" is one chain of launches with no host in it.  A call is a pure
 * function of device memory - no argument depends on the call's history - so it can be captured in a graph and replayed.
 *
 * Same conventions as vnd_analysis.h (plain C99, vnd_status, vnd_last_error, "*_dev" = device pointers and a hipStream_t
 * passed as void*), and kept out of vnd_amd.h and vnd_analysis.h so that both keep their fixed sets of functions.
 *
 * ---- one call, per slot b ---------------------------------------------------------------------------------------------
 * Read on the device: pos[b] from the state, counts[b] (int32, frames pushed for this slot in this call, 0..M, M =
 * max_frames_per_call) and flags[b] (int32, VND_VOICE_START and VND_VOICE_END of vnd_voice_stream.h; other bits are
 * ignored).  W = window, H = hop.
 *     p  = START ? 0 : pos[b]                 START: whatever the slot held is dropped
 *     n  = counts[b]
 *     wc(q) = q >= W ? (q - W) / H + 1 : 0    (windows complete after q frames)
 *     w0 = wc(p)
 *     out_counts[b] = wc(p + n) - w0          <= RC = ceil(M / H), the rows per call
 *     pos[b]        = END ? 0 : p + n         after the call
 * Row r < out_counts[b] of slot b is the correlogram row of window w0 + r of that voice, frames [(w0 + r) H, (w0 + r) H
 * + W).  Windows that never complete are dropped, as in the reference, so END has no tail: it returns what this call's
 * frames completed and puts the position back to 0 (END with n = 0: 0 rows).  A slot with n = 0 and no flag does nothing.
 * START and END in one call are a whole voice in one block.
 * Why out_counts[b] <= RC for every p, H > W included: let g(q) = floor((q - W) / H) + 1 for every integer q.  For q < W
 * the floor is at most -1, so g(q) <= 0; for q >= W, g(q) >= 1 and wc(q) = g(q): wc = max(0, g).  g(p + n) - g(p) =
 * floor(a + n / H) - floor(a) with a = (p - W) / H, at most ceil(n / H); t -> max(0, t) never widens a difference of
 * ordered values, so wc(p + n) - wc(p) <= ceil(n / H) <= ceil(M / H).
 *
 * out is float32 [slots][RC][num_lags]: the call writes the first out_counts[b] rows of row-block b and nothing at or
 * past them.  The strides are fixed by the pool, so no shape depends on data.  out_counts is int32 [slots].
 *
 * Contract.  Take one voice: the calls from a START - or from position 0 after an END or a reset - up to and including
 * its END.  The concatenation of its rows equals vnd_correlogram_f32_dev on that voice's whole signal, bit for bit, for
 * every schedule of counts, idle calls and neighbours, under the same numerics (float64 sums, the float32 normaliser,
 * silent and overflowing windows 0).
 *
 * Bad per-slot values (the other slots are unaffected): counts[b] outside [0, M], or - without START - a stored position
 * outside [0, 2^60] (a state that was never reset): out_counts[b] = -1; the rows, the position and the ring of the slot
 * are untouched and nothing is indexed with the bad value.  It is the rule of vnd_voice_stream.h, so a -1 from a
 * decorrelating pool, handed on as a count, passes through the meter as -1.
 *
 * ---- chunk ------------------------------------------------------------------------------------------------------------
 * Frame t (0 <= t < counts[b]) of slot b at x_dev[b * stream_stride + t * frame_stride], y_dev likewise, in elements
 * (x_dev and y_dev may be channels 0 and 1 of one (slots, M, 2) block: stream_stride 2 M, frame_stride 2).  Only the first
 * counts[b] frames of row b are read.  *_f32_dev takes float32.  *_f64_dev takes float64 - what the Haas and chain voice
 * pools return - and casts each sample to float32 as it reads it (round to nearest even, C's conversion); the ring keeps
 * the cast value, and the rows equal vnd_correlogram_f32_dev on the cast signal bit for bit.  Nothing is allocated and
 * nothing extra is launched for the cast.
 *
 * ---- state ------------------------------------------------------------------------------------------------------------
 * `state_bytes` at least what vnd_correlogram_voice_stream_state_bytes returns, state_dev 16-byte aligned: first one int64
 * position per slot (padded to a multiple of 16 bytes), then the ring of vnd_correlogram_stream.h, per slot W - 1 + M
 * interleaved float32 (x, y) pairs, ring slot = the voice's absolute frame mod capacity.  A call copies the last
 * min(n, W - 1) frames of each slot's chunk into its ring; a call with END writes nothing to it.  The ring is never
 * cleared and needs no clearing: a voice reads no frame below its own 0.  The positions must start at 0:
 * vnd_correlogram_voice_stream_reset_dev enqueues one hipMemsetAsync over the positions ONLY (it ends every voice).  A
 * call reads and writes the state on the call's stream: calls of one pool run in order on one hipStream_t (or are
 * ordered by the caller).
 *
 * *_dev: every array is device memory.  Enqueues two kernels on hip_stream only - the pool's rows, then one lane per slot
 * that writes pos and out_counts - with a grid fixed by (slots, M, W, H, num_lags): no allocation, no synchronisation, no
 * read of device memory by the host, no other stream.  Capturable.
 * Checked before anything is enqueued, with nothing written: VND_ERR_INVALID for a null pointer; slots, strides, window,
 * hop, num_lags or max_frames_per_call below 1 (or max_frames_per_call above INT32_MAX: counts are int32); a state_bytes
 * below the query's answer or a state not 16-byte aligned; out overlapping the chunk or the state, or the state
 * overlapping the chunk; extents that overflow.  VND_ERR_UNSUPPORTED for a window above VND_CORRELOGRAM_MAX_WINDOW, slots
 * above VND_MAX_STREAMS, ceil(RC / 4) * ceil(num_lags / 1024) workgroups per slot above 65535 or above 2^23 in the whole
 * launch, and an out of more than 2^40 values.                                                                          */
#ifndef VND_CORRELOGRAM_VOICE_STREAM_H
#define VND_CORRELOGRAM_VOICE_STREAM_H

#include "vnd_correlogram_stream.h"
#include "vnd_voice_stream.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The state of a pool: the positions (8 bytes a slot, padded to 16) and slots * (window - 1 + max_frames_per_call) * 8
 * bytes of ring.  No context.  VND_ERR_INVALID for slots, window or max_frames_per_call below 1, or a size that
 * overflows; VND_ERR_UNSUPPORTED for a window above VND_CORRELOGRAM_MAX_WINDOW or slots above VND_MAX_STREAMS. */
vnd_status vnd_correlogram_voice_stream_state_bytes(int64_t slots, int32_t window, int64_t max_frames_per_call,
                                                    int64_t *bytes);
vnd_status vnd_correlogram_voice_stream_reset_dev(vnd_ctx *ctx, void *state_dev, int64_t state_bytes, int64_t slots,
                                                  int32_t window, int64_t max_frames_per_call, void *hip_stream);
vnd_status vnd_correlogram_voice_stream_f32_dev(vnd_ctx *ctx, void *state_dev, int64_t state_bytes,
                                                int64_t max_frames_per_call, const float *x_dev, const float *y_dev,
                                                int64_t stream_stride, int32_t frame_stride, const int32_t *counts_dev,
                                                const int32_t *flags_dev, float *out_dev, int32_t *out_counts_dev,
                                                int64_t slots, int32_t window, int32_t hop, int32_t num_lags, float eps,
                                                void *hip_stream);
vnd_status vnd_correlogram_voice_stream_f64_dev(vnd_ctx *ctx, void *state_dev, int64_t state_bytes,
                                                int64_t max_frames_per_call, const double *x_dev, const double *y_dev,
                                                int64_t stream_stride, int32_t frame_stride, const int32_t *counts_dev,
                                                const int32_t *flags_dev, float *out_dev, int32_t *out_counts_dev,
                                                int64_t slots, int32_t window, int32_t hop, int32_t num_lags, float eps,
                                                void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* VND_CORRELOGRAM_VOICE_STREAM_H */

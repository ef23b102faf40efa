/* vnd_voice_fade_stream.h - a CROSSFADING VOICE POOL, exported by libvnd_amd.so: the voice pool of vnd_voice_stream.h whose
 * live voices can change their filter.  A call may carry VND_VOICE_SWITCH for a slot: from the first frame the slot has
 * not yet returned, its output fades over `fade_frames` frames from the filter it had to tables[b] of that call.  The voice
 * keeps its position, its H frames of history and its latency; nothing is discarded and no frame is returned twice.  One
 * fade per voice is in flight at a time: a switch that arrives before the previous fade was returned whole is ignored.
 *
 * Same conventions as vnd_voice_stream.h (plain C99, vnd_status, vnd_last_error, "*_dev" = device pointers and a
 * hipStream_t passed as void*; VND_MODE_EXACT only, mono or stereo in, stereo out, no normaliser).  x, counts, flags,
 * tables, y and out_counts have that header's shapes and meaning; H is the bank's largest tap index, M =
 * max_frames_per_call, T the bank's candidates.  vnd_voice_stream_f32_* and its state are untouched by this header.
 *
 * ---- the pool ---------------------------------------------------------------------------------------------------------
 * Built with fade_frames = F, 0 <= F <= VND_VOICE_FADE_MAX_FRAMES, and a device array `gains` of float32 [2][F]: row 0 the
 * fade-out gains, row 1 the fade-in gains, frame j of a fade scaled by gains[.][j].  gains may be null only when F == 0.
 * The same F and gains go to every call of one pool.
 *
 * ---- state ------------------------------------------------------------------------------------------------------------
 * `state_bytes` at least what vnd_voice_fade_stream_state_bytes returns, state_dev 16-byte aligned.  In this order:
 *   1. one int64 position per slot, padded to a multiple of 16 bytes (as vnd_voice_stream.h);
 *   2. one 16-byte record per slot: int64 s; int32 old; int32 cur - the first frame of the slot's latest fade, the table
 *      before it and the table after it;
 *   3. the ring of vnd_each_stream.h, capacity H + M frames per slot, ring slot = the voice's absolute frame mod capacity.
 * vnd_voice_fade_stream_reset_dev zeroes the positions ONLY.  Neither the records nor the ring need clearing: a slot at
 * position 0 is `fresh` below and takes its record from the call, and a voice never reads a frame below its position 0.
 *
 * ---- one call, per slot b ---------------------------------------------------------------------------------------------
 *     fresh = START || stored_pos == 0             a voice begins; the SWITCH bit is ignored
 *     p  = fresh ? 0 : stored_pos                  bad count / bad p: exactly vnd_voice_stream.h's rule
 *                                                  (out_counts = -1, fade_left = -1, nothing of the slot changes)
 *     n  = counts[b];  E = max(0, p - H);  E' = END ? p + n : max(0, p + n - H)
 *     (old, cur, s) = fresh ? (tables[b], tables[b], -F) : the stored record
 *     accept = SWITCH && !fresh && E >= s + F      the previous fade has been returned whole
 *     if accept: (old, cur, s) = (cur, tables[b], E)   the fade begins at the first frame not yet returned
 *     convolved frame f in [E, E'):
 *         f <  s      -> C_old[f]
 *         f >= s + F  -> C_cur[f]
 *         else        -> C_old[f] * gains[0][f - s] + C_cur[f] * gains[1][f - s]
 *                        float32: two rounded products, one rounded sum (the library is built with contraction off)
 *     then ms_encode / width, the stage's pointwise steps, on the result, as vnd_voice_stream.h
 *     after: pos = END ? 0 : p + n;  record = (old, cur, s);  out_counts = E' - E
 *            fade_left[b] = END ? 0 : min(F, max(0, s + F - E'))
 * C_t[f] is the plain convolution of the voice's whole signal with table t alone: the bits vnd_decorrelate_each_f32_*
 * gives without normaliser or pointwise steps.  Frame differences such as f - s are formed in int64; positions go up to
 * 2^60.
 *
 * tables[b] is read only when `fresh` or `accept` holds.  A SWITCH that is not accepted is ignored and the voice goes on as
 * planned.  A SWITCH is accepted exactly when the slot's fade_left after the previous call was 0: that is why fade_left is
 * an output.  fade_left is int32 [slots] and may be null.
 *
 * Consequences: a voice that never switches returns vnd_voice_stream_f32_*'s bytes; F == 0 is a hard switch at E;
 * switching to the table the voice already has is a fade like any other (a * g0 + a * g1 is computed).
 *
 * Bad per-slot values are vnd_voice_stream.h's.  A frame whose value depends on a table outside [0, T) is NaN: after a
 * switch to a bad table the frames below s are still the old table's and the frames from s on are NaN; the position
 * advances as in the existing pool.
 *
 * ---- entry points -----------------------------------------------------------------------------------------------------
 * *_dev: every array is device memory.  Enqueues two kernels on hip_stream only - the pool's frames, then one lane per
 * slot that writes pos, the record, out_counts and fade_left - with a grid fixed by (slots, M, H): no allocation, no
 * synchronisation, no read of device memory by the host, no other stream.  Capturable.  There is no *_host entry.
 * Checked before anything is enqueued, with nothing written: everything vnd_voice_stream.h lists, as it lists it, and
 * VND_ERR_INVALID for fade_frames < 0 and for a null gains with fade_frames > 0; VND_ERR_UNSUPPORTED for fade_frames above
 * VND_VOICE_FADE_MAX_FRAMES.                                                                                             */
#ifndef VND_VOICE_FADE_STREAM_H
#define VND_VOICE_FADE_STREAM_H

#include "vnd_voice_stream.h"

#define VND_VOICE_SWITCH 4
#define VND_VOICE_FADE_MAX_FRAMES (1 << 20)

#ifdef __cplusplus
extern "C" {
#endif

vnd_status vnd_voice_fade_stream_state_bytes(const vnd_taps *bank, int64_t slots, int32_t in_channels,
                                             int64_t max_frames_per_call, int64_t fade_frames, int64_t *bytes);
vnd_status vnd_voice_fade_stream_reset_dev(vnd_ctx *ctx, void *state_dev, int64_t state_bytes, int64_t slots,
                                           int32_t in_channels, const vnd_taps *bank, int64_t max_frames_per_call,
                                           int64_t fade_frames, void *hip_stream);
vnd_status vnd_voice_fade_stream_f32_dev(vnd_ctx *ctx, const vnd_taps *bank, void *state_dev, int64_t state_bytes,
                                         int64_t max_frames_per_call, int64_t fade_frames, const float *gains_dev,
                                         const float *x_dev, const int32_t *counts_dev, const int32_t *flags_dev,
                                         const int32_t *tables_dev, float *y_dev, int32_t *out_counts_dev,
                                         int32_t *fade_left_dev, int64_t slots, int32_t in_channels, int32_t mode,
                                         int32_t ms_encode, int32_t use_width, double width, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* VND_VOICE_FADE_STREAM_H */

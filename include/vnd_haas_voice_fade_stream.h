/* vnd_haas_voice_fade_stream.h - a CROSSFADING VOICE POOL OF HAAS DELAYS, exported by libvnd_amd.so: the Haas voice pool of
 * vnd_haas_voice_stream.h whose live voices can change their delay - the Haas sibling of vnd_voice_fade_stream.h.  A call
 * may carry VND_VOICE_SWITCH for a slot: from the first frame the slot has not yet returned, its delayed column fades over
 * `fade_frames` frames from the delay it had to delays[b] of that call.  The voice keeps its position and its ring; nothing
 * is discarded and no frame is returned twice.  One fade per voice is in flight at a time: a switch that arrives before
 * the previous fade was returned whole is ignored.
 *
 * Same conventions as vnd_haas_voice_stream.h (plain C99, vnd_status, vnd_last_error, "*_dev" = device pointers and a
 * hipStream_t passed as void*; mono or stereo float32 in, stereo FLOAT64 out).  x, counts, flags, delays, y and out_counts
 * have that header's shapes and meaning; M = max_frames_per_call; delayed_channel, ms_mode, use_width and width are
 * scalars of the call.  vnd_haas_voice_stream_f64_* and its state are untouched by this header.
 *
 * ---- the pool ---------------------------------------------------------------------------------------------------------
 * Built with fade_frames = F, 0 <= F <= VND_VOICE_FADE_MAX_FRAMES, and a device array `gains` of float32 [2][F] - the very
 * array vnd_voice_fade_stream.h takes, so that a chain fades both of its stages on one curve: row 0 the fade-out gains,
 * row 1 the fade-in gains, frame j of a fade scaled by gains[.][j].  gains may be null only when F == 0.  The same F and
 * gains go to every call of one pool.
 *
 * ---- state ------------------------------------------------------------------------------------------------------------
 * `state_bytes` at least what vnd_haas_voice_fade_stream_state_bytes returns, state_dev 16-byte aligned.  In this order:
 *   1. one int64 position per slot, padded to a multiple of 16 bytes (as vnd_haas_voice_stream.h);
 *   2. one 16-byte record per slot: int64 s; int32 old; int32 cur - the first frame of the slot's latest fade, and the
 *      DELAY IN FRAMES before it and after it;
 *   3. the Haas ring of vnd_each_stream.h, capacity max_delay + M frames per slot, ring slot = the voice's absolute frame
 *      mod capacity (none with max_delay = 0).  A switch needs no more ring: both delays are at most max_delay, and the
 *      ring holds [p - max_delay, p) already.
 * vnd_haas_voice_fade_stream_reset_dev zeroes the positions ONLY.  Neither the records nor the ring need clearing: a slot
 * at position 0 is `fresh` below and takes its record from the call, and a voice never reads a frame below its position 0.
 *
 * ---- one call, per slot b ---------------------------------------------------------------------------------------------
 * All frame differences are formed in int64; positions go up to 2^60.
 *     work   = counts[b] > 0 || START || END || SWITCH   an idle slot changes nothing; delays[b] is not looked at
 *     fresh  = START || stored_pos == 0                   a voice begins; the SWITCH bit is ignored
 *     p      = fresh ? 0 : stored_pos;   n = counts[b];   e = p + n
 *     (old, cur, s) = fresh ? (delays[b], delays[b], -F) : the stored record
 *     accept = SWITCH && !fresh && p >= s + F             the previous fade has been returned whole
 *     if accept: (old, cur, s) = (cur, delays[b], p)      Haas has no latency: the first frame not yet returned is p
 *     tail   = max(cur, min(old, max(0, s + F - e)))      END only
 *     out_counts = n + (END ? tail : 0)                   <= M + max_delay
 *     the delayed column of output frame t in [p, p + out_counts), with D_d[t] = the column of input frame t - d as
 *     vnd_haas_voice_stream.h reads it (ring below p, chunk in [p, e), zero below 0 and at or past e):
 *         t <  s      -> D_old[t]
 *         t >= s + F  -> D_cur[t]
 *         else        -> D_old[t] * (double)gains[0][t - s] + D_cur[t] * (double)gains[1][t - s]
 *                        float64: two rounded products, one rounded sum (the library is built with contraction off)
 *     the undelayed column (input frame t), then the MS decode, the mono compensation and the width on the pair, exactly
 *     as vnd_haas_voice_stream.h
 *     after: pos = END ? 0 : e;  record = (old, cur, s);  fade_left[b] = END ? 0 : min(F, max(0, s + F - e))
 * An idle slot (no work) answers out_counts = 0 and the fade_left its stored state gives (0 at position 0); its position
 * and record stay as they are.
 *
 * `tail` covers every frame to which either delay can still contribute: the new delay up to e + cur, the old one to frame
 * t only while t < s + F and t - old < e.  The fade goes on through the tail of an END: its frames are blended by the same
 * rule, and the length of the tail depends on the fade - in vnd_voice_fade_stream.h it is the bank's latency, whatever fades.
 *
 * delays[b] is read only when the slot is fresh and has work, or when `accept` holds.  A SWITCH that is not accepted is
 * ignored and the voice goes on as planned.  A SWITCH is accepted exactly when the slot's fade_left after the previous call
 * was 0: that is why fade_left is an output.  fade_left is int32 [slots] and may be null.
 *
 * Consequences: a voice that never switches returns vnd_haas_voice_stream_f64_dev's bytes - outside [s, s + F) a frame is
 * a SELECT of one delay's column, never a * 1 + b * 0; F == 0 is a hard switch at p; switching to the delay the voice
 * already has is a fade like any other (a * g0 + a * g1 is computed).
 *
 * Bad per-slot values (the other slots' bits are unchanged in every case): out_counts[b] = fade_left[b] = -1, row b of y,
 * the position, the record and the ring are untouched, and nothing is indexed with the bad value, for
 *   - counts[b] outside [0, M], or a stored position outside [0, 2^60] without START: vnd_haas_voice_stream.h's rule;
 *   - delays[b] outside [0, max_delay] on a call that would take it: a fresh slot with work, or an accepted SWITCH.  A
 *     refused SWITCH does not read delays[b];
 *   - on a slot that is not fresh and has work, a stored record whose old or cur lies outside [0, max_delay]: a state no
 *     call of this pool wrote.
 *
 * ---- entry points -----------------------------------------------------------------------------------------------------
 * *_dev: every array is device memory.  Enqueues two kernels on hip_stream only - the pool's frames, then one lane per
 * slot that writes pos, the record, out_counts and fade_left - with a grid fixed by (slots, M, max_delay): no allocation,
 * no synchronisation, no read of device memory by the host, no other stream.  Capturable.  There is no *_host entry.
 * Checked before anything is enqueued, with nothing written: everything vnd_haas_voice_stream.h lists, as it lists it, and
 * VND_ERR_INVALID for fade_frames < 0 and for a null gains with fade_frames > 0; VND_ERR_UNSUPPORTED for fade_frames above
 * VND_VOICE_FADE_MAX_FRAMES.                                                                                             */
#ifndef VND_HAAS_VOICE_FADE_STREAM_H
#define VND_HAAS_VOICE_FADE_STREAM_H

#include "vnd_haas_voice_stream.h"
#include "vnd_voice_fade_stream.h"

#ifdef __cplusplus
extern "C" {
#endif

vnd_status vnd_haas_voice_fade_stream_state_bytes(int64_t slots, int32_t in_channels, int32_t max_delay,
                                                  int64_t max_frames_per_call, int64_t fade_frames, int64_t *bytes);
vnd_status vnd_haas_voice_fade_stream_reset_dev(vnd_ctx *ctx, void *state_dev, int64_t state_bytes, int64_t slots,
                                                int32_t in_channels, int32_t max_delay, int64_t max_frames_per_call,
                                                int64_t fade_frames, void *hip_stream);
vnd_status vnd_haas_voice_fade_stream_f64_dev(vnd_ctx *ctx, void *state_dev, int64_t state_bytes,
                                              int64_t max_frames_per_call, int64_t fade_frames, const float *gains_dev,
                                              const float *x_dev, const int32_t *counts_dev, const int32_t *flags_dev,
                                              const int32_t *delays_dev, double *y_dev, int32_t *out_counts_dev,
                                              int32_t *fade_left_dev, int64_t slots, int32_t in_channels,
                                              int32_t max_delay, int32_t delayed_channel, int32_t ms_mode,
                                              int32_t use_width, double width, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* VND_HAAS_VOICE_FADE_STREAM_H */

/* vnd_spectrum_voice_stream.h - the short-time spectra of vnd_spectrum.h for a VOICE POOL, exported by libvnd_amd.so: the
 * spectrogram columns of vnd_spectrogram_*_dev and the Welch means of vnd_cross_spectra_*_dev, with the signal arriving block
 * by block, the position of every voice in the device state, one per slot, and a frame count and start / end flags per slot
 * and call, as vnd_voice_stream.h does it for the decorrelating pools.  It reads the rows and the out_counts of such a pool
 * straight from device memory, so "decorrelate, then meter the coherence" is one chain of launches with no host in it.  A
 * call is a pure function of device memory - no argument depends on the call's history - so it can be captured in a graph
 * and replayed.
 *
 * Same conventions as vnd_spectrum.h (plain C99, vnd_status, vnd_last_error, "*_dev" = device pointers and a hipStream_t
 * passed as void*).  The entries enqueue on hip_stream only: they allocate nothing, read no device memory from the host,
 * synchronise nothing and are graph-capturable.  Every argument is checked before anything is enqueued, with nothing
 * written: first the arguments (VND_ERR_INVALID, then VND_ERR_UNSUPPORTED), last the context (a null ctx is
 * VND_ERR_INVALID "null context"), so every refusal is reachable without a device.
 *
 * ---- one call, per slot b ---------------------------------------------------------------------------------------------
 * Read on the device: pos[b] from the state, counts[b] (int32, frames pushed for this slot in this call, 0..M, M =
 * max_frames_per_call) and flags[b] (int32, VND_VOICE_START and VND_VOICE_END of vnd_voice_stream.h; other bits are
 * ignored).  W = nperseg, H = hop.
 *     p  = START ? 0 : pos[b]                 START: whatever the slot held is dropped
 *     n  = counts[b]
 *     sc(q) = q >= W ? (q - W) / H + 1 : 0    (segments complete after q frames)
 *     w0 = sc(p),  w1 = sc(p + n)
 *     out_counts[b] = w1 - w0                 <= RC = ceil(M / H), the rows per call
 *     pos[b]        = END ? 0 : p + n         after the call
 * Segment t of a voice is its frames [t H, t H + W), as in vnd_spectrum.h.  Segments that never complete are dropped, so
 * END has no tail: it returns what this call's frames completed, reports the voice's final means and puts the position
 * back to 0.  START and END in one call are a whole voice in one block.  Why out_counts[b] <= RC: the proof of
 * vnd_correlogram_voice_stream.h, whose wc is this sc.
 * A BAD slot - counts[b] outside [0, M], or without START a stored position outside [0, 2^60] (a state that was never
 * reset) - answers out_counts[b] = -1: its rows, its means, its sums, its position and its ring are left alone and nothing
 * is indexed with the bad value; the other slots are unaffected.  It is the rule of vnd_voice_stream.h, so a -1 from a
 * decorrelating pool, handed on as a count, passes through the meter as -1.
 * An IDLE slot - n = 0 and neither flag - answers out_counts[b] = 0 and changes nothing else: its rows, means and segments
 * keep what they held.
 *
 * ---- chunk ------------------------------------------------------------------------------------------------------------
 * Sample t (0 <= t < counts[b]) of channel c of slot b is frames_dev[b * stream_stride + t * frame_stride + c], c <
 * channels (1 or 2), addressed as the pool of vnd_spectrum.h: a mono view of one channel of a stereo pool is channels = 1,
 * frame_stride = 2.  Only the first counts[b] frames of row b are read.  *_f32_dev takes float32, *_f64_dev float64, and
 * each computes in its own type as the one-shot entry of that type does: there is no cast.
 * window_dev, twiddles_dev, nperseg, hop, nfft, detrend and scale are those of vnd_spectrum.h, value for value.
 *
 * ---- outputs ----------------------------------------------------------------------------------------------------------
 * F = nfft / 2 + 1.  out_counts_dev: int32 [slots].
 * cols_dev: null, or [slots][RC][channels][F] of the sample type.  Row r < out_counts[b] of slot b holds the 'psd' column of
 * segment w0 + r of each channel; nothing at or past row out_counts[b] is written.  The layout is time-major, unlike
 * vnd_spectrogram_*_dev's [F][segments]: a row is complete when its call returns.
 * pxx_dev, pyy_dev: [slots][F]; pxy_dev: [slots][F][2] (re, im), of the sample type; segments_dev: int64 [slots].  Null as a
 * group (all four), or all given; with channels = 1 only pxx_dev and segments_dev are written, and pyy_dev and pxy_dev may
 * be null.  For every slot that is neither bad nor idle they hold, after the call, the Welch means over the segments [0, w1)
 * of the voice - what vnd_cross_spectra_*_dev returns for the frames pushed so far - and segments[b] = w1; zeros and 0 when
 * w1 = 0.  A call with END reports the voice's final means.
 *
 * Contract.  Take one voice: the calls from a START - or from position 0 after an END or a reset - up to the current one.
 * The concatenation of its rows equals vnd_spectrogram_{f32,f64}_dev on the concatenation of its frames, column for column
 * and bit for bit (a column is a function of its own segment alone), and after every call its means equal
 * vnd_cross_spectra_{f32,f64}_dev on the frames pushed so far, bit for bit, for every schedule of counts, idle calls and
 * neighbours.
 *
 * The order of the sums.  R = vnd_spectrum_run_length(nfft, nperseg, hop, is_float64, channels).  The one-shot call adds the
 * per-segment values of a bin in float64 from +0.0 in ascending t within runs of R consecutive segments, run j the segments
 * [j R, (j + 1) R); it adds the runs from +0.0 in ascending j, divides by the segment count and rounds once to the sample
 * type.  The pool keeps, per slot, bin and quantity (Pxx; and Pyy, re Pxy, im Pxy with two channels), two float64 values:
 *     total    the completed runs, added from +0.0 in ascending j
 *     partial  the run in progress, added from +0.0 in ascending t
 * A segment t with t % R == 0 starts partial again from +0.0, and the run before it, if there is one, has been folded by
 * then: total += partial, once, when its last segment (t % R == R - 1) was added.  The reported sum is total + partial when
 * w1 % R != 0, else total.  That is the one-shot order, whatever the calls' boundaries.
 *
 * ---- state ------------------------------------------------------------------------------------------------------------
 * `state_bytes` at least what vnd_spectrum_voice_stream_state_bytes returns, state_dev 16-byte aligned; Q = 1 for one
 * channel, 4 for two; G = ceil(RC / R) + 1, the runs a call can touch.  In this order, each part padded to a multiple of 16
 * bytes:
 *   1. positions: int64 [slots];
 *   2. sums:      float64 [slots][F][Q][2], (total, partial).  Logically zero at START and never cleared: partial is read
 *                 only when w0 % R != 0, total only when w0 >= R - both were then written by this voice;
 *   3. work:      float64 [slots][G][F][Q], the scratch between the two kernels of one call;
 *   4. ring:      per slot W - 1 + M frames x channels of the sample type, ring slot = the voice's absolute frame mod
 *                 (W - 1 + M).  A call reads only frames in [p - W + 1, p) from it and writes only the chunk's last
 *                 min(n, W - 1) frames, so no ring slot is both read and written in one call; a call with END writes
 *                 nothing.  Never cleared: a voice reads no frame below its own 0.
 * The positions must start at 0: vnd_spectrum_voice_stream_reset_dev enqueues one hipMemsetAsync over the positions ONLY
 * (it ends every voice).  A call reads and writes the state on the call's stream: calls of one pool run in order on one
 * hipStream_t (or are ordered by the caller).
 *
 * *_dev: enqueues two kernels on hip_stream only - the runs of the pool's new segments, then the fold of the runs, the means
 * and pos and out_counts - with a grid fixed by (slots, M, nperseg, hop, nfft, the sample type, channels) alone.
 *
 * ---- refusals ---------------------------------------------------------------------------------------------------------
 * VND_ERR_INVALID: a null pointer (cols_dev may be null; pxx_dev, pyy_dev, pxy_dev and segments_dev as a group; pyy_dev and
 * pxy_dev with one channel); slots, max_frames_per_call, a stride, nperseg - 1 or hop below 1; max_frames_per_call above
 * INT32_MAX (counts are int32); channels not 1 or 2, or above frame_stride; a scale that is NaN, or not positive and finite
 * in the sample type; a state_bytes below the query's answer or a state not 16-byte aligned; extents that overflow; outputs
 * overlapping one another, the state or any input, or the state overlapping an input.
 * VND_ERR_UNSUPPORTED: nfft not a power of two in [VND_SPECTRUM_MIN_NFFT, VND_SPECTRUM_MAX_NFFT]; nperseg above nfft; hop
 * above nperseg; slots above VND_MAX_STREAMS; G above 65535, or slots * G above 2^23 workgroups; a cols of more than 2^40
 * values (slots * RC * channels * F, whether or not cols_dev is given: a pool's limits do not depend on a call's
 * pointers).  Of the VND_ERR_INVALID checks, the state's size and alignment, the extents and the overlaps come after the
 * VND_ERR_UNSUPPORTED ones: they are defined for a supported shape only.                                                  */
#ifndef VND_SPECTRUM_VOICE_STREAM_H
#define VND_SPECTRUM_VOICE_STREAM_H

#include "vnd_spectrum.h"
#include "vnd_voice_stream.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The bytes of a pool's state.  No context.  *bytes is 0 on a refusal. */
vnd_status vnd_spectrum_voice_stream_state_bytes(int64_t slots, int32_t channels, int32_t nperseg, int32_t hop, int32_t nfft,
                                                 int64_t max_frames_per_call, int32_t is_float64, int64_t *bytes);
vnd_status vnd_spectrum_voice_stream_reset_dev(vnd_ctx *ctx, void *state_dev, int64_t state_bytes, int64_t slots,
                                               int32_t channels, int32_t nperseg, int32_t hop, int32_t nfft,
                                               int64_t max_frames_per_call, int32_t is_float64, void *hip_stream);
vnd_status vnd_spectrum_voice_stream_f32_dev(vnd_ctx *ctx, void *state_dev, int64_t state_bytes, int64_t max_frames_per_call,
                                             const float *frames_dev, int64_t stream_stride, int32_t frame_stride,
                                             int32_t channels, const int32_t *counts_dev, const int32_t *flags_dev,
                                             const float *window_dev, const float *twiddles_dev, int32_t nperseg, int32_t hop,
                                             int32_t nfft, int32_t detrend, double scale, float *cols_dev,
                                             int32_t *out_counts_dev, float *pxx_dev, float *pyy_dev, float *pxy_dev,
                                             int64_t *segments_dev, int64_t slots, void *hip_stream);
vnd_status vnd_spectrum_voice_stream_f64_dev(vnd_ctx *ctx, void *state_dev, int64_t state_bytes, int64_t max_frames_per_call,
                                             const double *frames_dev, int64_t stream_stride, int32_t frame_stride,
                                             int32_t channels, const int32_t *counts_dev, const int32_t *flags_dev,
                                             const double *window_dev, const double *twiddles_dev, int32_t nperseg,
                                             int32_t hop, int32_t nfft, int32_t detrend, double scale, double *cols_dev,
                                             int32_t *out_counts_dev, double *pxx_dev, double *pyy_dev, double *pxy_dev,
                                             int64_t *segments_dev, int64_t slots, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* VND_SPECTRUM_VOICE_STREAM_H */

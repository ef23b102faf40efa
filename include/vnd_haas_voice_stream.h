/* vnd_haas_voice_stream.h - a VOICE POOL of HaasEffect delays, exported by libvnd_amd.so: the Haas sibling of
 * vnd_voice_stream.h.  `slots` slots, each a voice with a life and a delay of its own: it is vnd_haas_each_stream_f64_*
 * (vnd_each_stream.h) with the stream position moved from the caller into the device state, one per slot, and with a
 * frame count and start / end flags per slot and call.  Voices join and leave at any call, bring blocks of any size or
 * none, and a slot is handed to a new voice with another delay without ending the pool.  A call is a pure function of
 * device memory - no argument depends on the call's history - so it can be captured in a graph and replayed.
 *
 * Same conventions as vnd_amd.h (plain C99, vnd_status, vnd_last_error, "*_dev" = device pointers and a hipStream_t
 * passed as void*), and kept out of it so that vnd_amd.h keeps its fixed set of functions.  Mono or stereo float32 in,
 * stereo FLOAT64 out, as every Haas entry.
 *
 * ---- one call, per slot b ---------------------------------------------------------------------------------------------
 * Read on the device: counts[b] (int32, frames pushed for this slot in this call, 0..M, M = max_frames_per_call),
 * flags[b] (int32, bit 0 VND_VOICE_START, bit 1 VND_VOICE_END of vnd_voice_stream.h; other bits are ignored) and
 * delays[b] (int32, the voice's delay in frames, 0..max_delay).  pos[b] is the slot's position in the state.
 *     p = START ? 0 : pos[b]                  START: whatever the slot held is discarded, unflushed
 *     n = counts[b]        d = delays[b]
 *     out_counts[b] = n + (END ? d : 0)       <= M + max_delay
 *     pos[b]        = END ? 0 : p + n         after the call
 * x is float32 [slots][M][in_channels]: only the first counts[b] frames of row b are read.  y is float64
 * [slots][M + max_delay][2]: the call writes the first out_counts[b] frames of row b and nothing at or past them.  Both
 * strides are fixed by the pool, so no shape depends on data.  out_counts is int32 [slots].
 * Output frame k of the call is the voice's absolute frame t = p + k.  The undelayed column reads input frame t, the
 * delayed column frame t - d: from the slot's ring for [p - d, p), from the chunk for [p, p + n), and as zero below 0 and
 * at or past p + n.  A voice's tail is its OWN d frames - the pool has a count per slot, so nothing is padded to
 * max_delay (vnd_haas_each_stream_f64_* pads, it has one n_out for the pool).
 * A slot with n = 0 and no flag does nothing and its position stays.  END with n = 0 flushes the d tail frames.  START
 * over a live voice drops it, unflushed.  START and END in one call are a whole voice in one block - one shorter than
 * its own delay included.
 *
 * Contract.  Take one voice: the calls from a START - or from position 0 after an END or a reset - up to and including
 * its END.  The concatenation of its outputs equals vnd_haas_f64_* (vnd_amd.h) on that voice's whole signal with
 * delay_frames = delays[b], n + d frames, bit for bit, for every schedule of counts, idle calls and neighbours.
 * delayed_channel, ms_mode, use_width and width are scalars of the call, as in vnd_haas_stream.h.
 *
 * Bad per-slot values (the other slots' bits are unchanged in every case): out_counts[b] = -1, row b of y, the
 * position and the ring are untouched, and nothing is indexed with the bad value, for
 *   - counts[b] outside [0, M];
 *   - a stored position outside [0, 2^60] (a state that was never reset), unless the call carries START;
 *   - delays[b] outside [0, max_delay] on a slot that has work (n > 0, START or END).
 * The last differs from the NaN rows that vnd_voice_stream.h answers a bad table with: there the table changes the
 * values of a row whose length is known; here a bad delay would also fix the LENGTH of the tail, so there is no row to
 * fill and the slot is left alone.  The delay of a slot is expected to change only with START; the C ABI does not
 * police this.
 *
 * ---- state ------------------------------------------------------------------------------------------------------------
 * `state_bytes` at least what vnd_haas_voice_stream_state_bytes returns, state_dev 16-byte aligned: first one int64
 * position per slot (padded to a multiple of 16 bytes), then the Haas ring of vnd_each_stream.h, capacity max_delay + M
 * frames of in_channels float32 per slot, ring slot = the voice's absolute frame mod capacity; with max_delay = 0 there
 * are the positions only.  A call reads ring frames in [p - max_delay, p) and writes the chunk's last min(n, max_delay)
 * frames, which lie in [p, p + n): less than one capacity apart, so no slot is both read and written in one call.  The
 * ring is never cleared and needs no clearing: a voice never reads a frame below its own position 0.  The positions must
 * start at 0: vnd_haas_voice_stream_reset_dev enqueues a hipMemsetAsync over the positions ONLY (it ends every voice,
 * unflushed).  A call reads and writes the state on the call's stream: calls of one pool run in order on one
 * hipStream_t (or are ordered by the caller).
 *
 * *_dev: every array is device memory.  Enqueues two kernels on hip_stream only - the pool's frames, then one lane per
 * slot that writes pos and out_counts - with a grid fixed by (slots, M, max_delay): no allocation, no synchronisation,
 * no read of device memory by the host, no other stream.  Capturable.
 * *_host: x, counts, flags, delays, y and out_counts in host memory, synchronous (the state stays in device memory).
 * counts and - for every slot with frames or a flag - delays are validated before anything is launched: one out of
 * range is VND_ERR_INVALID and the message names the slot.  The fixed-stride x goes up whole, and y goes up and comes
 * back whole, so that the rows at and past out_counts[b] keep the caller's bytes.
 * Checked before anything is enqueued, with nothing written: VND_ERR_INVALID for a null pointer, negative slots,
 * max_delay or max_frames_per_call, a state_bytes below the query's answer or a state not 16-byte aligned, in_channels
 * not in {1, 2}, delayed_channel not in {0, 1}; VND_ERR_UNSUPPORTED for slots above VND_MAX_STREAMS and for
 * M + max_delay above VND_HAAS_VOICE_MAX_ROW_FRAMES: the kernel has one lane per output frame and 256 lanes per
 * workgroup, and the workgroups of a row are one grid dimension of at most 65535, so a row holds at most
 * 65535 * 256 = 16776960 frames.  The call entries (not the query or the reset) also answer VND_ERR_UNSUPPORTED,
 * "problem too large", for a y of more than 2^40 values, slots * (M + max_delay) * 2, as the other stream entries do.  */
#ifndef VND_HAAS_VOICE_STREAM_H
#define VND_HAAS_VOICE_STREAM_H

#include "vnd_voice_stream.h"

#define VND_HAAS_VOICE_MAX_ROW_FRAMES 16776960

#ifdef __cplusplus
extern "C" {
#endif

vnd_status vnd_haas_voice_stream_state_bytes(int64_t slots, int32_t in_channels, int32_t max_delay,
                                             int64_t max_frames_per_call, int64_t *bytes);
vnd_status vnd_haas_voice_stream_reset_dev(vnd_ctx *ctx, void *state_dev, int64_t state_bytes, int64_t slots,
                                           int32_t in_channels, int32_t max_delay, int64_t max_frames_per_call,
                                           void *hip_stream);
vnd_status vnd_haas_voice_stream_f64_dev(vnd_ctx *ctx, void *state_dev, int64_t state_bytes, int64_t max_frames_per_call,
                                         const float *x_dev, const int32_t *counts_dev, const int32_t *flags_dev,
                                         const int32_t *delays_dev, double *y_dev, int32_t *out_counts_dev,
                                         int64_t slots, int32_t in_channels, int32_t max_delay, int32_t delayed_channel,
                                         int32_t ms_mode, int32_t use_width, double width, void *hip_stream);
vnd_status vnd_haas_voice_stream_f64_host(vnd_ctx *ctx, void *state_dev, int64_t state_bytes, int64_t max_frames_per_call,
                                          const float *x, const int32_t *counts, const int32_t *flags,
                                          const int32_t *delays, double *y, int32_t *out_counts, int64_t slots,
                                          int32_t in_channels, int32_t max_delay, int32_t delayed_channel,
                                          int32_t ms_mode, int32_t use_width, double width);

#ifdef __cplusplus
}
#endif
#endif /* VND_HAAS_VOICE_STREAM_H */

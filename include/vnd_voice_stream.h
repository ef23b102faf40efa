/* vnd_voice_stream.h - a VOICE POOL, exported by libvnd_amd.so: `slots` slots over a bank of velvet-noise filters, each
 * slot a voice with a life of its own.  It is vnd_each_stream_f32_* (vnd_each_stream.h) with the stream position moved
 * from the caller into the device state, one per slot, and with a frame count and start / end flags per slot and call:
 * voices join and leave at any call, bring 10 ms here and 20 ms there or nothing at all, and a slot is handed to a new
 * voice with another filter without ending the pool.  A call is a pure function of device memory - no argument depends
 * on the call's history - so it can be captured in a graph and replayed.
 *
 * Same conventions as vnd_amd.h (plain C99, vnd_status, vnd_last_error, "*_dev" = device pointers and a hipStream_t
 * passed as void*), and kept out of it so that vnd_amd.h keeps its fixed set of functions.  Exact mode only
 * (VND_MODE_EXACT), mono or stereo in, stereo out, no normaliser - as every stream.
 *
 * ---- one call, per slot b ---------------------------------------------------------------------------------------------
 * Read on the device: counts[b] (int32, frames pushed for this slot in this call, 0..M, M = max_frames_per_call),
 * flags[b] (int32, bit 0 VND_VOICE_START, bit 1 VND_VOICE_END; other bits are ignored) and tables[b] (int32, candidate
 * of the bank, as in vnd_each.h: candidate t owns channels 2t, 2t + 1).  H is the bank's largest tap index
 * (vnd_taps_info's max_index), the one latency of the pool.  pos[b] is the slot's position in the state.
 *     p  = START ? 0 : pos[b]                 START: whatever the slot held is discarded, unflushed
 *     n  = counts[b]
 *     E  = max(0, p - H)
 *     E' = END ? p + n : max(0, p + n - H)
 *     out_counts[b] = E' - E                  <= n + min(p, H) <= M + H
 *     pos[b]        = END ? 0 : p + n         after the call
 * x is float32 [slots][M][in_channels]: only the first counts[b] frames of row b are read.  y is float32
 * [slots][M + H][2]: the call writes the first out_counts[b] frames of row b and nothing at or past them.  Both strides
 * are fixed by the pool, so no shape depends on data.  out_counts is int32 [slots].
 * A slot with n = 0 and no flag does nothing and its position stays.  END with n = 0 flushes the tail, min(p, H) frames.
 * START and END in one call are a whole voice in one block.
 *
 * Contract.  Take one voice: the calls from a START - or from position 0 after an END or a reset - up to and including
 * its END.  The concatenation of its outputs equals vnd_decorrelate_each_f32_* without a normaliser (vnd_each.h) on that
 * voice's whole signal with its table alone, bit for bit, for every schedule of counts, idle calls and neighbours.
 * ms_encode / use_width, width: the decorrelate stage's pointwise steps, scalars of the call, as in vnd_stream.h.
 *
 * Bad per-slot values (the other slots are unaffected):
 *   - counts[b] outside [0, M]: out_counts[b] = -1, row b of y is untouched, position and ring are unchanged; nothing
 *     is indexed with the bad value.  The same answer is given for a slot whose stored position is not in [0, 2^60]
 *     (a state that was never reset) unless the call carries START.
 *   - tables[b] outside [0, T) on a slot that has work: that slot's out_counts[b] rows are NaN (the convention of
 *     vnd_each_stream.h); the position still advances.
 * The table of a slot is expected to change only with START; the C ABI does not police this.  (A live voice changes its
 * table, crossfaded, in the pool of vnd_voice_fade_stream.h.)
 *
 * ---- state ------------------------------------------------------------------------------------------------------------
 * `state_bytes` at least what vnd_voice_stream_state_bytes returns, state_dev 16-byte aligned: first one int64 position
 * per slot (padded to a multiple of 16 bytes), then the ring of vnd_each_stream.h, capacity H + M frames per slot,
 * ring slot = the voice's absolute frame mod capacity.  The ring is never cleared and needs no clearing: a voice never
 * reads a frame below its own position 0.  The positions must start at 0: vnd_voice_stream_reset_dev enqueues a
 * hipMemsetAsync over the positions ONLY (it ends every voice, unflushed).  A call reads and writes the state on the
 * call's stream: calls of one pool run in order on one hipStream_t (or are ordered by the caller).
 *
 * *_dev: every array is device memory.  Enqueues two kernels on hip_stream only - the pool's frames, then one lane per
 * slot that writes pos and out_counts - with a grid fixed by (slots, M, H): no allocation, no synchronisation, no read
 * of device memory by the host, no other stream.  Capturable.
 * *_host: x, counts, flags, tables, y and out_counts in host memory, synchronous (the state stays in device memory).
 * counts and - for every slot with frames or an END - tables are validated before anything is launched: one out of
 * range is VND_ERR_INVALID and the message names the slot.  The fixed-stride x goes up whole, and y goes up and comes
 * back whole, so that the rows at and past out_counts[b] keep the caller's bytes.
 * Checked before anything is enqueued, with nothing written: VND_ERR_INVALID for a null pointer, negative slots or
 * max_frames_per_call, a state_bytes below the query's answer or a state not 16-byte aligned, in_channels not in {1, 2},
 * a bank with an odd number of channels or on another device; VND_ERR_UNSUPPORTED for a mode other than VND_MODE_EXACT,
 * slots above VND_MAX_STREAMS, a bank whose largest tap index is above VND_VELVET_PAIRS_MAX_TAP_INDEX, a bank with a
 * weight that is not finite, and a max_frames_per_call above 2^24.                                                     */
#ifndef VND_VOICE_STREAM_H
#define VND_VOICE_STREAM_H

#include "vnd_each_stream.h"

#define VND_VOICE_START 1
#define VND_VOICE_END 2

#ifdef __cplusplus
extern "C" {
#endif

vnd_status vnd_voice_stream_state_bytes(const vnd_taps *bank, int64_t slots, int32_t in_channels,
                                        int64_t max_frames_per_call, int64_t *bytes);
vnd_status vnd_voice_stream_reset_dev(vnd_ctx *ctx, void *state_dev, int64_t state_bytes, int64_t slots,
                                      int32_t in_channels, const vnd_taps *bank, int64_t max_frames_per_call,
                                      void *hip_stream);
vnd_status vnd_voice_stream_f32_dev(vnd_ctx *ctx, const vnd_taps *bank, void *state_dev, int64_t state_bytes,
                                    int64_t max_frames_per_call, const float *x_dev, const int32_t *counts_dev,
                                    const int32_t *flags_dev, const int32_t *tables_dev, float *y_dev,
                                    int32_t *out_counts_dev, int64_t slots, int32_t in_channels, int32_t mode,
                                    int32_t ms_encode, int32_t use_width, double width, void *hip_stream);
vnd_status vnd_voice_stream_f32_host(vnd_ctx *ctx, const vnd_taps *bank, void *state_dev, int64_t state_bytes,
                                     int64_t max_frames_per_call, const float *x, const int32_t *counts,
                                     const int32_t *flags, const int32_t *tables, float *y, int32_t *out_counts,
                                     int64_t slots, int32_t in_channels, int32_t mode, int32_t ms_encode,
                                     int32_t use_width, double width);

#ifdef __cplusplus
}
#endif
#endif /* VND_VOICE_STREAM_H */

/* vnd_each_stream.h - a pool streamed block by block with its OWN filter or delay per stream, exported by
 * libvnd_amd.so: stream b of a pool runs through candidate tables[b] of a bank (velvet noise) or is delayed by delays[b]
 * frames (HaasEffect), one kernel launch per call for the whole pool - the streaming side of vnd_each.h, and the last
 * step of optimise per signal (vnd_velvet_search.h, vnd_haas_search.h), apply per signal, stream per signal.
 *
 * Same conventions as vnd_amd.h (plain C99, vnd_status, vnd_last_error, "*_dev" = device pointers and a hipStream_t
 * passed as void*), and kept out of it so that vnd_amd.h keeps its fixed set of functions.
 *
 * ---- velvet noise -------------------------------------------------------------------------------------------------
 * `bank` is a tap table of 2*T channels: candidate t owns channels 2t (left) and 2t + 1 (right), as in vnd_each.h.
 * The pool advances in lockstep at ONE latency H, the bank's largest tap index (vnd_taps_info's max_index): a stream
 * whose own filter is shorter waits with the others.  The caller holds `position`, the frames pushed per stream before
 * the call; a call pushes n_in more and returns the outputs that became final, as in vnd_stream.h:
 *     E  = max(0, position - H)                                    first output frame of the call
 *     E' = final ? position + n_in : max(0, position + n_in - H)   one past its last
 * *n_out = E' - E, computed on the host from these values alone, before anything is enqueued.  x is float32
 * [batch][n_in][in_channels] (in_channels 1: mono, fanned out to both outputs; 2: stereo), tables int32 [batch], y
 * float32 [batch][*n_out][2].  For every stream b the concatenation of every call's outputs, up to and including the one
 * with final = 1, equals row b of vnd_decorrelate_each_f32_* without a normaliser on the whole signals (vnd_each.h) - and
 * so vnd_decorrelate_f32_* of signal b alone with a table that holds candidate tables[b] alone - bit for bit, for every
 * schedule of calls.  n_in may change from call to call (0 included) up to max_frames_per_call.  After a final call the
 * state starts again at position 0.  Only VND_MODE_EXACT; there is no normaliser: a stream has not seen the whole signal.
 * ms_encode / use_width, width: the decorrelate stage's pointwise steps, scalars of the call, as in vnd_stream.h.
 *
 * State: a per-stream ring of the last input frames in device memory, `state_bytes` at least what
 * vnd_each_stream_state_bytes returns: capacity H + max_frames_per_call frames per stream, slot = absolute frame mod
 * capacity.  Its contents before position 0 are never read, so it needs no clearing.  A call copies the chunk's last
 * min(n_in, H) frames into it; a frame f it reads from the ring and a frame g it writes have
 * 0 < g - f <= H + n_in - 1 < capacity, so each call writes a ring slot at most once and never one it reads.  A call
 * reads and writes the state on the call's stream: calls of one pool run in order on one hipStream_t (or are ordered by
 * the caller).
 *
 * *_dev: tables, state, x and y are device memory; enqueues on hip_stream only: no allocation, no synchronisation, no
 * other stream.  tables is only read on the device: an entry outside [0, T) fills that stream's output rows of the call
 * with NaN from a bounds check in the kernel; nothing is indexed with it and the other streams are unaffected.
 * `position` is a kernel argument, so a captured graph would replay one call's position: do not capture it.
 * *_host: tables, x and y in host memory, synchronous (the state stays in device memory; work the caller enqueued on it
 * elsewhere must be complete).  Every entry of tables is validated before anything is launched: one out of range is
 * VND_ERR_INVALID, and the message names the stream.
 * Checked before anything is enqueued, with nothing written: VND_ERR_INVALID for a null pointer that the call would
 * use, negative counts or position, n_in > max_frames_per_call, a state_bytes below the query's answer, in_channels not
 * in {1, 2}, a bank with an odd number of channels or on another device; VND_ERR_UNSUPPORTED for a mode other than
 * VND_MODE_EXACT, batch above VND_MAX_STREAMS, a bank whose largest tap index is above VND_VELVET_PAIRS_MAX_TAP_INDEX,
 * and a bank with a weight that is not finite.
 *
 * ---- HaasEffect ---------------------------------------------------------------------------------------------------
 * vnd_haas_stream_f64_* (vnd_haas_stream.h) with a delay per stream, delays int32 [batch], each in [0, max_delay].  The
 * delay is causal: a call returns the n_in frames it pushed, and the final call max_delay frames more, so
 * *n_out = n_in + (final ? max_delay : 0), y FLOAT64 [batch][*n_out][2].  With n frames pushed in all, the first
 * n + delays[b] frames of stream b's concatenation are vnd_haas_f64_*'s for delay_frames = delays[b], bit for bit; the
 * remaining max_delay - delays[b] are written as +0.0 (the padded block of vnd_haas_each_f64_*).  delayed_channel,
 * ms_mode, use_width and width are scalars of the call.
 * State: a ring of max_delay + max_frames_per_call frames per stream (none for max_delay 0).  A call copies the chunk's
 * last min(n_in, max_delay) frames into it, so the frames [position - max_delay, position) are there for every stream's
 * own delay; read and written frames are less than the capacity apart, as above with H = max_delay, and a frame below 0
 * is never loaded.
 * *_dev: delays is only read on the device: an entry outside [0, max_delay] fills that stream's output rows of the call
 * with NaN from a bounds check in the kernel; the other streams are unaffected.  Not graph-capturable, as above.
 * *_host: a delay outside [0, max_delay] is VND_ERR_INVALID, the message names the stream, nothing is written.
 * VND_ERR_INVALID for a null pointer that the call would use, negative counts, position or max_delay,
 * n_in > max_frames_per_call, a small state, in_channels not in {1, 2}, delayed_channel not in {0, 1};
 * VND_ERR_UNSUPPORTED for batch above VND_MAX_STREAMS.                                                                */
#ifndef VND_EACH_STREAM_H
#define VND_EACH_STREAM_H

#include "vnd_each.h"
#include "vnd_stream.h"

#ifdef __cplusplus
extern "C" {
#endif

vnd_status vnd_each_stream_state_bytes(const vnd_taps *bank, int64_t batch, int32_t in_channels,
                                       int64_t max_frames_per_call, int64_t *bytes);
vnd_status vnd_each_stream_f32_dev(vnd_ctx *ctx, const vnd_taps *bank, const int32_t *tables_dev, void *state_dev,
                                   int64_t state_bytes, int64_t max_frames_per_call, const float *x_dev, float *y_dev,
                                   int64_t batch, int64_t position, int64_t n_in, int32_t in_channels, int32_t final,
                                   int32_t mode, int32_t ms_encode, int32_t use_width, double width, int64_t *n_out,
                                   void *hip_stream);
vnd_status vnd_each_stream_f32_host(vnd_ctx *ctx, const vnd_taps *bank, const int32_t *tables, void *state_dev,
                                    int64_t state_bytes, int64_t max_frames_per_call, const float *x, float *y,
                                    int64_t batch, int64_t position, int64_t n_in, int32_t in_channels, int32_t final,
                                    int32_t mode, int32_t ms_encode, int32_t use_width, double width, int64_t *n_out);

vnd_status vnd_haas_each_stream_state_bytes(int64_t batch, int32_t in_channels, int32_t max_delay,
                                            int64_t max_frames_per_call, int64_t *bytes);
vnd_status vnd_haas_each_stream_f64_dev(vnd_ctx *ctx, void *state_dev, int64_t state_bytes, int64_t max_frames_per_call,
                                        const float *x_dev, double *y_dev, int64_t batch, int64_t position, int64_t n_in,
                                        int32_t in_channels, int32_t final, const int32_t *delays_dev, int32_t max_delay,
                                        int32_t delayed_channel, int32_t ms_mode, int32_t use_width, double width,
                                        int64_t *n_out, void *hip_stream);
vnd_status vnd_haas_each_stream_f64_host(vnd_ctx *ctx, void *state_dev, int64_t state_bytes, int64_t max_frames_per_call,
                                         const float *x, double *y, int64_t batch, int64_t position, int64_t n_in,
                                         int32_t in_channels, int32_t final, const int32_t *delays, int32_t max_delay,
                                         int32_t delayed_channel, int32_t ms_mode, int32_t use_width, double width,
                                         int64_t *n_out);

#ifdef __cplusplus
}
#endif
#endif /* VND_EACH_STREAM_H */

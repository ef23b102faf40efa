/* vnd_haas_stream.h - chunked streaming of the HaasEffect delay, exported by libvnd_amd.so.
 *
 * Same conventions as vnd_stream.h (plain C99, vnd_status, vnd_last_error, "*_dev" = device pointers and a hipStream_t
 * passed as void*), and kept out of vnd_amd.h and vnd_stream.h so that both keep their fixed sets of functions.
 *
 * HaasEffect delays one column - of the left / right pair, or of the mid / side pair in MS mode - by d = delay_frames:
 * output frame t reads input frame t for the undelayed column and t - d for the delayed one.  The delay is causal, so a
 * stream has no latency.  A pool of `batch` streams advances in lockstep; the caller holds `position`, the frames pushed
 * per stream before the call; a call pushes n_in more and returns output frames [E, E'):
 *     E  = position
 *     E' = position + n_in + (final ? d : 0)
 * *n_out = E' - E.  Frames below 0 read as zeros (the zero tail that np.roll wraps to the front); in the d tail frames of
 * the final call the undelayed column reads zeros (the reference's zero-padded (n + d, 2) buffer).  The concatenation of
 * every call's outputs, up to and including the one with final = 1, is n + d frames and equals vnd_haas_f64_* on the whole
 * signal bit for bit: every output frame is the same float64 operation sequence.  n_in may change from call to call
 * (0 included) up to max_frames_per_call.  After a final call the state starts again at position 0.
 *
 * State: a per-stream ring of the last d input frames (raw float32, in_channels per frame) in device memory, `state_bytes`
 * at least what vnd_haas_stream_state_bytes returns; its contents before position 0 are never read, so it needs no
 * clearing.  With d = 0 the size is 0 and the state pointer may be null.  A call reads and writes it on the call's
 * stream: calls of one stream run in order on one hipStream_t (or are ordered by the caller).
 *
 * x float32 [batch][n_in][in_channels] (in_channels 1: a mono signal, read by both columns; 2: stereo), y float64
 * [batch][*n_out][2].  delayed_channel 0 | 1; ms_mode: the mid / side layout (LayoutMode.MS); use_width, width: the
 * stereo width applied to the output.
 * vnd_haas_stream_f64_dev: device memory; enqueues on hip_stream only: no allocation, no synchronisation, no other
 * stream.  `position` is a kernel argument, so a captured graph would replay one call's position: do not capture it.
 * vnd_haas_stream_f64_host: the same with x and y in host memory, synchronous (the state stays in device memory; work
 * the caller enqueued on it elsewhere must be complete).
 * VND_ERR_INVALID, checked before anything is enqueued and with nothing written, for: n_in > max_frames_per_call; a
 * state_bytes below what vnd_haas_stream_state_bytes returns; a batch above VND_MAX_STREAMS; in_channels other than 1
 * or 2; delayed_channel other than 0 or 1; negative counts, delay or position; a null pointer that the call would use. */
#ifndef VND_HAAS_STREAM_H
#define VND_HAAS_STREAM_H

#include "vnd_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

vnd_status vnd_haas_stream_state_bytes(int64_t batch, int32_t in_channels, int32_t delay_frames,
                                       int64_t max_frames_per_call, int64_t *bytes);
vnd_status vnd_haas_stream_f64_dev(vnd_ctx *ctx, void *state_dev, int64_t state_bytes, int64_t max_frames_per_call,
                                   const float *x_dev, double *y_dev, int64_t batch, int64_t position, int64_t n_in,
                                   int32_t in_channels, int32_t final, int32_t delay_frames, int32_t delayed_channel,
                                   int32_t ms_mode, int32_t use_width, double width, int64_t *n_out, void *hip_stream);
vnd_status vnd_haas_stream_f64_host(vnd_ctx *ctx, void *state_dev, int64_t state_bytes, int64_t max_frames_per_call,
                                    const float *x, double *y, int64_t batch, int64_t position, int64_t n_in,
                                    int32_t in_channels, int32_t final, int32_t delay_frames, int32_t delayed_channel,
                                    int32_t ms_mode, int32_t use_width, double width, int64_t *n_out);

#ifdef __cplusplus
}
#endif
#endif /* VND_HAAS_STREAM_H */

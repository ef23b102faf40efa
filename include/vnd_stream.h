/* vnd_stream.h - chunked streaming of the velvet-noise tap sum, exported by libvnd_amd.so.
 *
 * Same conventions as vnd_amd.h (plain C99, vnd_status, vnd_last_error, "*_dev" = device pointers and a hipStream_t
 * passed as void*), and kept out of it so that vnd_amd.h keeps its fixed set of functions.
 *
 * The tap sum is anti-causal, y[n][c] = sum_k w[c][k] * x[n + i[c][k]][c % in_channels], so output frame n is final
 * once input frame n + H has arrived (H = the table's largest tap index, vnd_taps_info's max_index): a stream has a
 * fixed latency of H frames.  A pool of `batch` streams advances in lockstep.  The caller holds `position`, the frames
 * pushed per stream before the call; a call pushes n_in more and returns the outputs that became final:
 *     E  = max(0, position - H)                                    first output frame of the call
 *     E' = final ? position + n_in : max(0, position + n_in - H)   one past its last
 * *n_out = E' - E, computed on the host from these values alone.  The concatenation of every call's outputs, up to and
 * including the one with final = 1, equals the one-shot vnd_convolve_f32_* / vnd_convolve_fanout_f32_* call on the whole
 * signal, bit for bit in VND_MODE_EXACT and VND_MODE_FMA; VND_MODE_FAST is within its tolerance of it (its summation
 * order follows the call's tiles) and bit-identical from run to run of the same schedule.  n_in may change from call to
 * call (0 included) up to max_frames_per_call.  After a final call the state starts again at position 0.
 *
 * State: a per-stream ring of the last input frames in device memory, `state_bytes` at least what
 * vnd_stream_state_bytes returns for the table, batch, in_channels and max_frames_per_call.  The caller allocates it
 * and keeps it for the life of the stream; its contents before position 0 are never read, so it needs no clearing.
 * A call reads and writes it on the call's stream: calls of one stream run in order on one hipStream_t (or are
 * ordered by the caller).  Each call writes a ring slot at most once and never one it reads.
 *
 * ms_encode / use_width, width: the decorrelate stage's pointwise steps (side-channel encode of a stereo - or mono,
 * fanned out - input, stereo width, in the reference's float32 operation order), for tables of 2 channels.
 *
 * vnd_stream_f32_dev: x float32 [batch][n_in][in_channels], y float32 [batch][*n_out][C], both device memory;
 * enqueues on hip_stream only: no allocation, no synchronisation, no other stream.  `position` is a kernel argument,
 * so a captured graph would replay one call's position: do not capture it.
 * vnd_stream_f32_host: the same with x and y in host memory, synchronous (the state stays in device memory; work the
 * caller enqueued on it elsewhere must be complete).
 * VND_ERR_INVALID, checked before anything is enqueued and with nothing written, for: n_in > max_frames_per_call; a
 * state_bytes below what vnd_stream_state_bytes returns; a batch above VND_MAX_STREAMS; in_channels that do not divide
 * the table's channel count; ms_encode or use_width with other than 2 output channels; negative counts or position; an
 * unknown mode; a null pointer that the call would use.                                                                 */
#ifndef VND_STREAM_H
#define VND_STREAM_H

#include "vnd_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

vnd_status vnd_stream_state_bytes(const vnd_taps *taps, int64_t batch, int32_t in_channels,
                                  int64_t max_frames_per_call, int64_t *bytes);
vnd_status vnd_stream_f32_dev(vnd_ctx *ctx, const vnd_taps *taps, void *state_dev, int64_t state_bytes,
                              int64_t max_frames_per_call, const float *x_dev, float *y_dev, int64_t batch,
                              int64_t position, int64_t n_in, int32_t in_channels, int32_t final, int32_t mode,
                              int32_t ms_encode, int32_t use_width, double width, int64_t *n_out, void *hip_stream);
vnd_status vnd_stream_f32_host(vnd_ctx *ctx, const vnd_taps *taps, void *state_dev, int64_t state_bytes,
                               int64_t max_frames_per_call, const float *x, float *y, int64_t batch,
                               int64_t position, int64_t n_in, int32_t in_channels, int32_t final, int32_t mode,
                               int32_t ms_encode, int32_t use_width, double width, int64_t *n_out);

#ifdef __cplusplus
}
#endif
#endif /* VND_STREAM_H */

/* vnd_correlogram_stream.h - the cross-correlogram of vnd_correlogram_f32_dev (vnd_analysis.h), streamed block by block,
 * exported by libvnd_amd.so.
 *
 * Same conventions as vnd_analysis.h (plain C99, vnd_status, vnd_last_error, "*_dev" = device pointers and a hipStream_t
 * passed as void*), and kept out of vnd_amd.h and vnd_analysis.h so that both keep their fixed sets of functions.
 *
 * Each window of W = window frames at hop H is independent: window w covers frames [w H, w H + W) and is final once frame
 * w H + W - 1 has arrived.  Windows that never complete are dropped, as in the reference, so a stream has no tail.  A pool
 * of `batch` streams advances in lockstep; the caller holds `position`, the frames pushed per stream before the call; a
 * call pushes n_in more and writes the rows of the windows that became final:
 *     wc(p) = p >= W ? (p - W) / H + 1 : 0          (windows complete after p frames)
 *     rows [wc(position), wc(position + n_in)),     *n_rows = wc(position + n_in) - wc(position)
 * computed on the host from these values alone, into out float32 [batch][*n_rows][num_lags], C-contiguous.  Each row is
 * what vnd_correlogram_f32_dev writes for that window, under the same contract (the column map, the float64 sums, the
 * float32 normaliser, silent and overflowing windows 0), and the concatenation of every call's rows is equal bit for bit
 * to vnd_correlogram_f32_dev on the whole signal.  n_in may change from call to call (0 included) up to
 * max_frames_per_call.  To start a new signal, call again with position 0.
 *
 * State: per stream, a ring of (x, y) float32 pairs, capacity W - 1 + max_frames_per_call frames, slot = absolute frame mod
 * capacity, in device memory of at least vnd_correlogram_stream_state_bytes = batch * capacity * 8 bytes.  A call reads
 * frames below `position` from the ring and frames from `position` on from the caller's chunk, and copies the chunk's last
 * min(n_in, W - 1) frames into the ring in the same launch.  Its contents before frame 0 are never read, so it needs no
 * clearing.  A call reads and writes it on the call's stream: calls of one stream run in order on one hipStream_t (or are
 * ordered by the caller).
 *
 * Chunk: frame t (0 <= t < n_in) of stream b at x_dev[b * stream_stride + t * frame_stride], y_dev likewise (x_dev and
 * y_dev may alias: channels 0 and 1 of one (batch, n_in, 2) block, frame_stride 2).  The chunk is read only by the call.
 * vnd_correlogram_stream_f32_dev enqueues on hip_stream only: no allocation, no synchronisation, no other stream.  A call
 * with n_in > 0 is one launch (more only past VND_MAX_STREAMS streams or 2^23 workgroups), even when no window completes;
 * a call with n_in = 0 launches nothing.  `position` is a kernel argument, so a captured graph would replay one call's
 * position: do not capture it.
 * VND_ERR_INVALID, checked before anything is enqueued and with nothing written, for: a state_bytes below
 * vnd_correlogram_stream_state_bytes; n_in > max_frames_per_call; a negative position or n_in; batch, strides, window,
 * hop, num_lags or max_frames_per_call below 1; a null context, n_rows, or state, chunk or output pointer the call would
 * use; out overlapping the chunk or the state, or the state overlapping the chunk; extents that overflow.
 * window > VND_CORRELOGRAM_MAX_WINDOW is VND_ERR_UNSUPPORTED. */
#ifndef VND_CORRELOGRAM_STREAM_H
#define VND_CORRELOGRAM_STREAM_H

#include "vnd_analysis.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The state one call needs: batch * (window - 1 + max_frames_per_call) * 8 bytes.  No context.  VND_ERR_INVALID for
 * batch, window or max_frames_per_call below 1, or a size that overflows; VND_ERR_UNSUPPORTED for a window above
 * VND_CORRELOGRAM_MAX_WINDOW. */
vnd_status vnd_correlogram_stream_state_bytes(int64_t batch, int32_t window, int64_t max_frames_per_call, int64_t *bytes);
vnd_status vnd_correlogram_stream_f32_dev(vnd_ctx *ctx, void *state_dev, int64_t state_bytes,
                                          int64_t max_frames_per_call, const float *x_dev, const float *y_dev,
                                          int64_t stream_stride, int32_t frame_stride, float *out_dev, int64_t batch,
                                          int64_t position, int64_t n_in, int32_t window, int32_t hop, int32_t num_lags,
                                          float eps, int64_t *n_rows, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* VND_CORRELOGRAM_STREAM_H */

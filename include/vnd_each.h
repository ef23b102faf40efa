/* vnd_each.h - per-signal entry points of libvnd_amd.so: signal b of a pool goes through its OWN filter of a bank
 * (velvet noise) or its own delay (HaasEffect), in one launch chain for the whole pool - the application side of the
 * batched optimisers (vnd_velvet_search.h, vnd_haas_search.h), which return one kappa or one delay per signal.
 *
 * Same conventions as vnd_amd.h (plain C99, vnd_status, vnd_last_error, "*_dev" = device pointers and a hipStream_t
 * passed as void*), exported by the same library, and kept out of vnd_amd.h so that it keeps its fixed set of
 * functions.
 */
#ifndef VND_EACH_H
#define VND_EACH_H

#include "vnd_amd.h"
#include "vnd_velvet_search.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- velvet noise: signal b through candidate tables[b] of a bank --------------------------------------------------
 * `bank` is a tap table of 2*T channels: candidate t owns channels 2t (left) and 2t + 1 (right), as in
 * vnd_velvet_pairs_f32_*.  Class-path tables (segments, gains, pass-through flags) and function-path tables are both
 * taken.  x is float32 [batch][n_frames][in_channels] (in_channels 1: mono, fanned out to both outputs; 2: stereo),
 * tables int32 [batch], y float32 [batch][n_frames][2].
 *
 * vnd_convolve_each_f32_*: row b of y is the convolution of signal b with candidate tables[b].
 * vnd_decorrelate_each_f32_*: the whole decorrelate stage behind it - side-channel encode (ms_encode), stereo width
 * (use_width, width) and the RMS normaliser (normalize: VND_NORMALIZE_*, eps), as vnd_decorrelate_f32_* applies them.
 * The stage settings are scalars of the call, the same for every signal.  The workspace is the one
 * vnd_decorrelate_workspace_bytes(batch, n_frames, 2) sizes (needed with a normaliser only).
 *
 * Numerics: only VND_MODE_EXACT.  Row b of vnd_convolve_each is bit-identical to vnd_convolve_f32_* (mono:
 * vnd_convolve_fanout_f32_*) of signal b alone with a table that holds candidate tables[b] alone; row b of
 * vnd_decorrelate_each to vnd_decorrelate_f32_* of signal b alone, normaliser included.  A row depends only on its
 * signal's samples, n_frames, in_channels, its candidate's taps, segments, gains and flags and the stage scalars: not
 * on the candidate's place in the bank or the other candidates, not on the other signals or how a pool is split into
 * calls, and not on the signal's index.  Non-finite samples are outside the contract.
 *
 * *_dev: x, tables, y and workspace are device memory.  tables is only read on the device: an entry outside [0, T)
 * fills that signal's row with NaN from a bounds check in the kernel; nothing out of range is accessed and the other
 * rows are unaffected.  Checked before anything is launched: VND_ERR_INVALID for a null context, bank or pointer,
 * negative counts, in_channels not in {1, 2}, a bank with an odd number of channels or on another device, x and y
 * that overlap, or (with a normaliser) a workspace smaller than the query's answer; VND_ERR_UNSUPPORTED for a mode
 * other than VND_MODE_EXACT, batch above VND_MAX_STREAMS, a bank whose largest tap index is above
 * VND_VELVET_PAIRS_MAX_TAP_INDEX, and a bank with a weight that is not finite.  Enqueues on hip_stream only:
 * allocates nothing, graph-capturable, thread-safe.
 * *_host: the same from host memory, synchronous.  Every entry of tables is validated before anything is launched:
 * one out of range is VND_ERR_INVALID, and the message names the signal.                                           */
vnd_status vnd_convolve_each_f32_dev(vnd_ctx *ctx, const vnd_taps *bank, const float *x_dev, const int32_t *tables_dev,
                                     float *y_dev, int32_t batch, int64_t n_frames, int32_t in_channels, int32_t mode,
                                     void *hip_stream);
vnd_status vnd_convolve_each_f32_host(vnd_ctx *ctx, const vnd_taps *bank, const float *x, const int32_t *tables,
                                      float *y, int32_t batch, int64_t n_frames, int32_t in_channels, int32_t mode);
vnd_status vnd_decorrelate_each_f32_dev(vnd_ctx *ctx, const vnd_taps *bank, const float *x_dev,
                                        const int32_t *tables_dev, float *y_dev, int32_t batch, int64_t n_frames,
                                        int32_t in_channels, int32_t mode, int32_t ms_encode, int32_t use_width,
                                        double width, int32_t normalize, float eps, void *workspace_dev,
                                        int64_t workspace_bytes, void *hip_stream);
vnd_status vnd_decorrelate_each_f32_host(vnd_ctx *ctx, const vnd_taps *bank, const float *x, const int32_t *tables,
                                         float *y, int32_t batch, int64_t n_frames, int32_t in_channels, int32_t mode,
                                         int32_t ms_encode, int32_t use_width, double width, int32_t normalize,
                                         float eps);

/* ---- HaasEffect: signal b delayed by delays[b] frames --------------------------------------------------------------
 * vnd_haas_f64_* with a delay per signal: x float32 [batch][n_frames][in_channels], delays int32 [batch], y FLOAT64
 * [batch][n_frames + max_delay][2] - one padded block, row stride n_frames + max_delay frames.  Rows
 * [0, n_frames + delays[b]) of signal b are vnd_haas_f64_*'s for delay_frames = delays[b], bit for bit; rows
 * [n_frames + delays[b], n_frames + max_delay) are written as zeros.  delayed_channel, ms_mode, use_width and width
 * are scalars of the call.
 * *_dev: delays is only read on the device: an entry outside [0, max_delay] fills that signal's rows with NaN from a
 * bounds check in the kernel; the other signals are unaffected.  VND_ERR_INVALID for a null context or pointer,
 * negative counts or max_delay, in_channels not in {1, 2}, delayed_channel not in {0, 1}; VND_ERR_UNSUPPORTED for
 * batch above VND_MAX_STREAMS.  Enqueues on hip_stream only: allocates nothing, graph-capturable, thread-safe.
 * *_host: the same from host memory, synchronous; a delay outside [0, max_delay] is VND_ERR_INVALID, and the message
 * names the signal.                                                                                                 */
vnd_status vnd_haas_each_f64_dev(vnd_ctx *ctx, const float *x_dev, double *y_dev, int64_t batch, int64_t n_frames,
                                 int32_t in_channels, const int32_t *delays_dev, int32_t max_delay,
                                 int32_t delayed_channel, int32_t ms_mode, int32_t use_width, double width,
                                 void *hip_stream);
vnd_status vnd_haas_each_f64_host(vnd_ctx *ctx, const float *x, double *y, int64_t batch, int64_t n_frames,
                                  int32_t in_channels, const int32_t *delays, int32_t max_delay,
                                  int32_t delayed_channel, int32_t ms_mode, int32_t use_width, double width);

#ifdef __cplusplus
}
#endif
#endif /* VND_EACH_H */

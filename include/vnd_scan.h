/* vnd_scan.h - optimiser scan entry points of libvnd_amd.so: score many candidate decorrelators of one signal at once.
 *
 * Same conventions as vnd_amd.h (plain C99, vnd_status, vnd_last_error, "*_dev" = device pointers and a hipStream_t
 * passed as void*), exported by the same library, and kept out of vnd_amd.h and vnd_analysis.h so that those
 * headers keep their fixed sets of functions.
 */
#ifndef VND_SCAN_H
#define VND_SCAN_H

#include "vnd_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Delays one vnd_haas_scan_f64_* call takes at most (split larger scans). */
#define VND_HAAS_SCAN_MAX_DELAYS 1048560

/* ---- Haas-delay scan (optimization.py:107-117 over HaasEffect candidates, as :158-227 builds them) ----------------
 * For one float32 signal x[n_frames][in_channels] (in_channels 1: mono, duplicated as the reference does; 2: stereo)
 * and F = n_delays integer delays d_f >= 0, all under one HaasEffect configuration (delayed_channel 0 | 1, ms = MS
 * layout, use_width / width = apply_stereo_width), moments[f] are the eight float64 quantities of the velvet-noise
 * scan (vnd_scan_bank_f32_host), in its order, over all n_frames + d_f frames (L, R) of
 * HaasEffect(delay d_f).decorrelate(x):
 *   { sum r, sum r*t, sum r*t^2, sum r*t^3, max |t|, sum L*R, sum L^2, sum R^2 },
 *   t = atan2(L - R, L + R) folded onto [-pi/2, pi/2], r = sqrt(L^2 + R^2).
 * Numerics: each frame is bit-identical to the reference's float64 frame (the float64 operations of
 * vnd_haas_f64_dev); t, r and every product are float64, the fold uses float64 pi; atan2 follows NumPy's signed-zero
 * rules, so a silent frame has t = +-0 and adds 0 to every moment.  The device atan2 may differ from the host's in the
 * last bit.  Every sum is float64 in a fixed order that depends only on n_frames and d_f: results are bit-identical
 * across runs, across the other delays of a call and across how the delays are split into calls.  Against NumPy's
 * pairwise float64 sums a moment differs by summation rounding only.  Delays in ascending order run fastest (a
 * workgroup stages the history window of 16 consecutive delays once); any order gives the same results.
 * Non-finite samples are outside the contract.
 *
 * vnd_haas_scan_workspace_bytes: the workspace vnd_haas_scan_f64_dev needs for n_delays delays of at most max_delay
 * frames; VND_ERR_INVALID for negative arguments.
 * vnd_haas_scan_f64_dev: x float32, delays int32 [n_delays], moments float64 [n_delays][8] and workspace_bytes of
 * workspace, all device memory.  The delays are only read on the device: a delay that is negative, or above the
 * max_delay the workspace was sized for, gives that candidate a row of NaN.  VND_ERR_INVALID, checked before anything
 * is launched, for n_frames < 0, n_delays < 0, in_channels not in {1, 2}, delayed_channel not in {0, 1}, a negative
 * workspace_bytes or a null pointer; VND_ERR_UNSUPPORTED above VND_HAAS_SCAN_MAX_DELAYS delays.  Enqueues on
 * hip_stream only: allocates nothing, graph-capturable, thread-safe.
 * vnd_haas_scan_f64_host: the same from host memory (x float32, delays int32, moments float64), synchronous; a
 * negative delay is VND_ERR_INVALID, checked before anything is launched.                                           */
vnd_status vnd_haas_scan_workspace_bytes(int64_t n_frames, int32_t n_delays, int32_t max_delay, int64_t *bytes);
vnd_status vnd_haas_scan_f64_dev(vnd_ctx *ctx, const float *x_dev, int64_t n_frames, int32_t in_channels,
                                 const int32_t *delays_dev, int32_t n_delays, int32_t delayed_channel, int32_t ms,
                                 int32_t use_width, double width, double *moments_dev, void *workspace_dev,
                                 int64_t workspace_bytes, void *hip_stream);
vnd_status vnd_haas_scan_f64_host(vnd_ctx *ctx, const float *x, int64_t n_frames, int32_t in_channels,
                                  const int32_t *delays, int32_t n_delays, int32_t delayed_channel, int32_t ms,
                                  int32_t use_width, double width, double *moments);

#ifdef __cplusplus
}
#endif
#endif /* VND_SCAN_H */

/* vnd_analysis.h - analysis entry points of libvnd_amd.so: how well a decorrelator decorrelated.
 *
 * Same conventions as vnd_amd.h (plain C99, vnd_status, vnd_last_error, "*_dev" = device pointers and a
 * hipStream_t passed as void*), exported by the same library, and kept out of vnd_amd.h so that the
 * decorrelation ABI stays small.
 */
#ifndef VND_ANALYSIS_H
#define VND_ANALYSIS_H

#include "vnd_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Largest window (samples) vnd_correlogram_f32_dev covers: it bounds the kernel's LDS staging. */
#define VND_CORRELOGRAM_MAX_WINDOW 16384

/* ---- cross-correlogram (utils/dsp.py:313-356) -------------------------------------------------------
 * For each stream b and window w (start s = w * hop), with x_w[i] = x[b * stream_stride + (s + i) * frame_stride]
 * and y_w likewise, i in [0, window):
 *   num[j]  = sum over i of y_w[i] * x_w[i + j - (window - 1)]        (x_w = 0 outside [0, window))
 *           = np.correlate(x_w, y_w, 'full')[j],   j in [0, 2 window - 1): lag j - (window - 1)
 *   out[b][w][j] = num[j] / f32(sqrtf(f32(Exx * Eyy)) + eps)   for j < min(num_lags, 2 window - 1), else 0
 * with Exx = sum x_w^2, Eyy = sum y_w^2.  Output layout: float32 [batch][windows][num_lags], C-contiguous,
 * windows = n_frames >= window ? (n_frames - window) / hop + 1 : 0.  The column map keeps the reference's own:
 * num_lags < 2 window - 1 keeps the most negative lags; num_lags > 2 window - 1 leaves trailing zero columns.
 * Numerics: each num[j] is one float64 FMA chain over the exact products f64(x) * f64(y), in a fixed order,
 * rounded once to float32; Exx and Eyy are float64 sums, each rounded once to float32; the normaliser and the
 * division are float32 as NumPy 2 does them (correctly rounded, denormals kept).  Against R, the same formula
 * with exact sums, the result is within one float32 ulp (it is R unless a float64 sum lands next to a float32
 * rounding boundary), and within (2 window + 4) * 2^-24 absolute of the reference's float32 result.  Silent
 * windows and windows whose float32 energy product overflows give 0, as in the reference.  The order of every
 * sum is fixed: results are bit-identical across batch sizes, stream positions, frame strides and runs.
 * Non-finite samples are outside the contract.
 * x, y: device float32; out: device float32, not overlapping x or y (x and y may alias: an auto-correlogram,
 * or channels 0 and 1 of one (batch, n, 2) buffer with frame_stride 2).  Every size and stride must be >= 1
 * (VND_ERR_INVALID otherwise, checked before anything is launched); window > VND_CORRELOGRAM_MAX_WINDOW is
 * VND_ERR_UNSUPPORTED.  Enqueues on hip_stream only: allocates nothing, graph-capturable, thread-safe.        */
vnd_status vnd_correlogram_f32_dev(vnd_ctx *ctx, const float *x_dev, const float *y_dev, float *out_dev,
                                   int64_t batch, int64_t n_frames, int64_t stream_stride, int32_t frame_stride,
                                   int32_t window, int32_t hop, int32_t num_lags, float eps, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* VND_ANALYSIS_H */

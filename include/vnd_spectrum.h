/* vnd_spectrum.h - short-time spectra of a pool on the device, exported by libvnd_amd.so: for every signal and channel of a
 * pool, scipy.signal.spectrogram's power columns (mode 'psd', one-sided), and Welch's averages of them - Pxx, Pyy and the
 * cross spectrum Pxy = conj(X_L) * X_R, which scipy.signal.welch, csd and coherence are made of.
 *
 * Same conventions as vnd_level.h (plain C99, vnd_status, vnd_last_error, "*_dev" = device pointers and a hipStream_t passed
 * as void*).  The entries enqueue on hip_stream only: they allocate nothing, read no device memory from the host, synchronise
 * nothing, are graph-capturable and thread-safe.  Every argument is checked before anything is enqueued, with nothing
 * written: first the arguments (VND_ERR_INVALID, then VND_ERR_UNSUPPORTED), last the context (a null ctx is VND_ERR_INVALID
 * "null context").
 *
 * ---- the pool -----------------------------------------------------------------------------------------------------------
 * Sample t of channel c of signal b is frames_dev[b * stream_stride + t * frame_stride + c], c < channels (1 or 2), so
 * frame_stride >= channels; a mono view of one channel of a stereo pool is channels = 1, frame_stride = 2.  n_each_dev: null,
 * or int32 [batch] in device memory: signal b is its first n_each[b] frames; a value outside [0, n_frames] contributes no
 * frame, and nothing is indexed with it.
 *
 * ---- a segment ----------------------------------------------------------------------------------------------------------
 * Segment t of a signal is its frames [t * hop, t * hop + nperseg); a signal of m frames has (m - nperseg) / hop + 1 whole
 * segments (none when m < nperseg - unlike SciPy, nperseg is never shortened), and the pool's columns are
 * segments = (n_frames - nperseg) / hop + 1.  detrend != 0 subtracts the segment's mean: the frames are added in float64 in a
 * fixed tree that depends on nfft alone, divided by nperseg and rounded once to the sample type.  The difference is multiplied
 * by window_dev[i] (nperseg values of the sample type), zero-padded to nfft and transformed: a real-input transform of the
 * segment alone - even samples real, odd samples imaginary, an nfft/2-point Stockham transform in LDS (radix 4, one radix-2
 * stage when log2(nfft/2) is odd) and the split step - so a column is a function of its own segment of its own channel only,
 * bit for bit, wherever it lies in the pool.  twiddles_dev: nfft pairs (cos, -sin) of 2 pi i / nfft in the sample type, rounded
 * from float64 by the caller.  No product is fused (the build has -ffp-contract=off).
 *
 * A power is (re * re + im * im) * scale, doubled for every bin but 0 and nfft / 2; a cross product is
 * (reL * reR + imL * imR, reL * imR - imL * reR) * scale, doubled likewise; `scale` is rounded to the sample type once.  All of
 * it is sample-type arithmetic, as SciPy's.
 *
 * ---- outputs ------------------------------------------------------------------------------------------------------------
 * F = nfft / 2 + 1.  sxx_dev: [batch][channels][F][segments] of the sample type, fully written: a column at or past a
 * signal's own segment count is zero.  pxx_dev, pyy_dev: [batch][F]; pxy_dev: [batch][F][2] (re, im): the per-segment values
 * are added in float64 in ascending segment order - a workgroup its run of VND_SPECTRUM_RUN-bounded consecutive segments, a
 * second kernel the runs - divided by the signal's own segment count and rounded once; no floating-point atomics, so a result
 * does not depend on the pool, the schedule or the run.  A signal with no whole segment gives zeros.  With channels = 1 only
 * pxx_dev is written, and pyy_dev and pxy_dev may be null.
 *
 * ---- work ---------------------------------------------------------------------------------------------------------------
 * work_dev (cross spectra only): caller-owned, 8-byte aligned, at least vnd_cross_spectra_work_bytes(...) bytes: the float64
 * sums of every run.  What the memory held does not matter.
 *
 * ---- refusals -----------------------------------------------------------------------------------------------------------
 * VND_ERR_INVALID: a null pointer (n_each_dev may be null; pyy_dev, pxy_dev with one channel); batch, n_frames, a stride,
 * nperseg - 1 or hop below 1; channels not 1 or 2, or above frame_stride; n_frames < nperseg; a scale that is NaN, or not
 * positive and finite in the sample type; work_bytes below the query's answer or work_dev not 8-byte aligned; outputs
 * overlapping one another or any input.
 * VND_ERR_UNSUPPORTED: nfft not a power of two in [VND_SPECTRUM_MIN_NFFT, VND_SPECTRUM_MAX_NFFT]; nperseg above nfft; hop
 * above nperseg; batch above VND_MAX_STREAMS; n_frames above 2^31 - 1; more than 2^23 workgroups in a launch; extents of
 * the pool or of an output that overflow (2^59 elements).  What the work memory must hold, and which buffers overlap, is
 * defined for a supported shape only: of the VND_ERR_INVALID checks, work_bytes and the overlaps come after the
 * VND_ERR_UNSUPPORTED ones.                                                                                                */
#ifndef VND_SPECTRUM_H
#define VND_SPECTRUM_H

#include "vnd_scope.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VND_SPECTRUM_MIN_NFFT 64
#define VND_SPECTRUM_MAX_NFFT 4096
#define VND_SPECTRUM_RUN 32                /* the most consecutive segments a workgroup owns */

/* The run length of a call: consecutive segments of one signal per workgroup, 1..VND_SPECTRUM_RUN, a function of these
 * arguments alone.  cross_channels: 0 for the spectrogram, 1 or 2 for the cross spectra - the same for both, so that a
 * channel's sums are grouped alike in a stereo pool and in a mono view of it.  No context. */
vnd_status vnd_spectrum_run_length(int32_t nfft, int32_t nperseg, int32_t hop, int32_t is_float64, int32_t cross_channels,
                                   int32_t *run);

/* Bytes of work memory for a cross-spectra call of this shape.  No context. */
vnd_status vnd_cross_spectra_work_bytes(int64_t batch, int64_t n_frames, int32_t channels, int32_t nperseg, int32_t hop,
                                        int32_t nfft, int32_t is_float64, int64_t *bytes);

vnd_status vnd_spectrogram_f32_dev(vnd_ctx *ctx, const float *frames_dev, int64_t batch, int64_t n_frames,
                                   int64_t stream_stride, int32_t frame_stride, int32_t channels, const float *window_dev,
                                   const float *twiddles_dev, int32_t nperseg, int32_t hop, int32_t nfft, int32_t detrend,
                                   double scale, const int32_t *n_each_dev, float *sxx_dev, void *hip_stream);
vnd_status vnd_spectrogram_f64_dev(vnd_ctx *ctx, const double *frames_dev, int64_t batch, int64_t n_frames,
                                   int64_t stream_stride, int32_t frame_stride, int32_t channels, const double *window_dev,
                                   const double *twiddles_dev, int32_t nperseg, int32_t hop, int32_t nfft, int32_t detrend,
                                   double scale, const int32_t *n_each_dev, double *sxx_dev, void *hip_stream);

vnd_status vnd_cross_spectra_f32_dev(vnd_ctx *ctx, const float *frames_dev, int64_t batch, int64_t n_frames,
                                     int64_t stream_stride, int32_t frame_stride, int32_t channels, const float *window_dev,
                                     const float *twiddles_dev, int32_t nperseg, int32_t hop, int32_t nfft, int32_t detrend,
                                     double scale, const int32_t *n_each_dev, float *pxx_dev, float *pyy_dev, float *pxy_dev,
                                     void *work_dev, int64_t work_bytes, void *hip_stream);
vnd_status vnd_cross_spectra_f64_dev(vnd_ctx *ctx, const double *frames_dev, int64_t batch, int64_t n_frames,
                                     int64_t stream_stride, int32_t frame_stride, int32_t channels, const double *window_dev,
                                     const double *twiddles_dev, int32_t nperseg, int32_t hop, int32_t nfft, int32_t detrend,
                                     double scale, const int32_t *n_each_dev, double *pxx_dev, double *pyy_dev,
                                     double *pxy_dev, void *work_dev, int64_t work_bytes, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* VND_SPECTRUM_H */

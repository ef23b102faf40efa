/* vnd_velvet_search.h - velvet-noise search entry points of libvnd_amd.so: score (signal, candidate filter) pairs of a
 * pool of signals in one launch, the unit of work of a batched velvet-noise optimiser.
 *
 * Same conventions as vnd_amd.h (plain C99, vnd_status, vnd_last_error, "*_dev" = device pointers and a hipStream_t
 * passed as void*), exported by the same library, and kept out of vnd_amd.h, vnd_scan.h and vnd_haas_search.h so that
 * those headers keep their fixed sets of functions.
 */
#ifndef VND_VELVET_SEARCH_H
#define VND_VELVET_SEARCH_H

#include "vnd_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Pairs one vnd_velvet_pairs_f32_* call takes at most (split larger sets). */
#define VND_VELVET_PAIRS_MAX 1048560
/* Largest tap index of a bank the pairs kernel takes: a workgroup stages a tile of 2048 frames plus the bank's largest
 * tap index in LDS.  A bank beyond it is VND_ERR_UNSUPPORTED (score it with vnd_scan_bank_f32_host, signal by signal). */
#define VND_VELVET_PAIRS_MAX_TAP_INDEX 4094

/* ---- velvet-noise scan over (signal, candidate) pairs of a pool ----------------------------------------------------
 * `bank` is a tap table of 2*T channels: candidate t owns channels 2t (left) and 2t + 1 (right), as in
 * vnd_scan_bank_f32_host.  Class-path tables (segments, gains, pass-through flags) and function-path tables are both
 * taken.  For a float32 pool x[batch][n_frames][in_channels] (in_channels 1: mono, fanned out to both outputs;
 * 2: stereo) and P = n_pairs pairs (signals[p], candidates[p]), moments[p] is the eight float64 quantities of
 * vnd_scan_bank_f32_host, in its order,
 *   { sum r, sum r*t, sum r*t^2, sum r*t^3, max |t|, sum L*R, sum L^2, sum R^2 },
 * over the n_frames frames (L, R) of candidate candidates[p] convolved with signal x[signals[p]].
 * Numerics: only VND_MODE_EXACT; every frame is bit-identical to the exact-mode convolution of vnd_convolve_* (per
 * segment seg += x*w with two roundings per tap in table order, seg *= gain, out += seg; terms with n + i >= n_frames
 * drop out; a pass-through channel is the input).  t, r and the products are float32 as in vnd_scan_bank_f32_host,
 * the sums float64 in a fixed order that depends on n_frames alone.  So a row depends only on its signal's samples,
 * n_frames, in_channels and its candidate's taps, segments, gains and flags: not on the candidate's position in the
 * bank or the other candidates, not on the other pairs, their order, duplicates or how pairs are split into calls, and
 * not on the signal's index in the pool.  Pairs sorted by (signal, candidate) run fastest (a workgroup stages the
 * window of a run of one signal's pairs once); any order gives the same rows.  Non-finite samples or weights are
 * outside the contract.
 *
 * vnd_velvet_pairs_workspace_bytes: the workspace vnd_velvet_pairs_f32_dev needs: ceil(n_frames / 2048) * n_pairs * 64
 * bytes; VND_ERR_INVALID for negative arguments or a null result pointer.
 * vnd_velvet_pairs_f32_dev: x float32, signals and candidates int32 [n_pairs], moments float64 [n_pairs][8] and
 * workspace_bytes of workspace, all device memory.  Signal and candidate indices are only read on the device: a pair
 * whose signal is outside [0, batch) or whose candidate is outside [0, T) gets a row of NaN from a bounds check in the
 * kernel; nothing out of range is accessed and the other rows are unaffected.  Checked before anything is launched:
 * VND_ERR_INVALID for a null context or bank, negative counts, in_channels not in {1, 2}, a bank with an odd number of
 * channels, a workspace smaller than the query's answer, or a null pointer; VND_ERR_UNSUPPORTED for a mode other
 * than VND_MODE_EXACT, above VND_VELVET_PAIRS_MAX pairs, for a bank whose largest tap index is above
 * VND_VELVET_PAIRS_MAX_TAP_INDEX, and for a bank with a weight that is not finite.  Enqueues on hip_stream only: allocates nothing, graph-capturable, thread-safe.
 * vnd_velvet_pairs_f32_host: the same from host memory, synchronous.  Every signal and candidate index is validated
 * before anything is launched: one out of range is VND_ERR_INVALID, and the message names the pair.                  */
vnd_status vnd_velvet_pairs_workspace_bytes(int64_t n_frames, int32_t n_pairs, int64_t *bytes);
vnd_status vnd_velvet_pairs_f32_dev(vnd_ctx *ctx, const vnd_taps *bank, const float *x_dev, int32_t batch,
                                    int64_t n_frames, int32_t in_channels, const int32_t *signals_dev,
                                    const int32_t *candidates_dev, int32_t n_pairs, int32_t mode, double *moments_dev,
                                    void *workspace_dev, int64_t workspace_bytes, void *hip_stream);
vnd_status vnd_velvet_pairs_f32_host(vnd_ctx *ctx, const vnd_taps *bank, const float *x, int32_t batch,
                                     int64_t n_frames, int32_t in_channels, const int32_t *signals,
                                     const int32_t *candidates, int32_t n_pairs, int32_t mode, double *moments);

#ifdef __cplusplus
}
#endif
#endif /* VND_VELVET_SEARCH_H */

/* vnd_haas_search.h - Haas-delay search entry points of libvnd_amd.so: score (signal, delay) pairs of a pool of
 * signals in one launch, the unit of work of a batched Haas-delay optimiser.
 *
 * Same conventions as vnd_amd.h (plain C99, vnd_status, vnd_last_error, "*_dev" = device pointers and a hipStream_t
 * passed as void*), exported by the same library, and kept out of vnd_amd.h and vnd_scan.h so that those headers keep
 * their fixed sets of functions.
 */
#ifndef VND_HAAS_SEARCH_H
#define VND_HAAS_SEARCH_H

#include "vnd_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Pairs one vnd_haas_pairs_f64_* call takes at most (split larger sets). */
#define VND_HAAS_PAIRS_MAX 1048560

/* ---- Haas-delay scan over (signal, delay) pairs of a pool ---------------------------------------------------------
 * For a float32 pool x[batch][n_frames][in_channels] (in_channels 1: mono, 2: stereo) and P = n_pairs pairs
 * (signals[p], delays[p]), all under one HaasEffect configuration (delayed_channel 0 | 1, ms = MS layout,
 * use_width / width = apply_stereo_width), moments[p] is the row vnd_haas_scan_f64_* (vnd_scan.h) gives for signal
 * x[signals[p]] alone with the one delay delays[p], bit for bit: the same eight float64 quantities in the same order
 * and the same fixed summation order, which depends only on n_frames and delays[p].  A row depends neither on the
 * order of the pairs, nor on the other pairs of a call, nor on how the pairs are split into calls.  Pairs sorted by
 * (signal, delay) run fastest (a workgroup stages the history window of a run of one signal's pairs once); any order
 * and duplicate pairs give the same rows.  Non-finite samples are outside the contract.
 *
 * vnd_haas_pairs_workspace_bytes: the workspace vnd_haas_pairs_f64_dev needs for n_pairs pairs whose delays are at
 * most max_delay frames (the same formula as vnd_haas_scan_workspace_bytes); VND_ERR_INVALID for negative arguments.
 * vnd_haas_pairs_f64_dev: x float32, signals and delays int32 [n_pairs], moments float64 [n_pairs][8] and
 * workspace_bytes of workspace, all device memory.  Signal indices and delays are only read on the device: a pair
 * whose signal is outside [0, batch), whose delay is negative, or whose delay is above the max_delay the workspace was
 * sized for gets a row of NaN; the other rows are unaffected.  VND_ERR_INVALID, checked before anything is launched,
 * for batch < 0, n_frames < 0, n_pairs < 0, in_channels not in {1, 2}, delayed_channel not in {0, 1}, a negative
 * workspace_bytes or a null pointer; VND_ERR_UNSUPPORTED above VND_HAAS_PAIRS_MAX pairs.  Enqueues on hip_stream
 * only: allocates nothing, graph-capturable, thread-safe.
 * vnd_haas_pairs_f64_host: the same from host memory, synchronous.  Every signal index and delay is validated
 * before anything is launched: one outside [0, batch), or a negative delay, is VND_ERR_INVALID.                      */
vnd_status vnd_haas_pairs_workspace_bytes(int64_t n_frames, int32_t n_pairs, int32_t max_delay, int64_t *bytes);
vnd_status vnd_haas_pairs_f64_dev(vnd_ctx *ctx, const float *x_dev, int32_t batch, int64_t n_frames,
                                  int32_t in_channels, const int32_t *signals_dev, const int32_t *delays_dev,
                                  int32_t n_pairs, int32_t delayed_channel, int32_t ms, int32_t use_width, double width,
                                  double *moments_dev, void *workspace_dev, int64_t workspace_bytes, void *hip_stream);
vnd_status vnd_haas_pairs_f64_host(vnd_ctx *ctx, const float *x, int32_t batch, int64_t n_frames, int32_t in_channels,
                                   const int32_t *signals, const int32_t *delays, int32_t n_pairs,
                                   int32_t delayed_channel, int32_t ms, int32_t use_width, double width,
                                   double *moments);

#ifdef __cplusplus
}
#endif
#endif /* VND_HAAS_SEARCH_H */

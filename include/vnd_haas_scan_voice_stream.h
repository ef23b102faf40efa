/* vnd_haas_scan_voice_stream.h - the Haas-delay scan of a VOICE POOL, exported by libvnd_amd.so: the eight polar moments of
 * vnd_scan.h / vnd_haas_search.h for (slot, delay) pairs of a pool whose slots are voices and whose positions live in device
 * memory, scored against the last W = window_frames input frames of each voice.  It is what a server needs to re-optimise the
 * Haas delay of a running voice: push every block, scan a grid of candidate delays when a decision is due, take the argmin and
 * hand it to vnd_haas_voice_fade_stream.h as the voice's new delay - all on the device, on one stream.  A delay cares about the
 * order of the frames, so the pool keeps the window itself: a ring per slot remembers the voice's last W input frames as they
 * were pushed.  It reads the x, the counts and the flags of a decorrelating pool (vnd_haas_voice_stream.h,
 * vnd_haas_voice_fade_stream.h) straight from device memory.  A call is a pure function of device memory - no argument depends
 * on the call's history - so it can be captured in a graph and replayed.
 *
 * Same conventions as vnd_polar_level_voice_stream.h (plain C99, vnd_status, vnd_last_error, "*_dev" = device pointers and a
 * hipStream_t passed as void*), and kept out of vnd_amd.h, vnd_scan.h and vnd_haas_search.h so that they keep their fixed sets
 * of functions.  Every *_dev entry enqueues on hip_stream only: no allocation, no synchronisation, no read of device memory by
 * the host, no other stream; capturable and thread-safe.  Two entries: the PUSH takes a call's frames into the rings; PAIRS
 * scores (slot, delay) pairs from the state alone.  Blocks arrive a hundred times a second and a voice is re-optimised now and
 * then: push every block, scan when a delay is to be chosen.
 *
 * ---- push: one call, per slot b -----------------------------------------------------------------------------------------
 * The slot rule of vnd_scope_voice_stream.h.  Read on the device: pos[b] from the state, counts[b] (int32, frames pushed for
 * this slot in this call, 0..M, M = max_frames_per_call) and flags[b] (int32, VND_VOICE_START and VND_VOICE_END of
 * vnd_voice_stream.h; other bits are ignored - VND_VOICE_SWITCH of vnd_voice_fade_stream.h in particular, so the pool takes the
 * very x, counts and flags of a fading pool):
 *     p = START ? 0 : pos[b]                  START: whatever the slot held is dropped
 *     n = counts[b]
 *     for every frame g in [p, p + n):  ring[b][g mod W] = frame g, its in_channels float32 values
 *     valid[b] = 1
 *     fill[b]  = min(p + n, W)                how many ring entries are the voice's
 *     head[b]  = (p + n) mod W                the entry the voice's next frame would take
 *     pos[b]   = END ? 0 : p + n              after the call; END leaves fill, head and the ring as they are: the window
 *                                             stays readable until the slot's next voice
 * A slot with n = 0 and neither flag is idle: valid[b] = 0 and nothing of its state is touched.  START and END in one call
 * are a whole voice in one block.
 * The window in time order is the ring entries (head[b] - fill[b] + k) mod W, k in [0, fill[b]): the voice's frames
 * [q - fill[b], q), q its position after its last answered push.  The level pool (vnd_polar_level_voice_stream.h) keeps fill
 * alone because a percentile does not depend on order; a delay does, and the position cannot stand for head because an END
 * zeroes it.  After a START over a full ring the stale entries of the previous voice lie outside the window and are never read.
 * Why no lane races another on the ring: max_frames_per_call <= W is required, so the frames [p, p + n) of one call have
 * n <= W distinct residues mod W - every entry a call touches is written by the one lane that owns its frame, although the
 * workgroups of a slot are not ordered.  The ring is never cleared and never read by the push.
 *
 * Bad per-slot values (the other slots are unaffected): counts[b] outside [0, M], or - without START - a stored position
 * outside [0, 2^60] (a state that was never reset): valid[b] = -1; the ring, fill, head and the position of the slot are
 * untouched and nothing is indexed with the bad value.  It is the rule of vnd_voice_stream.h, so a -1 from a decorrelating
 * pool, handed on as a count, passes through as -1.
 *
 * Chunk: x_dev float32 [slots][M][in_channels], contiguous, in_channels 1 (mono) or 2 (stereo); only the first counts[b] frames
 * of row b are read.  valid_dev: int32 [slots].  Two kernels: the copy (ceil(M / 1024) workgroups a slot; idle and bad slots
 * and workgroups past n leave at once) and one lane per slot that writes valid, fill, head and pos.
 *
 * ---- pairs --------------------------------------------------------------------------------------------------------------
 * A pure function of the state.  For P = n_pairs pairs (slots_of_pair[p], delays[p]), int32 arrays read on the device, all
 * under one HaasEffect configuration (delayed_channel 0 | 1, ms = MS layout, use_width / width = apply_stereo_width),
 * moments_dev [P][8] float64 is fully written by every successful call.
 * Contract.  moments[p] equals BYTE FOR BYTE the row vnd_haas_scan_f64_* (vnd_scan.h) - and so vnd_haas_pairs_f64_*
 * (vnd_haas_search.h) - gives for a contiguous signal x[n_frames][in_channels] that is slot slots_of_pair[p]'s window in time
 * order, n_frames = fill[slot], at the one delay delays[p]: the same eight float64 quantities in the same order and the same
 * summation order - per lane over its 8 frames of a tile of 2048, a fixed shuffle tree and wave order per (tile, pair)
 * partial, then the fixed reduction of the pair's ceil((fill + d) / 2048) partials - for every schedule of block sizes, idle
 * calls, restarts and neighbours, for every order of the pairs and every split of the pairs into calls.  Both entries run one
 * kernel body; only where a frame is loaded from differs.  Pairs sorted by (slot, delay) run fastest (a workgroup stages the
 * history window of a run of one slot's pairs once); any order and duplicate pairs give the same rows.  Non-finite samples are
 * outside the contract.
 * A slot that never started, or that started without a frame, has fill = 0: its row is the one-shot's for n_frames = 0, which
 * is eight times +0.0 at every delay - with d = 0 there is no frame and the reduction starts from +0.0; with d > 0 the d frames
 * of the roll are (0, 0), whose atan2 is 0 (or +-pi, folded to 0), whose radius is 0 and whose every term is a zero added to
 * +0.0.
 * What is read from device memory and would index something: slots_of_pair[p] outside [0, slots); delays[p] negative or above
 * max_delay; a slot whose fill is outside [0, W] or whose head is outside [0, W) (a state that was never reset).  Each gives
 * that pair a row of eight NaN; nothing is addressed with the bad value and the other rows are unaffected.
 * Grid: (ceil((W + max_delay) / 2048), ceil(P / 16)) for the scan, workgroups past a pair's own fill + d leave before any
 * barrier; P workgroups for the reduction.  workspace_dev: caller-owned, 8-byte aligned, at least
 * vnd_haas_scan_voice_stream_workspace_bytes(window_frames, n_pairs, max_delay) = P * ceil((W + max_delay) / 2048) * 64 bytes;
 * it is written before it is read, nothing needs clearing.
 *
 * ---- state --------------------------------------------------------------------------------------------------------------
 * `state_bytes` at least what vnd_haas_scan_voice_stream_state_bytes returns, state_dev 16-byte aligned.  In this order,
 * each part padded to a multiple of 16 bytes:
 *     positions  int64 [slots]
 *     fill       int32 [slots]
 *     head       int32 [slots]
 *     ring       float32 [slots][W][in_channels]
 * Positions, fills and heads must start at 0: vnd_haas_scan_voice_stream_reset_dev enqueues one hipMemsetAsync over those
 * three (and their padding) ONLY (it ends every voice and empties every window; the rings are never cleared and never read
 * beyond fill).  Push and pairs read and write the state on the call's stream: calls of one pool run in order on one
 * hipStream_t (or are ordered by the caller).
 *
 * ---- refusals -----------------------------------------------------------------------------------------------------------
 * Checked before anything is enqueued, with nothing written, first the arguments and last the context (a null ctx is
 * VND_ERR_INVALID).  VND_ERR_INVALID: a null pointer; slots, max_frames_per_call or n_pairs below 1 (or max_frames_per_call
 * above INT32_MAX: counts are int32); window_frames below max_frames_per_call; in_channels not 1 or 2; delayed_channel not 0
 * or 1; a negative max_delay; state_bytes or workspace_bytes below the query's answer; a state not 16-byte aligned, a chunk not
 * aligned to a frame, moments or a workspace not 8-byte aligned; outputs (valid; moments, workspace) and - for the push - the
 * state overlapping one another or any input (the chunk, counts, flags; the state, the slot indices, the delays).
 * VND_ERR_UNSUPPORTED: slots above VND_MAX_STREAMS; window_frames above INT32_MAX; n_pairs above VND_HAAS_PAIRS_MAX; more than
 * 2^23 workgroups in the push's launch (slots * ceil(M / 1024)).                                                             */
#ifndef VND_HAAS_SCAN_VOICE_STREAM_H
#define VND_HAAS_SCAN_VOICE_STREAM_H

#include "vnd_amd.h"
#include "vnd_haas_search.h"
#include "vnd_voice_stream.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The state of a pool, in bytes (see "state" above).  No context. */
vnd_status vnd_haas_scan_voice_stream_state_bytes(int64_t slots, int64_t max_frames_per_call, int64_t window_frames,
                                                  int32_t in_channels, int64_t *bytes);
/* Every position, fill and head to 0, with the pool's own checks.  The rings are left alone. */
vnd_status vnd_haas_scan_voice_stream_reset_dev(vnd_ctx *ctx, void *state_dev, int64_t state_bytes, int64_t slots,
                                                int64_t max_frames_per_call, int64_t window_frames, int32_t in_channels,
                                                void *hip_stream);

/* x_dev: float32 [slots][max_frames_per_call][in_channels]; counts_dev, flags_dev, valid_dev: int32 [slots]. */
vnd_status vnd_haas_scan_voice_stream_push_f32_dev(vnd_ctx *ctx, void *state_dev, int64_t state_bytes,
                                                   int64_t max_frames_per_call, int64_t window_frames, const float *x_dev,
                                                   int32_t in_channels, const int32_t *counts_dev, const int32_t *flags_dev,
                                                   int32_t *valid_dev, int64_t slots, void *hip_stream);

/* Bytes of workspace for a pairs call of n_pairs pairs whose delays are at most max_delay frames.  No context. */
vnd_status vnd_haas_scan_voice_stream_workspace_bytes(int64_t window_frames, int32_t n_pairs, int32_t max_delay,
                                                      int64_t *bytes);

/* slots_of_pair_dev, delays_dev: int32 [n_pairs]; moments_dev: float64 [n_pairs][8]. */
vnd_status vnd_haas_scan_voice_stream_pairs_f64_dev(vnd_ctx *ctx, const void *state_dev, int64_t state_bytes,
                                                    int64_t max_frames_per_call, int64_t window_frames, int32_t in_channels,
                                                    int64_t slots, const int32_t *slots_of_pair_dev,
                                                    const int32_t *delays_dev, int32_t n_pairs, int32_t max_delay,
                                                    int32_t delayed_channel, int32_t ms, int32_t use_width, double width,
                                                    double *moments_dev, void *workspace_dev, int64_t workspace_bytes,
                                                    void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* VND_HAAS_SCAN_VOICE_STREAM_H */

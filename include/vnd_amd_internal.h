/* vnd_amd_internal.h - measurement, tuning and diagnosis hooks of libvnd_amd.so.
 *
 * NOT part of the drop-in ABI (include/vnd_amd.h): bench.py, tools/ and the tests use these to time
 * launches, to read the per-table kernel sources without a device, and to force kernel variants.
 * They are exported by the same shared library, may change with any build, and a host that only
 * decorrelates never needs them.  Same conventions as vnd_amd.h (plain C, vnd_status, no torch types).
 */
#ifndef VND_AMD_INTERNAL_H
#define VND_AMD_INTERNAL_H

#include "vnd_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- measurement helpers (used by bench.py; not on the data path) ---------- */
/* Launches the convolve `iters` times back to back on `hip_stream`, cycling
 * through `n_buffers` (x,y) pairs laid out at x_dev + i*stride_elems, and
 * returns the average kernel milliseconds between two hipEvents recorded on
 * that same stream.                                                          */
vnd_status vnd_time_convolve_f32_dev(vnd_ctx *ctx, const vnd_taps *taps, const float *x_dev,
                                     float *y_dev, int64_t batch, int64_t n_frames,
                                     int32_t n_channels, int32_t mode, int32_t n_buffers,
                                     int64_t stride_elems, int32_t iters, void *hip_stream,
                                     float *avg_ms);
/* Bytes of private (scratch) memory per lane the kernel `kernel` of a gfx950 code object (an ELF image)
 * asks for, read from its kernel descriptor: > 0 means the compiler spilled registers.  The library
 * rejects such builds of the window form of its per-table kernels (the registers ARE that kernel);
 * exposed so that the check can be tested without a device.  -1: no such kernel in the image.        */
vnd_status vnd_code_object_private_bytes(const void *code, int64_t bytes, const char *kernel,
                                         int64_t *private_bytes);
/* The box's streaming ceiling, as a companion of the 8 TB/s figure: `iters` plain copies of `elems`
 * floats (a multiple of 4; 16-byte aligned buffers) with 16-byte non-temporal accesses, the average
 * kernel milliseconds between two hipEvents on `hip_stream`.                                    */
vnd_status vnd_time_copy_f32_dev(vnd_ctx *ctx, const float *x_dev, float *y_dev, int64_t elems,
                                 int32_t iters, void *hip_stream, float *avg_ms);
/* VND_MODE_FAST and VND_MODE_EXACT compile a kernel PER TAP TABLE with hipRTC on first use
 * (offsets become LDS-read immediates, weights literals; persistent workgroups over an LDS ring;
 * `mode` picks the arithmetic: free summation order, or the reference's own association bit for
 * bit); the generic kernels take over whenever that is not possible.  This returns the HIP source the
 * library would hand to hipRTC for a function-path table - no device needed - so that it can be
 * audited or compiled offline (`hipcc --offload-arch=gfx950 -include hip/hip_runtime.h`).
 * text == NULL queries the size.  Even channel counts only (channel pairs share a workgroup). */
vnd_status vnd_spec_kernel_source(int32_t num_channels, const int32_t *tap_offsets,
                                  const int32_t *tap_index, const float *tap_weight, int32_t mode,
                                  char *text, int64_t capacity, int64_t *bytes);
/* The WINDOW form of the per-table kernel (stereo tables): a lane owns `frames_per_lane` (16 | 32 | 64)
 * consecutive output frames and reads the union of its taps' windows from LDS once.
 * Same contract as vnd_spec_kernel_source; the table as for vnd_taps_create (seg_* NULL: function path);
 * `threads` = workgroup size (multiple of 64).  When `lds_bytes_per_tile` / `fmas_per_tile` are non-NULL
 * they receive what ONE lane reads from LDS for its tap sums per tile and the (tap, output) products that
 * feeds - the kernel's figure of merit. */
vnd_status vnd_window_kernel_source(int32_t num_channels, const int32_t *tap_offsets,
                                    const int32_t *tap_index, const float *tap_weight,
                                    const int32_t *seg_offsets, const int32_t *seg_end,
                                    const float *seg_gain, int32_t apply_gain, int32_t mode,
                                    int32_t frames_per_lane, int32_t threads, char *text,
                                    int64_t capacity, int64_t *bytes, int64_t *lds_bytes_per_tile,
                                    int64_t *fmas_per_tile);
/* Kernel variant override for tuning runs: -1 = automatic choice. */
vnd_status vnd_set_variant(vnd_ctx *ctx, int32_t variant);
/* Reads a tuning variable the way the launch planner does (VND_TUNING=1 sessions only; otherwise *value = fallback).  A name that
 * is not in the library's registry (kTuningNames, csrc/vnd_spec.hpp) returns VND_ERR_INVALID with the name in vnd_last_error -
 * the same report a launch gives when the LIBRARY reads such a name (until round 5 a debug-build abort()) - and leaves no trace. */
vnd_status vnd_tuning_read(const char *name, int32_t fallback, int32_t *value);
/* Diagnosis (VND_TUNING=1 with VND_WIN_STAMPS=<workgroups>): the window-form kernel that a launch of this shape
 * uses was built with phase stamps - wave 0 of its first workgroups leaves the 100 MHz wall clock at its phase
 * boundaries, 16 uint64 per workgroup ([0] start, [1] ring filled, then per tile: taps done, window dead, outputs
 * exchanged, refill published; [15] = HW_ID | XCC_ID << 32).  Copies up to `capacity` uint64 of the last launch's
 * stamps into `stamps`; *count = how many the kernel holds (0: this launch's kernel has none).        */
vnd_status vnd_debug_read_stamps(vnd_ctx *ctx, const vnd_taps *taps, int64_t batch, int64_t n_frames,
                                 int32_t in_channels, int32_t mode, uint64_t *stamps, int64_t capacity,
                                 int64_t *count);
/* Diagnosis: the launch plan a vnd_stream_f32_dev call (include/vnd_stream.h) of `batch` streams with `n_out` output frames per
 * stream would take - the same planner, no device work - as one line of key=value fields: direct, r (frame pairs per lane),
 * cg (channels per workgroup), bc (one staged plane for a mono input fanned out), W (window frames), lds_bytes, tiles,
 * groups, nblocks.  epilogue = the call's ms_encode || use_width.                                                      */
vnd_status vnd_describe_stream_launch(vnd_ctx *ctx, const vnd_taps *taps, int64_t batch, int64_t n_out,
                                      int32_t in_channels, int32_t mode, int32_t epilogue, char *text, int32_t len);
/* Diagnosis (tests): the route a vnd_scan_bank_f32_host call of this shape takes - the call's own scalar checks and the one
 * function that decides for it, no pointers, no device work - as one line.  It starts with `fused` (the convolution's store
 * phase leaves the moments; y is never written) or `unfused` followed by `by_frame` / `by_candidate` (the stand-alone reducer's
 * kernel: a lane per candidate from 64 pairs on), then the convolution's kernel (conv_ordered | conv_fast, with _fanout for a
 * mono input staged once; conv_direct; conv_none for an empty signal) and the plan as key=value fields: cg (channels per
 * workgroup), r (frame pairs per lane: the tile is 2 * nt * r frames), nt (threads), bc (1: the fan-out staging), tiles,
 * direct, halo, lds, workgroups, mode, pairs.                                                                            */
vnd_status vnd_describe_scan(vnd_ctx *ctx, const vnd_taps *bank, int64_t n_frames, int32_t in_channels, int32_t mode,
                             char *text, int32_t len);
/* Diagnosis: the launch a vnd_each_stream_f32_dev call (include/vnd_each_stream.h) with these arguments would take - the
 * call's own scalar checks and planner, no device work - as one line of key=value fields: r (frame pairs per lane: the
 * tile is 2 * 256 * r frames), W (window frames), lds_bytes, tiles (per stream), nblocks, n_out, fma (a bank of +-1
 * weights takes the fma instantiation: the same bits).  epilogue = the call's ms_encode || use_width.                    */
vnd_status vnd_describe_each_stream_launch(vnd_ctx *ctx, const vnd_taps *bank, int64_t max_frames_per_call, int64_t batch,
                                           int64_t position, int64_t n_in, int32_t in_channels, int32_t final,
                                           int32_t mode, int32_t epilogue, char *text, int32_t len);
/* Diagnosis: the launch every vnd_voice_stream_f32_dev call (include/vnd_voice_stream.h) on a pool with these arguments
 * takes - the pool's own scalar checks and planner, no pointers, no device work - as one line of key=value fields: r, W,
 * lds_bytes, tiles (of the longest row, max_frames_per_call + H frames), nblocks (slots x tiles), fma, epilogue, threads,
 * advance_groups (the workgroups of the kernel that advances the positions, one lane per slot).                          */
vnd_status vnd_describe_voice_stream_launch(vnd_ctx *ctx, const vnd_taps *bank, int64_t max_frames_per_call, int64_t slots,
                                            int32_t in_channels, int32_t mode, int32_t epilogue, char *text, int32_t len);
/* Diagnosis: the launch every vnd_voice_fade_stream_f32_dev call (include/vnd_voice_fade_stream.h) on a pool with these
 * arguments takes - that pool's scalar checks, vnd_describe_voice_stream_launch's planner - as one line that starts with
 * voice_fade_stream and carries that hook's fields, then fade_frames.                                                   */
vnd_status vnd_describe_voice_fade_stream_launch(vnd_ctx *ctx, const vnd_taps *bank, int64_t max_frames_per_call,
                                                 int64_t fade_frames, int64_t slots, int32_t in_channels, int32_t mode,
                                                 int32_t epilogue, char *text, int32_t len);
/* Diagnosis: the launch every vnd_correlogram_voice_stream_*_dev call (include/vnd_correlogram_voice_stream.h) on a pool with
 * these sizes takes - the pool's own scalar checks and planner, no context, no pointers, no device work - as one line of
 * key=value fields: rows_per_call (RC = ceil(max_frames_per_call / hop)), groups (window groups of 4 rows per slot), tiles
 * (column tiles of 1024 lags), nblocks (slots x groups x tiles), threads, advance_groups (the workgroups of the kernel that
 * advances the positions, one lane per slot).                                                                           */
vnd_status vnd_describe_correlogram_voice_stream_launch(int64_t slots, int32_t window, int32_t hop, int32_t num_lags,
                                                        int64_t max_frames_per_call, char *text, int32_t len);
/* Diagnosis: the launch every vnd_polar_voice_stream_*_dev call (include/vnd_polar_voice_stream.h) on a pool with these sizes
 * takes - the pool's own scalar checks and planner, no context, no pointers, no device work - as one line of key=value
 * fields: groups (chunk workgroups per slot, ceil(max_frames_per_call / 512) + 1), nblocks (slots x groups), finish_groups
 * (the workgroups of the kernel that folds the partials and advances the positions, one per slot), threads, state_bytes. */
vnd_status vnd_describe_polar_voice_stream_launch(int64_t slots, int64_t max_frames_per_call, int32_t sample_bytes,
                                                  char *text, int32_t len);
/* Diagnosis: the launch every vnd_spectrum_voice_stream_*_dev call (include/vnd_spectrum_voice_stream.h) on a pool with these
 * sizes takes - the pool's own scalar checks and planner, no context, no pointers, no device work - as one line of key=value
 * fields: rows_per_call (RC = ceil(max_frames_per_call / hop)), run (R, the run length of the one-shot cross spectra), groups
 * (G = ceil(RC / R) + 1 run workgroups per slot), nblocks (slots x groups), threads, advance_groups (the workgroups of the
 * kernel that folds the runs, writes the means and advances the positions, one per slot), state_bytes.                   */
vnd_status vnd_describe_spectrum_voice_stream_launch(int64_t slots, int32_t channels, int32_t nperseg, int32_t hop,
                                                     int32_t nfft, int64_t max_frames_per_call, int32_t is_float64, char *text,
                                                     int32_t len);
/* Diagnosis (tests): vnd_decorrelate_fanout_f32_dev (in_channels == the table's channels: vnd_decorrelate_f32_dev), and which of the
 * stage's forms ran, in taken[4]: [0] 0 the table-order launch with the pointwise steps and the sums as passes of their own, 1 the
 * fast kernel with the pointwise steps (and, with VND_NORMALIZE_RMS, the sums) fused into its store phase, 2 the quad / octet kernel
 * leaving the normaliser's sums, -1 nothing ran (no frames); [1] what the convolution launch reports: 0 a generic kernel, 1 the per-table
 * kernel and it left the sums of squares, 2 the per-table kernel without them; [2] 1 if the sums are taken in NumPy's own order;
 * [3] 1 if the convolution's store phase left the block sums those start from.  The planning is decorrelate's own.              */
vnd_status vnd_debug_decorrelate_f32_dev(vnd_ctx *ctx, const vnd_taps *taps, const float *x, float *y, int64_t batch, int64_t n,
                                         int32_t in_channels, int32_t mode, int32_t ms_encode, int32_t use_width, double width,
                                         int32_t normalize, float eps, void *workspace, int64_t workspace_bytes, void *stream,
                                         int32_t *taken);

#ifdef __cplusplus
}
#endif
#endif /* VND_AMD_INTERNAL_H */

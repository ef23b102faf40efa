"""ctypes binding of ``libvnd_amd.so`` (C ABI in ``include/vnd_amd.h``).

This is the only way the package computes anything: there is no NumPy or CPU
fallback.  If the shared library is missing, or no gfx950 device is visible,
the first call that needs the GPU raises ``RuntimeError`` - loudly, by design.

How a header gets bound: its functions go into one ``*_SIGNATURES`` table, the table into ``HEADERS`` under the header's
file name.  ``load_library`` declares the prototypes of every table in ``HEADERS``; ``tests/test_abi.py`` holds every row
to its header type by type.  The wrappers pass plain ``int`` addresses, ``None`` and ``bool`` flags: the declared
``argtypes`` convert them (and refuse anything else with ``ctypes.ArgumentError``).  ``float(...)`` stays where a NumPy
scalar may arrive: ``c_double`` does not take ``np.float32``.
"""
from __future__ import annotations

import ctypes
import os
import pathlib
import threading
import weakref
from typing import Optional

import numpy as np

ABI_VERSION = 2
MODE_EXACT = 0   # acc = f32(acc + f32(x*w)) : bit-identical to the reference's NumPy paths
MODE_FMA = 1     # acc = fma(x, w, acc), table order
MODE_FAST = 2    # fma, free summation order, gains folded into weights: the throughput mode
MOMENTS = 8      # VND_MOMENTS: doubles per candidate returned by the scan
MAX_STREAMS_PER_CALL = 65535   # VND_MAX_STREAMS: the decorrelate / Haas kernels index streams by gridDim.y
NORMALIZE_OFF, NORMALIZE_RMS, NORMALIZE_RMS_REFERENCE_ORDER = 0, 1, 2   # the `normalize` argument of the decorrelate calls

_PKG = pathlib.Path(__file__).resolve().parent
LIB_PATH = pathlib.Path(os.environ.get('VND_AMD_LIBRARY', _PKG / 'libvnd_amd.so'))   # override: tuning builds only

# the C types of the headers: vnd_status / int, const char *, int32_t, int64_t, float, double, void *, and pointers to them
_int, _str, _i32, _i64, _f32, _f64, _p = (ctypes.c_int, ctypes.c_char_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float,
                                          ctypes.c_double, ctypes.c_void_p)
_i32p, _i64p, _f32p, _f64p, _u8p, _pp = (ctypes.POINTER(t) for t in (_i32, _i64, _f32, _f64, ctypes.c_uint8, _p))

# name -> (restype, argtypes), a table per header; tests/test_abi.py checks every row against its header
_CONVOLVE_DEV_ARGS = [_p, _p, _p, _p, _i64, _i64, _i32, _i32, _p]
_CONVOLVE_HOST_ARGS = [_p, _p, _f32p, _f32p, _i64, _i64, _i32, _i32]
_DECORRELATE_DEV_ARGS = [_p, _p, _p, _p, _i64, _i64, _i32, _i32, _i32, _i32, _f64, _i32, _f32, _p, _i64, _p]
_DECORRELATE_HOST_ARGS = [_p, _p, _f32p, _f32p, _i64, _i64, _i32, _i32, _i32, _i32, _f64, _i32, _f32]
_DESCRIBE_LAUNCH_ARGS = [_p, _p, _i64, _i64, _i32, _i32, _str, _i32]
SIGNATURES = {
    'vnd_abi_version': (_int, []),
    'vnd_last_error': (_str, []),
    'vnd_device_count': (_int, [_i32p]),
    'vnd_ctx_create': (_int, [_i32, _pp]),
    'vnd_ctx_destroy': (_int, [_p]),
    'vnd_ctx_info': (_int, [_p, _str, _i32, _i32p, _i64p, _i32p]),
    'vnd_taps_create': (_int, [_p, _i32, _i32p, _i32p, _f32p, _i32p, _i32p, _f32p, _u8p, _i32, _pp]),
    'vnd_taps_destroy': (_int, [_p]),
    'vnd_taps_info': (_int, [_p, _i32p, _i32p, _i32p]),
    'vnd_taps_serialize': (_int, [_p, _p, _i64, _i64p]),
    'vnd_taps_deserialize': (_int, [_p, _p, _i64, _pp]),
    'vnd_shard_range': (_int, [_i64, _i32, _i32, _i64p, _i64p]),
    'vnd_taps_broadcast_rccl': (_int, [_p, _pp, _i32, _i32, _p, _p]),
    'vnd_convolve_f32_dev': (_int, _CONVOLVE_DEV_ARGS),
    'vnd_convolve_f32_host': (_int, _CONVOLVE_HOST_ARGS),
    'vnd_decorrelate_workspace_bytes': (_int, [_i64, _i64, _i32, _i64p]),
    'vnd_decorrelate_f32_dev': (_int, _DECORRELATE_DEV_ARGS),
    'vnd_decorrelate_f32_host': (_int, _DECORRELATE_HOST_ARGS),
    'vnd_convolve_fanout_f32_dev': (_int, _CONVOLVE_DEV_ARGS),
    'vnd_convolve_fanout_f32_host': (_int, _CONVOLVE_HOST_ARGS),
    'vnd_decorrelate_fanout_f32_dev': (_int, _DECORRELATE_DEV_ARGS),
    'vnd_decorrelate_fanout_f32_host': (_int, _DECORRELATE_HOST_ARGS),
    'vnd_describe_fanout_launch': (_int, _DESCRIBE_LAUNCH_ARGS),
    'vnd_polar_moments_workspace_bytes': (_int, [_i64, _i32, _i64p]),
    'vnd_polar_moments_f32_dev': (_int, [_p, _p, _i64, _i32, _p, _p, _i64, _p]),
    'vnd_scan_bank_f32_host': (_int, [_p, _p, _f32p, _i64, _i32, _i32, _f64p]),
    'vnd_haas_f64_dev': (_int, [_p, _p, _p, _i64, _i64, _i32, _i32, _i32, _i32, _i32, _f64, _p]),
    'vnd_haas_f64_host': (_int, [_p, _f32p, _f64p, _i64, _i64, _i32, _i32, _i32, _i32, _i32, _f64]),
    'vnd_convolve_promote_host': (_int, [_p, _i32, _i32p, _i32p, _f64p, _p, _i32, _f32p, _i64, _i64]),
    'vnd_white_noise_f32_dev': (_int, [_p, _p, _p, _p, _i64, _i64, _i32, _i32, _i32, _i32, _f64, _i32, _f32, _p, _i64, _p]),
    'vnd_host_alloc': (_int, [_i64, _pp]),
    'vnd_host_buffers_mapped': (_int, [_p, _i64, _p, _i64, _i32p]),
    'vnd_host_free': (_int, [_p]),
    'vnd_prepare_launch': (_int, [_p, _p, _i64, _i64, _i32, _i32]),
    'vnd_describe_launch': (_int, _DESCRIBE_LAUNCH_ARGS),
}

# include/vnd_amd_internal.h: measurement, tuning and diagnosis hooks (bench.py, tools/, tests) - not the drop-in ABI
INTERNAL_SIGNATURES = {
    'vnd_time_convolve_f32_dev': (_int, [_p, _p, _p, _p, _i64, _i64, _i32, _i32, _i32, _i64, _i32, _p, _f32p]),
    'vnd_time_copy_f32_dev': (_int, [_p, _p, _p, _i64, _i32, _p, _f32p]),
    'vnd_code_object_private_bytes': (_int, [_str, _i64, _str, _i64p]),
    'vnd_spec_kernel_source': (_int, [_i32, _i32p, _i32p, _f32p, _i32, _str, _i64, _i64p]),
    'vnd_window_kernel_source': (_int, [_i32, _i32p, _i32p, _f32p, _i32p, _i32p, _f32p, _i32, _i32, _i32, _i32, _str, _i64,
                                        _i64p, _i64p, _i64p]),
    'vnd_set_variant': (_int, [_p, _i32]),
    'vnd_tuning_read': (_int, [_str, _i32, _i32p]),
    'vnd_debug_read_stamps': (_int, [_p, _p, _i64, _i64, _i32, _i32, _p, _i64, _i64p]),
    'vnd_describe_stream_launch': (_int, [_p, _p, _i64, _i64, _i32, _i32, _i32, _str, _i32]),
    'vnd_describe_scan': (_int, [_p, _p, _i64, _i32, _i32, _str, _i32]),
    'vnd_describe_each_stream_launch': (_int, [_p, _p, _i64, _i64, _i64, _i64, _i32, _i32, _i32, _i32, _str, _i32]),
    'vnd_describe_voice_stream_launch': (_int, [_p, _p, _i64, _i64, _i32, _i32, _i32, _str, _i32]),
    'vnd_describe_voice_fade_stream_launch': (_int, [_p, _p, _i64, _i64, _i64, _i32, _i32, _i32, _str, _i32]),
    'vnd_describe_correlogram_voice_stream_launch': (_int, [_i64, _i32, _i32, _i32, _i64, _str, _i32]),
    'vnd_describe_polar_voice_stream_launch': (_int, [_i64, _i64, _i32, _str, _i32]),
    'vnd_describe_spectrum_voice_stream_launch': (_int, [_i64, _i32, _i32, _i32, _i32, _i64, _i32, _str, _i32]),
    'vnd_debug_decorrelate_f32_dev': (_int, _DECORRELATE_DEV_ARGS + [_i32p]),
}

# include/vnd_analysis.h: the analysis entry points, bound apart so that SIGNATURES keeps matching vnd_amd.h
ANALYSIS_SIGNATURES = {
    'vnd_correlogram_f32_dev': (_int, [_p, _p, _p, _p, _i64, _i64, _i64, _i32, _i32, _i32, _i32, _f32, _p]),
}
CORRELOGRAM_MAX_WINDOW = 16384   # VND_CORRELOGRAM_MAX_WINDOW

# include/vnd_scan.h: the optimiser's scan entry points, bound apart like the analysis ones
SCAN_SIGNATURES = {
    'vnd_haas_scan_workspace_bytes': (_int, [_i64, _i32, _i32, _i64p]),
    'vnd_haas_scan_f64_dev': (_int, [_p, _p, _i64, _i32, _p, _i32, _i32, _i32, _i32, _f64, _p, _p, _i64, _p]),
    'vnd_haas_scan_f64_host': (_int, [_p, _f32p, _i64, _i32, _i32p, _i32, _i32, _i32, _i32, _f64, _f64p]),
}

# include/vnd_haas_search.h: (signal, delay) pairs of a pool, the batched Haas-delay optimiser's unit of work
HAAS_SEARCH_SIGNATURES = {
    'vnd_haas_pairs_workspace_bytes': (_int, [_i64, _i32, _i32, _i64p]),
    'vnd_haas_pairs_f64_dev': (_int, [_p, _p, _i32, _i64, _i32, _p, _p, _i32, _i32, _i32, _i32, _f64, _p, _p, _i64, _p]),
    'vnd_haas_pairs_f64_host': (_int, [_p, _f32p, _i32, _i64, _i32, _i32p, _i32p, _i32, _i32, _i32, _i32, _f64, _f64p]),
}
HAAS_PAIRS_MAX = 1048560   # VND_HAAS_PAIRS_MAX: pairs per call

# include/vnd_velvet_search.h: (signal, candidate) pairs of a pool, the batched velvet-noise optimiser's unit of work
VELVET_SEARCH_SIGNATURES = {
    'vnd_velvet_pairs_workspace_bytes': (_int, [_i64, _i32, _i64p]),
    'vnd_velvet_pairs_f32_dev': (_int, [_p, _p, _p, _i32, _i64, _i32, _p, _p, _i32, _i32, _p, _p, _i64, _p]),
    'vnd_velvet_pairs_f32_host': (_int, [_p, _p, _f32p, _i32, _i64, _i32, _i32p, _i32p, _i32, _i32, _f64p]),
}
VELVET_PAIRS_MAX = 1048560           # VND_VELVET_PAIRS_MAX: pairs per call
VELVET_PAIRS_MAX_TAP_INDEX = 4094    # VND_VELVET_PAIRS_MAX_TAP_INDEX: the largest tap index of a bank the kernel takes
VELVET_PAIRS_TILE = 2048             # frames per workspace partial (vnd_velvet_pairs.hpp)
VELVET_BANK_MAX_CANDIDATES = 32767   # vnd_taps_create takes at most 65535 channels: two per candidate

# include/vnd_each.h: a pool through one filter or one delay per signal
_EACH_STAGE = [_i32, _i32, _f64, _i32, _f32]
_EACH_DEV_HEAD = [_p, _p, _p, _p, _p, _i32, _i64, _i32, _i32]
_EACH_HOST_HEAD = [_p, _p, _f32p, _i32p, _f32p, _i32, _i64, _i32, _i32]
EACH_SIGNATURES = {
    'vnd_convolve_each_f32_dev': (_int, _EACH_DEV_HEAD + [_p]),
    'vnd_convolve_each_f32_host': (_int, _EACH_HOST_HEAD),
    'vnd_decorrelate_each_f32_dev': (_int, _EACH_DEV_HEAD + _EACH_STAGE + [_p, _i64, _p]),
    'vnd_decorrelate_each_f32_host': (_int, _EACH_HOST_HEAD + _EACH_STAGE),
    'vnd_haas_each_f64_dev': (_int, [_p, _p, _p, _i64, _i64, _i32, _p, _i32, _i32, _i32, _i32, _f64, _p]),
    'vnd_haas_each_f64_host': (_int, [_p, _f32p, _f64p, _i64, _i64, _i32, _i32p, _i32, _i32, _i32, _i32, _f64]),
}

# include/vnd_stream.h: chunked streaming of the tap sum, bound apart like the scan and analysis entry points
_STREAM_ARGS = [_p, _p, _p, _i64, _i64, _p, _p, _i64, _i64, _i64, _i32, _i32, _i32, _i32, _i32, _f64, _i64p]
STREAM_SIGNATURES = {
    'vnd_stream_state_bytes': (_int, [_p, _i64, _i32, _i64, _i64p]),
    'vnd_stream_f32_dev': (_int, _STREAM_ARGS + [_p]),
    'vnd_stream_f32_host': (_int, _STREAM_ARGS),
}

# include/vnd_haas_stream.h: chunked streaming of the HaasEffect delay, bound apart like the tap-sum stream
_HAAS_STREAM_ARGS = [_p, _p, _i64, _i64, _p, _p, _i64, _i64, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _f64, _i64p]
HAAS_STREAM_SIGNATURES = {
    'vnd_haas_stream_state_bytes': (_int, [_i64, _i32, _i32, _i64, _i64p]),
    'vnd_haas_stream_f64_dev': (_int, _HAAS_STREAM_ARGS + [_p]),
    'vnd_haas_stream_f64_host': (_int, _HAAS_STREAM_ARGS),
}

# include/vnd_correlogram_stream.h: the cross-correlogram streamed block by block, bound apart like the other streams
CORRELOGRAM_STREAM_SIGNATURES = {
    'vnd_correlogram_stream_state_bytes': (_int, [_i64, _i32, _i64, _i64p]),
    'vnd_correlogram_stream_f32_dev': (_int, [_p, _p, _i64, _i64, _p, _p, _i64, _i32, _p, _i64, _i64, _i64, _i32, _i32, _i32,
                                              _f32, _i64p, _p]),
}

# include/vnd_each_stream.h: a pool streamed with its own filter or delay per stream
_EACH_STREAM_ARGS = [_p, _p, _p, _p, _i64, _i64, _p, _p, _i64, _i64, _i64, _i32, _i32, _i32, _i32, _i32, _f64, _i64p]
_HAAS_EACH_STREAM_ARGS = [_p, _p, _i64, _i64, _p, _p, _i64, _i64, _i64, _i32, _i32, _p, _i32, _i32, _i32, _i32, _f64, _i64p]
EACH_STREAM_SIGNATURES = {
    'vnd_each_stream_state_bytes': (_int, [_p, _i64, _i32, _i64, _i64p]),
    'vnd_each_stream_f32_dev': (_int, _EACH_STREAM_ARGS + [_p]),
    'vnd_each_stream_f32_host': (_int, _EACH_STREAM_ARGS),
    'vnd_haas_each_stream_state_bytes': (_int, [_i64, _i32, _i32, _i64, _i64p]),
    'vnd_haas_each_stream_f64_dev': (_int, _HAAS_EACH_STREAM_ARGS + [_p]),
    'vnd_haas_each_stream_f64_host': (_int, _HAAS_EACH_STREAM_ARGS),
}

# include/vnd_voice_stream.h: a voice pool - the position per slot in the device state, counts and flags per slot and call
VOICE_START, VOICE_END = 1, 2
_VOICE_STREAM_ARGS = [_p, _p, _p, _i64, _i64, _p, _p, _p, _p, _p, _p, _i64, _i32, _i32, _i32, _i32, _f64]
VOICE_STREAM_SIGNATURES = {
    'vnd_voice_stream_state_bytes': (_int, [_p, _i64, _i32, _i64, _i64p]),
    'vnd_voice_stream_reset_dev': (_int, [_p, _p, _i64, _i64, _i32, _p, _i64, _p]),
    'vnd_voice_stream_f32_dev': (_int, _VOICE_STREAM_ARGS + [_p]),
    'vnd_voice_stream_f32_host': (_int, _VOICE_STREAM_ARGS),
}

# include/vnd_voice_fade_stream.h: the voice pool whose live voices change their filter, crossfaded (the wrappers:
# _native_fade.py)
VOICE_SWITCH = 4                      # VND_VOICE_SWITCH
VOICE_FADE_MAX_FRAMES = 1 << 20       # VND_VOICE_FADE_MAX_FRAMES
VOICE_FADE_STREAM_SIGNATURES = {
    'vnd_voice_fade_stream_state_bytes': (_int, [_p, _i64, _i32, _i64, _i64, _i64p]),
    'vnd_voice_fade_stream_reset_dev': (_int, [_p, _p, _i64, _i64, _i32, _p, _i64, _i64, _p]),
    'vnd_voice_fade_stream_f32_dev': (_int, [_p, _p, _p, _i64, _i64, _i64, _p, _p, _p, _p, _p, _p, _p, _p, _i64, _i32, _i32,
                                             _i32, _i32, _f64, _p]),
}

# include/vnd_haas_voice_stream.h: the voice pool of HaasEffect delays, a delay per slot
_HAAS_VOICE_STREAM_ARGS = [_p, _p, _i64, _i64, _p, _p, _p, _p, _p, _p, _i64, _i32, _i32, _i32, _i32, _i32, _f64]
HAAS_VOICE_STREAM_SIGNATURES = {
    'vnd_haas_voice_stream_state_bytes': (_int, [_i64, _i32, _i32, _i64, _i64p]),
    'vnd_haas_voice_stream_reset_dev': (_int, [_p, _p, _i64, _i64, _i32, _i32, _i64, _p]),
    'vnd_haas_voice_stream_f64_dev': (_int, _HAAS_VOICE_STREAM_ARGS + [_p]),
    'vnd_haas_voice_stream_f64_host': (_int, _HAAS_VOICE_STREAM_ARGS),
}

# include/vnd_haas_voice_fade_stream.h: the Haas voice pool whose live voices change their delay, crossfaded (the
# wrappers: _native_haas_fade.py)
HAAS_VOICE_FADE_STREAM_SIGNATURES = {
    'vnd_haas_voice_fade_stream_state_bytes': (_int, [_i64, _i32, _i32, _i64, _i64, _i64p]),
    'vnd_haas_voice_fade_stream_reset_dev': (_int, [_p, _p, _i64, _i64, _i32, _i32, _i64, _i64, _p]),
    'vnd_haas_voice_fade_stream_f64_dev': (_int, [_p, _p, _i64, _i64, _i64, _p, _p, _p, _p, _p, _p, _p, _p, _i64, _i32, _i32,
                                                  _i32, _i32, _i32, _f64, _p]),
}

# include/vnd_correlogram_voice_stream.h: the cross-correlogram of a voice pool - positions in the device state, counts and
# flags per slot and call, float32 or float64 chunks
_CORRELOGRAM_VOICE_STREAM_ARGS = [_p, _p, _i64, _i64, _p, _p, _i64, _i32, _p, _p, _p, _p, _i64, _i32, _i32, _i32, _f32, _p]
CORRELOGRAM_VOICE_STREAM_SIGNATURES = {
    'vnd_correlogram_voice_stream_state_bytes': (_int, [_i64, _i32, _i64, _i64p]),
    'vnd_correlogram_voice_stream_reset_dev': (_int, [_p, _p, _i64, _i64, _i32, _i64, _p]),
    'vnd_correlogram_voice_stream_f32_dev': (_int, _CORRELOGRAM_VOICE_STREAM_ARGS),
    'vnd_correlogram_voice_stream_f64_dev': (_int, _CORRELOGRAM_VOICE_STREAM_ARGS),
}

# include/vnd_polar_voice_stream.h: the eight polar moments of a voice pool - positions, reduce-lane sums and the incomplete
# chunk's frames in the device state, counts and flags per slot and call, float32 or float64 chunks
_POLAR_VOICE_STREAM_ARGS = [_p, _p, _i64, _i64, _p, _p, _i64, _i32, _p, _p, _p, _p, _i64, _p]
POLAR_VOICE_STREAM_SIGNATURES = {
    'vnd_polar_voice_stream_state_bytes': (_int, [_i64, _i64, _i32, _i64p]),
    'vnd_polar_voice_stream_reset_dev': (_int, [_p, _p, _i64, _i64, _i64, _i32, _p]),
    'vnd_polar_voice_stream_f32_dev': (_int, _POLAR_VOICE_STREAM_ARGS),
    'vnd_polar_voice_stream_f64_dev': (_int, _POLAR_VOICE_STREAM_ARGS),
}

# include/vnd_scope.h: the vectorscope's data - the polar sample of every frame of a pool, and the polar and Lissajous count
# grids, float32 or float64 frames
_POLAR_COORDS_ARGS = [_p, _p, _p, _i64, _i64, _i64, _i32, _i32, _i32, _i32, _p, _p, _p, _i64, _p]
_POLAR_HIST_ARGS = [_p, _p, _p, _i64, _i64, _i64, _i32, _i32, _i32, _f64, _p, _i32, _p, _i32, _p, _p, _i32, _p, _i64, _p]
_LISSAJOUS_HIST_ARGS = [_p, _p, _p, _i64, _i64, _i64, _i32, _i64, _p, _i32, _p, _i32, _p, _p, _i32, _p]
SCOPE_SIGNATURES = {
    'vnd_scope_work_bytes': (_int, [_i64, _i64p]),
    'vnd_scope_route': (_int, [_i32, _i32, _i64, _i32p]),
    'vnd_polar_coords_f32_dev': (_int, _POLAR_COORDS_ARGS),
    'vnd_polar_coords_f64_dev': (_int, _POLAR_COORDS_ARGS),
    'vnd_polar_hist_f32_dev': (_int, _POLAR_HIST_ARGS),
    'vnd_polar_hist_f64_dev': (_int, _POLAR_HIST_ARGS),
    'vnd_lissajous_hist_f32_dev': (_int, _LISSAJOUS_HIST_ARGS),
    'vnd_lissajous_hist_f64_dev': (_int, _LISSAJOUS_HIST_ARGS),
}
SCOPE_MAX_BINS = 4096             # VND_SCOPE_MAX_BINS
SCOPE_LDS_BYTES = 163840          # VND_SCOPE_LDS_BYTES
SCOPE_SPAN_FRAMES = 32768         # VND_SCOPE_SPAN_FRAMES
SCOPE_DIRECT_SPAN_FRAMES = 4096   # VND_SCOPE_DIRECT_SPAN_FRAMES
SCOPE_ROUTE_LDS, SCOPE_ROUTE_DIRECT = 1, 2

# include/vnd_level.h: the polar level envelope - np.percentile of the radii of every angular slice of every signal
_POLAR_LEVEL_ARGS = [_p, _p, _p, _i64, _i64, _i64, _i32, _i32, _i32, _f64, _p, _i32, _f64p, _i32, _p, _p, _p, _p, _i64, _p]
LEVEL_SIGNATURES = {
    'vnd_polar_level_work_bytes': (_int, [_i64, _i64, _i32, _i32, _i32, _i64p]),
    'vnd_polar_level_f32_dev': (_int, _POLAR_LEVEL_ARGS),
    'vnd_polar_level_f64_dev': (_int, _POLAR_LEVEL_ARGS),
}
LEVEL_MAX_PERCENTILES = 4         # VND_LEVEL_MAX_PERCENTILES
LEVEL_MAX_BINS = 1024             # VND_LEVEL_MAX_BINS
LEVEL_SPAN_FRAMES = 32768         # VND_LEVEL_SPAN_FRAMES

# include/vnd_spectrum.h: short-time spectra of a pool - spectrogram columns and the Welch sums Pxx, Pyy, Pxy
_SPECTRUM_ARGS = [_p, _p, _i64, _i64, _i64, _i32, _i32, _p, _p, _i32, _i32, _i32, _i32, _f64, _p]
_SPECTROGRAM_ARGS = _SPECTRUM_ARGS + [_p, _p]
_CROSS_SPECTRA_ARGS = _SPECTRUM_ARGS + [_p, _p, _p, _p, _i64, _p]
SPECTRUM_SIGNATURES = {
    'vnd_spectrum_run_length': (_int, [_i32, _i32, _i32, _i32, _i32, _i32p]),
    'vnd_cross_spectra_work_bytes': (_int, [_i64, _i64, _i32, _i32, _i32, _i32, _i32, _i64p]),
    'vnd_spectrogram_f32_dev': (_int, _SPECTROGRAM_ARGS),
    'vnd_spectrogram_f64_dev': (_int, _SPECTROGRAM_ARGS),
    'vnd_cross_spectra_f32_dev': (_int, _CROSS_SPECTRA_ARGS),
    'vnd_cross_spectra_f64_dev': (_int, _CROSS_SPECTRA_ARGS),
}
SPECTRUM_MIN_NFFT = 64            # VND_SPECTRUM_MIN_NFFT
SPECTRUM_MAX_NFFT = 4096          # VND_SPECTRUM_MAX_NFFT
SPECTRUM_RUN = 32                 # VND_SPECTRUM_RUN

# include/vnd_spectrum_voice_stream.h: the short-time spectra of a voice pool - positions, Welch sums and the ring in the
# device state, counts and flags per slot and call, float32 or float64 chunks
_SPECTRUM_VOICE_STREAM_ARGS = [_p, _p, _i64, _i64, _p, _i64, _i32, _i32, _p, _p, _p, _p, _i32, _i32, _i32, _i32, _f64, _p, _p,
                               _p, _p, _p, _p, _i64, _p]
SPECTRUM_VOICE_STREAM_SIGNATURES = {
    'vnd_spectrum_voice_stream_state_bytes': (_int, [_i64, _i32, _i32, _i32, _i32, _i64, _i32, _i64p]),
    'vnd_spectrum_voice_stream_reset_dev': (_int, [_p, _p, _i64, _i64, _i32, _i32, _i32, _i32, _i64, _i32, _p]),
    'vnd_spectrum_voice_stream_f32_dev': (_int, _SPECTRUM_VOICE_STREAM_ARGS),
    'vnd_spectrum_voice_stream_f64_dev': (_int, _SPECTRUM_VOICE_STREAM_ARGS),
}

# include/vnd_scope_voice_stream.h: the vectorscope of a voice pool - positions and the ring of cells in the device state, the
# count grids in caller-owned memory that belongs to the pool between calls, whole-voice or over a sliding window
_SCOPE_VOICE_HEAD_ARGS = [_p, _p, _i64, _i64, _i64, _p, _p, _i64, _i32, _p, _p]
_SCOPE_VOICE_TAIL_ARGS = [_p, _i32, _p, _i32, _p, _p, _i64, _p]
_POLAR_HIST_VOICE_ARGS = _SCOPE_VOICE_HEAD_ARGS + [_i32, _i32, _f64] + _SCOPE_VOICE_TAIL_ARGS
_LISSAJOUS_HIST_VOICE_ARGS = _SCOPE_VOICE_HEAD_ARGS + _SCOPE_VOICE_TAIL_ARGS
SCOPE_VOICE_STREAM_SIGNATURES = {
    'vnd_scope_voice_stream_state_bytes': (_int, [_i64, _i64, _i64, _i64p]),
    'vnd_scope_voice_stream_reset_dev': (_int, [_p, _p, _i64, _i64, _i64, _i64, _p]),
    'vnd_polar_hist_voice_stream_f32_dev': (_int, _POLAR_HIST_VOICE_ARGS),
    'vnd_polar_hist_voice_stream_f64_dev': (_int, _POLAR_HIST_VOICE_ARGS),
    'vnd_lissajous_hist_voice_stream_f32_dev': (_int, _LISSAJOUS_HIST_VOICE_ARGS),
    'vnd_lissajous_hist_voice_stream_f64_dev': (_int, _LISSAJOUS_HIST_VOICE_ARGS),
}
SCOPE_VOICE_SPAN_FRAMES = 1024    # kScopeVoiceSpan: frames of one slot per workgroup of the bin kernel

# include/vnd_polar_level_voice_stream.h: the level envelope of a voice pool - positions, fills and the rings of keys and
# slices in the device state; a push per block, the levels from the state alone
_LEVEL_VOICE_PUSH_ARGS = [_p, _p, _i64, _i64, _i64, _p, _p, _i64, _i32, _p, _p, _i32, _i32, _f64, _p, _i32, _p, _i64, _p]
_LEVEL_VOICE_LEVELS_ARGS = [_p, _p, _i64, _i64, _i64, _i32, _f64p, _i32, _p, _p, _p, _i64, _i64, _p]
LEVEL_VOICE_STREAM_SIGNATURES = {
    'vnd_polar_level_voice_stream_state_bytes': (_int, [_i64, _i64, _i64, _i32, _i64p]),
    'vnd_polar_level_voice_stream_reset_dev': (_int, [_p, _p, _i64, _i64, _i64, _i64, _i32, _p]),
    'vnd_polar_level_voice_stream_push_f32_dev': (_int, _LEVEL_VOICE_PUSH_ARGS),
    'vnd_polar_level_voice_stream_push_f64_dev': (_int, _LEVEL_VOICE_PUSH_ARGS),
    'vnd_polar_level_voice_stream_work_bytes': (_int, [_i64, _i64, _i32, _i32, _i32, _i64p]),
    'vnd_polar_level_voice_stream_levels_f32_dev': (_int, _LEVEL_VOICE_LEVELS_ARGS),
    'vnd_polar_level_voice_stream_levels_f64_dev': (_int, _LEVEL_VOICE_LEVELS_ARGS),
}

# include/vnd_haas_scan_voice_stream.h: the Haas-delay scan of a voice pool - positions, fills, heads and the ring of input
# frames in the device state; a push per block, (slot, delay) pairs scored from the state alone (wrappers: _native_haas_scan_voice.py)
HAAS_SCAN_VOICE_STREAM_SIGNATURES = {
    'vnd_haas_scan_voice_stream_state_bytes': (_int, [_i64, _i64, _i64, _i32, _i64p]),
    'vnd_haas_scan_voice_stream_reset_dev': (_int, [_p, _p, _i64, _i64, _i64, _i64, _i32, _p]),
    'vnd_haas_scan_voice_stream_push_f32_dev': (_int, [_p, _p, _i64, _i64, _i64, _p, _i32, _p, _p, _p, _i64, _p]),
    'vnd_haas_scan_voice_stream_workspace_bytes': (_int, [_i64, _i32, _i32, _i64p]),
    'vnd_haas_scan_voice_stream_pairs_f64_dev': (_int, [_p, _p, _i64, _i64, _i64, _i32, _i64, _p, _p, _i32, _i32, _i32, _i32, _i32,
                                                        _f64, _p, _p, _i64, _p]),
}

# header under include/ -> its table: load_library declares all of them, and a new header is one line here
HEADERS = {
    'vnd_amd.h': SIGNATURES,
    'vnd_amd_internal.h': INTERNAL_SIGNATURES,
    'vnd_analysis.h': ANALYSIS_SIGNATURES,
    'vnd_scan.h': SCAN_SIGNATURES,
    'vnd_haas_search.h': HAAS_SEARCH_SIGNATURES,
    'vnd_velvet_search.h': VELVET_SEARCH_SIGNATURES,
    'vnd_each.h': EACH_SIGNATURES,
    'vnd_stream.h': STREAM_SIGNATURES,
    'vnd_haas_stream.h': HAAS_STREAM_SIGNATURES,
    'vnd_correlogram_stream.h': CORRELOGRAM_STREAM_SIGNATURES,
    'vnd_each_stream.h': EACH_STREAM_SIGNATURES,
    'vnd_voice_stream.h': VOICE_STREAM_SIGNATURES,
    'vnd_voice_fade_stream.h': VOICE_FADE_STREAM_SIGNATURES,
    'vnd_haas_voice_stream.h': HAAS_VOICE_STREAM_SIGNATURES,
    'vnd_haas_voice_fade_stream.h': HAAS_VOICE_FADE_STREAM_SIGNATURES,
    'vnd_correlogram_voice_stream.h': CORRELOGRAM_VOICE_STREAM_SIGNATURES,
    'vnd_polar_voice_stream.h': POLAR_VOICE_STREAM_SIGNATURES,
    'vnd_scope.h': SCOPE_SIGNATURES,
    'vnd_level.h': LEVEL_SIGNATURES,
    'vnd_spectrum.h': SPECTRUM_SIGNATURES,
    'vnd_spectrum_voice_stream.h': SPECTRUM_VOICE_STREAM_SIGNATURES,
    'vnd_scope_voice_stream.h': SCOPE_VOICE_STREAM_SIGNATURES,
    'vnd_polar_level_voice_stream.h': LEVEL_VOICE_STREAM_SIGNATURES,
    'vnd_haas_scan_voice_stream.h': HAAS_SCAN_VOICE_STREAM_SIGNATURES,
}

_lib = None
_lib_lock = threading.Lock()


def _preload_hip_runtime() -> None:
    """Keep ONE HIP runtime in the process.

    PyTorch-ROCm wheels bundle their own ``libamdhip64.so`` (soname
    ``libamdhip64.so.7``) and ask for it by the unversioned name, so if this
    extension pulled in ``/opt/rocm``'s copy first, a later ``import torch`` would
    map a second runtime and see no GPUs.  When torch is installed but not yet
    imported, map its runtime first: our NEEDED ``libamdhip64.so.7`` then binds
    to it by soname, and torch later finds the same file already loaded.
    """
    try:
        with open('/proc/self/maps') as maps:
            if any('libamdhip64' in line for line in maps):
                return
    except OSError:
        pass
    import importlib.util
    spec = importlib.util.find_spec('torch')
    if spec is None or not spec.submodule_search_locations:
        return
    cand = pathlib.Path(list(spec.submodule_search_locations)[0]) / 'lib' / 'libamdhip64.so'
    if cand.exists():
        ctypes.CDLL(str(cand), mode=ctypes.RTLD_GLOBAL)


class NativeError(RuntimeError):
    """The HIP extension is missing or a device call failed."""


def load_library():
    """dlopen the in-tree extension and declare every prototype of every header in ``HEADERS``."""
    global _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        if not LIB_PATH.exists():
            raise NativeError(
                f'{LIB_PATH} is missing: build it with `python -c "import __graft_entry__ as g; '
                f'g.build()"` (hipcc --offload-arch=gfx950).  vndecorrelate_amd has no CPU fallback.')
        _preload_hip_runtime()
        lib = ctypes.CDLL(str(LIB_PATH))
        for table in HEADERS.values():
            for name, (res, args) in table.items():
                fn = getattr(lib, name)
                fn.restype = res
                fn.argtypes = args
        got = lib.vnd_abi_version()
        if got != ABI_VERSION:
            raise NativeError(f'{LIB_PATH} has ABI {got}, expected {ABI_VERSION}: rebuild it')
        _lib = lib
        return lib


def shard_range(total: int, world_size: int, rank: int):
    """``vnd_shard_range``: ``(first, count)`` of ``rank``'s contiguous block of ``total`` streams."""
    first, count = ctypes.c_int64(), ctypes.c_int64()
    _call(load_library(), 'vnd_shard_range', total, world_size, rank, ctypes.byref(first), ctypes.byref(count))
    return first.value, count.value


def _check(rc: int, what: str):
    if rc == 0:
        return
    msg = load_library().vnd_last_error().decode(errors='replace')
    if rc == 1:
        raise ValueError(f'{what}: {msg}')
    raise NativeError(f'{what} failed (status {rc}): {msg}')


def _ptr(a: Optional[np.ndarray], ctype):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctype))


# ---- the one call path: every wrapper below goes through _call, by the C function's name ----------------------------------
def _call(lib, name: str, *args):
    """``lib.<name>(*args)``, its status checked under the same name.  The function is the attribute the ``CDLL`` caches."""
    _check(getattr(lib, name)(*args), name)


def _query(lib, name: str, *args, out=ctypes.c_int64, then=()):
    """A call that answers through an out-parameter behind ``args`` (``then``: what follows it): a byte count, a frame or
    row count, or with ``out`` another type.  Returns the value."""
    value = out()
    _call(lib, name, *args, ctypes.byref(value), *then)
    return value.value


def _describe(lib, name: str, *args) -> str:
    """A ``vnd_describe_*`` call: the text it writes into a buffer of 512 bytes."""
    buf = ctypes.create_string_buffer(512)
    _call(lib, name, *args, buf, 512)
    return buf.value.decode()


def _width(width, *stage):
    """``use_width, width`` as the C ABI takes them; with ``normalize, eps`` given, the decorrelate stage's tail behind them."""
    if not stage:
        return width is not None, float(width or 0.0)
    normalize, eps = stage
    return width is not None, float(width or 0.0), int(normalize), float(eps)


def _typed(name: str, float64: bool) -> str:
    """``name`` with its ``{}`` filled by the sample type: ``f64`` or ``f32``."""
    return name.format('f64' if float64 else 'f32')


class _PinnedPool:
    """Result arrays of the host API in page-locked memory (``vnd_host_alloc``).

    The reference allocates its result afresh in every call (decorrelation.py:647); a fresh pageable
    array of hundreds of MB costs tens of milliseconds of page faults and a staged download.  Blocks
    are recycled when the NumPy array (and every view of it) is garbage-collected; the pool keeps at
    most ``VND_PINNED_POOL_MB`` (default 2048; 0 turns it off) of idle blocks.  Results below 1 MiB stay
    ordinary NumPy arrays."""

    MIN_BYTES = 1 << 20

    def __init__(self):
        self._lock = threading.Lock()
        self._free: dict = {}            # rounded size -> [ptr, ...]
        self._idle = 0
        self.limit = int(os.environ.get('VND_PINNED_POOL_MB', '2048')) << 20
        self.hits = self.misses = 0

    @staticmethod
    def _round(nbytes: int) -> int:
        size = 1 << 20
        while size < nbytes:
            size <<= 1
        return size if size - nbytes <= nbytes // 4 else ((nbytes + (1 << 20) - 1) >> 20) << 20

    def empty(self, shape, dtype=np.float32) -> np.ndarray:
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        if self.limit <= 0 or nbytes < self.MIN_BYTES:
            return np.empty(shape, dtype)
        size = self._round(nbytes)
        ptr = None
        with self._lock:
            blocks = self._free.get(size)
            if blocks:
                ptr = blocks.pop()
                self._idle -= size
                self.hits += 1
        if ptr is None:
            h = ctypes.c_void_p()
            try:
                rc = load_library().vnd_host_alloc(size, ctypes.byref(h))
            except Exception:
                rc = 1
            if rc != 0 or not h.value:
                return np.empty(shape, dtype)          # no pinned memory to be had: an ordinary array
            ptr = h.value
            self.misses += 1
        buf = (ctypes.c_char * nbytes).from_address(ptr)
        weakref.finalize(buf, self._release, ptr, size)
        return np.frombuffer(buf, dtype=dtype).reshape(shape)

    def _release(self, ptr: int, size: int):
        with self._lock:
            if self._idle + size <= self.limit:
                self._free.setdefault(size, []).append(ptr)
                self._idle += size
                return
        try:
            load_library().vnd_host_free(ptr)
        except Exception:
            pass

    def trim(self):
        with self._lock:
            blocks = [p for v in self._free.values() for p in v]
            self._free.clear()
            self._idle = 0
        for p in blocks:
            load_library().vnd_host_free(p)


pinned_pool = _PinnedPool()


class Context:
    """One per (process, device): owns the stream and staging buffers of the
    synchronous host-pointer calls.  Thread-safe: the library holds a per-context
    mutex across every ``*_host`` entry point (ctypes drops the GIL during the call),
    so concurrent callers are serialised, never interleaved; use one Context per
    thread for host calls that should overlap."""

    def __init__(self, device: int = 0):
        lib = load_library()
        h = ctypes.c_void_p()
        _call(lib, 'vnd_ctx_create', int(device), ctypes.byref(h))
        self._lib = lib
        self._h = h
        self.device = int(device)

    def close(self):
        if getattr(self, '_h', None):
            self._lib.vnd_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        if not self._h:
            raise NativeError('context is closed')
        return self._h

    def info(self) -> dict:
        name = ctypes.create_string_buffer(256)
        cus, lds = ctypes.c_int32(), ctypes.c_int32()
        hbm = ctypes.c_int64()
        _call(self._lib, 'vnd_ctx_info', self.handle, name, 256, ctypes.byref(cus), ctypes.byref(hbm), ctypes.byref(lds))
        return {'name': name.value.decode(), 'compute_units': cus.value, 'hbm_bytes': hbm.value,
                'lds_bytes': lds.value}

    def set_variant(self, variant: int):
        _call(self._lib, 'vnd_set_variant', self.handle, int(variant))

    def time_copy(self, x_ptr: int, y_ptr: int, elems: int, iters: int = 10, stream: int = 0) -> float:
        """Average kernel milliseconds of a plain streaming copy of ``elems`` floats (``vnd_time_copy_f32_dev``:
        the box's streaming ceiling for bench.py; not on the data path)."""
        return _query(self._lib, 'vnd_time_copy_f32_dev', self.handle, x_ptr, y_ptr, int(elems), int(iters), stream,
                      out=ctypes.c_float)


class TapTable:
    """Device-resident, immutable tap table (``vnd_taps``)."""

    def __init__(self, ctx: Context, handle):
        self.ctx = ctx
        self._lib = ctx._lib
        self._h = handle
        c, t, m = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        _call(self._lib, 'vnd_taps_info', handle, ctypes.byref(c), ctypes.byref(t), ctypes.byref(m))
        self.num_channels, self.total_taps, self.max_index = c.value, t.value, m.value

    @classmethod
    def create(cls, ctx: Context, tap_offsets, tap_index, tap_weight, *, seg_offsets=None,
               seg_end=None, seg_gain=None, chan_flags=None, apply_gain=False) -> 'TapTable':
        """The arrays of ``vnd_taps_create`` (include/vnd_amd.h).  The C side reads ``tap_offsets[-1]`` taps and
        ``seg_offsets[-1]`` segments through bare pointers: arrays shorter than that are refused here, before the call
        (``tap_index`` / ``tap_weight`` may be ``None`` for a table without taps)."""
        tap_offsets = np.ascontiguousarray(tap_offsets, np.int32).ravel()
        tap_index = None if tap_index is None else np.ascontiguousarray(tap_index, np.int32).ravel()
        tap_weight = None if tap_weight is None else np.ascontiguousarray(tap_weight, np.float32).ravel()
        channels = len(tap_offsets) - 1
        if channels < 1:
            raise ValueError('tap_offsets needs one entry per channel and one more')
        total = int(tap_offsets[-1])
        for name, a in (('tap_index', tap_index), ('tap_weight', tap_weight)):
            if (0 if a is None else len(a)) < total:
                raise ValueError(f'{name} holds {0 if a is None else len(a)} entries, tap_offsets[-1] asks for {total}')
        if seg_offsets is not None:
            if seg_end is None or seg_gain is None:
                raise ValueError('seg_offsets comes with seg_end and seg_gain')
            seg_offsets = np.ascontiguousarray(seg_offsets, np.int32).ravel()
            seg_end = np.ascontiguousarray(seg_end, np.int32).ravel()
            seg_gain = np.ascontiguousarray(seg_gain, np.float32).ravel()
            if len(seg_offsets) != len(tap_offsets):
                raise ValueError(f'seg_offsets has {len(seg_offsets)} entries, tap_offsets {len(tap_offsets)}')
            segs = int(seg_offsets[-1])
            for name, a in (('seg_end', seg_end), ('seg_gain', seg_gain)):
                if len(a) < segs:
                    raise ValueError(f'{name} holds {len(a)} entries, seg_offsets[-1] asks for {segs}')
        if chan_flags is not None:
            chan_flags = np.ascontiguousarray(chan_flags, np.uint8).ravel()
            if len(chan_flags) < channels:
                raise ValueError(f'chan_flags holds {len(chan_flags)} entries for {channels} channels')
        h = ctypes.c_void_p()
        _call(ctx._lib, 'vnd_taps_create', ctx.handle, channels, _ptr(tap_offsets, _i32), _ptr(tap_index, _i32),
              _ptr(tap_weight, _f32), _ptr(seg_offsets, _i32), _ptr(seg_end, _i32), _ptr(seg_gain, _f32),
              _ptr(chan_flags, ctypes.c_uint8), bool(apply_gain), ctypes.byref(h))
        return cls(ctx, h)

    @classmethod
    def from_bytes(cls, ctx: Context, image: bytes) -> 'TapTable':
        image = bytes(image)
        if not image:
            raise ValueError('empty tap image')
        buf = ctypes.create_string_buffer(image, len(image))       # (its own copy, aligned for the words the C side reads in place)
        h = ctypes.c_void_p()
        _call(ctx._lib, 'vnd_taps_deserialize', ctx.handle, buf, len(image), ctypes.byref(h))
        return cls(ctx, h)

    @classmethod
    def broadcast_rccl(cls, ctx: 'Context', table: Optional['TapTable'], root: int, rank: int, comm: int,
                       stream: int = 0) -> 'TapTable':
        """The C ABI's own table broadcast over an RCCL communicator (``ncclComm_t`` as an integer) - for
        hosts that shard without torch.distributed.  ``table`` is needed on ``root`` only; every rank
        returns a table on its device (the root its own)."""
        h = ctypes.c_void_p((table._h.value if isinstance(table._h, ctypes.c_void_p) else table._h) if (table is not None and rank == root) else None)
        _call(ctx._lib, 'vnd_taps_broadcast_rccl', ctx.handle, ctypes.byref(h), root, rank, comm, stream)
        return table if rank == root else cls(ctx, h)

    def to_bytes(self) -> bytes:
        need = _query(self._lib, 'vnd_taps_serialize', self.handle, None, 0)
        buf = ctypes.create_string_buffer(need)
        need = _query(self._lib, 'vnd_taps_serialize', self.handle, buf, need)
        return buf.raw[:need]

    @property
    def handle(self):
        if not self._h:
            raise NativeError('tap table is closed')
        return self._h

    def close(self):
        if getattr(self, '_h', None):
            self._lib.vnd_taps_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- the hot path ---------------------------------------------------------
    # A signal with fewer channels than the table is fanned out: output channel c reads
    # input channel c % in_channels (vnd_*_fanout_*; mono -> stereo, or one signal through
    # a bank of filters).  The result always has the table's channel count.
    def _fanned(self, name: str, channels: int) -> str:
        """``name`` with its ``{}`` filled for a signal of ``channels`` channels: empty, or ``fanout_``."""
        return name.format('' if channels == self.num_channels else 'fanout_')

    def _host_shapes(self, x: np.ndarray, what: str, out: Optional[np.ndarray] = None):
        if x.dtype != np.float32 or not x.flags.c_contiguous:
            raise ValueError(f'{what} wants a C-contiguous float32 array')
        if x.ndim == 2:
            batch, (n, c) = 1, x.shape
        elif x.ndim == 3:
            batch, n, c = x.shape
        else:
            raise ValueError(f'expected (n, C) or (batch, n, C), got {x.shape}')
        shape = x.shape[:-1] + (self.num_channels,)
        if out is None:
            y = pinned_pool.empty(shape, np.float32)
        else:                                   # the caller's block of a larger result (multi.DevicePool): written in place
            if out.dtype != np.float32 or not out.flags.c_contiguous or out.shape != shape:
                raise ValueError(f'{what}: out must be a C-contiguous float32 array of shape {shape}')
            y = out
        return batch, n, c, y

    def convolve_host(self, x: np.ndarray, mode: int = MODE_EXACT, *, out: Optional[np.ndarray] = None) -> np.ndarray:
        """x: C-contiguous float32 ``(n, C)`` or ``(batch, n, C)``; returns a new array (or ``out``, filled)."""
        batch, n, c, y = self._host_shapes(x, 'convolve_host', out)
        _call(self._lib, self._fanned('vnd_convolve_{}f32_host', c), self.ctx.handle, self.handle, _ptr(x, _f32), _ptr(y, _f32),
              batch, n, c, int(mode))
        return y

    def decorrelate_host(self, x: np.ndarray, mode: int = MODE_EXACT, *, ms_encode: bool, width,
                         normalize, eps: float = 1e-10, out: Optional[np.ndarray] = None) -> np.ndarray:
        """Convolution + decorrelate epilogue on the device; x as in ``convolve_host``.
        ``normalize``: False/True or one of the ``NORMALIZE_*`` values."""
        batch, n, c, y = self._host_shapes(x, 'decorrelate_host', out)
        if batch > MAX_STREAMS_PER_CALL:
            for first in range(0, batch, MAX_STREAMS_PER_CALL):
                self.decorrelate_host(x[first:first + MAX_STREAMS_PER_CALL], mode, ms_encode=ms_encode, width=width,
                                      normalize=normalize, eps=eps, out=y[first:first + MAX_STREAMS_PER_CALL])
            return y
        _call(self._lib, self._fanned('vnd_decorrelate_{}f32_host', c), self.ctx.handle, self.handle, _ptr(x, _f32),
              _ptr(y, _f32), batch, n, c, int(mode), bool(ms_encode), *_width(width, normalize, eps))
        return y

    def _decorrelate_args(self, x_ptr, y_ptr, batch, n, channels, mode, ms_encode, width, normalize, eps, workspace_ptr,
                          workspace_bytes, stream):
        return (self.ctx.handle, self.handle, x_ptr, y_ptr, batch, n, channels, int(mode), bool(ms_encode),
                *_width(width, normalize, eps), workspace_ptr, workspace_bytes, stream)

    def decorrelate_device(self, x_ptr: int, y_ptr: int, batch: int, n: int, channels: int, *, mode: int,
                           ms_encode: bool, width, normalize: bool, workspace_ptr: int, workspace_bytes: int,
                           eps: float = 1e-10, stream: int = 0):
        """``channels`` = channels of x; y has the table's channel count."""
        _call(self._lib, self._fanned('vnd_decorrelate_{}f32_dev', channels),
              *self._decorrelate_args(x_ptr, y_ptr, batch, n, channels, mode, ms_encode, width, normalize, eps, workspace_ptr,
                                      workspace_bytes, stream))

    def decorrelate_device_taken(self, x_ptr: int, y_ptr: int, batch: int, n: int, channels: int, *, mode: int,
                                 ms_encode: bool, width, normalize: int, workspace_ptr: int, workspace_bytes: int,
                                 eps: float = 1e-10, stream: int = 0) -> dict:
        """``decorrelate_device``, and which form of the stage ran (``vnd_debug_decorrelate_f32_dev``; tests only):
        ``branch`` ('table-order', 'fused', 'q_done' or None when nothing ran), ``conv_path`` (0 a generic kernel, 1 the
        per-table kernel leaving the sums, 2 the per-table kernel without them), ``numpy_order`` and ``blk_done``."""
        taken = np.zeros(4, np.int32)
        _call(self._lib, 'vnd_debug_decorrelate_f32_dev',
              *self._decorrelate_args(x_ptr, y_ptr, batch, n, channels, mode, ms_encode, width, normalize, eps, workspace_ptr,
                                      workspace_bytes, stream), _ptr(taken, _i32))
        branch = {-1: None, 0: 'table-order', 1: 'fused', 2: 'q_done'}[int(taken[0])]
        return dict(branch=branch, conv_path=int(taken[1]), numpy_order=bool(taken[2]), blk_done=bool(taken[3]))

    def convolve_device(self, x_ptr: int, y_ptr: int, batch: int, n: int, channels: int,
                        mode: int = MODE_EXACT, stream: int = 0):
        """Enqueue on ``stream`` (a hipStream_t as int); pointers are device addresses.
        ``channels`` = channels of x; y has the table's channel count."""
        _call(self._lib, self._fanned('vnd_convolve_{}f32_dev', channels), self.ctx.handle, self.handle, x_ptr, y_ptr, batch, n,
              channels, int(mode), stream)

    def scan_host(self, x: np.ndarray, mode: int = MODE_EXACT) -> np.ndarray:
        """Candidate scan: this table is a bank of F stereo pairs, ``x`` a ``(n, 1)`` or
        ``(n, 2)`` float32 signal; returns ``(F, 8)`` float64 polar moments (``vnd_amd.h``)."""
        if x.dtype != np.float32 or not x.flags.c_contiguous or x.ndim != 2:
            raise ValueError('scan_host wants a C-contiguous float32 (n, channels) array')
        out = np.zeros((self.num_channels // 2, MOMENTS), np.float64)
        _call(self._lib, 'vnd_scan_bank_f32_host', self.ctx.handle, self.handle, _ptr(x, _f32), x.shape[0], x.shape[1],
              int(mode), _ptr(out, _f64))
        return out

    def time_device(self, x_ptr: int, y_ptr: int, batch: int, n: int, channels: int, *, mode: int,
                    n_buffers: int, stride_elems: int, iters: int, stream: int = 0) -> float:
        """Average milliseconds per launch between two hipEvents on ``stream``."""
        return _query(self._lib, 'vnd_time_convolve_f32_dev', self.ctx.handle, self.handle, x_ptr, y_ptr, batch, n, channels,
                      int(mode), n_buffers, stride_elems, iters, stream, out=ctypes.c_float)

    def prepare(self, batch: int, n: int, channels: int, mode: int = MODE_EXACT) -> None:
        """Build now the per-table kernel that launches of this shape would use (``vnd_prepare_launch``): small
        launches never trigger a build themselves, so a host that repeats one small shape prepares it once."""
        _call(self._lib, 'vnd_prepare_launch', self.ctx.handle, self.handle, batch, n, channels, int(mode))

    def describe(self, batch: int, n: int, channels: int, mode: int = MODE_EXACT) -> str:
        return _describe(self._lib, self._fanned('vnd_describe_{}launch', channels), self.ctx.handle, self.handle, batch, n,
                         channels, int(mode))

    def describe_stream(self, batch: int, n_out: int, in_channels: int, mode: int = MODE_EXACT,
                        epilogue: bool = False) -> str:
        """The plan of a ``vnd_stream_f32_dev`` call with ``n_out`` output frames per stream
        (``vnd_describe_stream_launch``)."""
        return _describe(self._lib, 'vnd_describe_stream_launch', self.ctx.handle, self.handle, batch, n_out, in_channels,
                         int(mode), bool(epilogue))

    def describe_scan(self, n: int, in_channels: int, mode: int = MODE_EXACT) -> str:
        """The route ``scan_host`` takes for an ``(n, in_channels)`` signal (``vnd_describe_scan``; no device work): the
        text starts with ``fused`` or ``unfused by_frame`` / ``unfused by_candidate``, then names the convolution's kernel
        and carries ``cg=``, ``r=``, ``nt=``, ``bc=``, ``tiles=``, ``direct=`` among its fields."""
        return _describe(self._lib, 'vnd_describe_scan', self.ctx.handle, self.handle, n, in_channels, int(mode))

    def describe_each_stream(self, max_frames_per_call: int, batch: int, position: int, n_in: int, in_channels: int,
                             final: bool = False, mode: int = MODE_EXACT, epilogue: bool = False) -> str:
        """The launch of a ``vnd_each_stream_f32_dev`` call with these arguments on this bank
        (``vnd_describe_each_stream_launch``): ``r=``, ``tiles=``, ``nblocks=`` among its fields."""
        return _describe(self._lib, 'vnd_describe_each_stream_launch', self.ctx.handle, self.handle, max_frames_per_call, batch,
                         position, n_in, in_channels, bool(final), int(mode), bool(epilogue))

    def describe_voice_stream(self, max_frames_per_call: int, slots: int, in_channels: int, mode: int = MODE_EXACT,
                              epilogue: bool = False) -> str:
        """The launch of every ``vnd_voice_stream_f32_dev`` call on a pool of ``slots`` voices over this bank
        (``vnd_describe_voice_stream_launch``): ``r=``, ``tiles=``, ``nblocks=``, ``advance_groups=`` among its fields."""
        return _describe(self._lib, 'vnd_describe_voice_stream_launch', self.ctx.handle, self.handle, max_frames_per_call,
                         slots, in_channels, int(mode), bool(epilogue))

    def read_stamps(self, batch: int, n: int, channels: int, mode: int = MODE_EXACT) -> np.ndarray:
        """Phase stamps of the window-form kernel of this launch shape (``vnd_debug_read_stamps``; diagnosis builds
        under ``VND_TUNING=1 VND_WIN_STAMPS=<workgroups>``): ``(workgroups, 16)`` uint64, empty without such a build."""
        shape = (self.ctx.handle, self.handle, batch, n, channels, int(mode))
        count = _query(self._lib, 'vnd_debug_read_stamps', *shape, None, 0)
        out = np.zeros(count, np.uint64)
        if count:
            _query(self._lib, 'vnd_debug_read_stamps', *shape, out.ctypes.data, count)
        return out.reshape(-1, 16)


def decorrelate_workspace_bytes(batch: int, n: int, channels: int) -> int:
    return _query(load_library(), 'vnd_decorrelate_workspace_bytes', batch, n, channels)


def convolve_promote_host(ctx: 'Context', x: np.ndarray, tap_offsets: np.ndarray, tap_index: np.ndarray,
                          tap_weight: np.ndarray) -> np.ndarray:
    """The function path on operands NumPy promotes to float64 (``vnd_convolve_promote_host``):
    x float32 or float64 ``(n, C)`` / ``(batch, n, C)``, float64 weights; float32 result."""
    if x.dtype not in (np.float32, np.float64) or not x.flags.c_contiguous or x.ndim not in (2, 3):
        raise ValueError('convolve_promote_host wants a C-contiguous float32/float64 (n, C) or (batch, n, C) array')
    batch = 1 if x.ndim == 2 else x.shape[0]
    n, c = x.shape[-2:]
    offs = np.ascontiguousarray(tap_offsets, np.int32)
    idx = np.ascontiguousarray(tap_index, np.int32)
    w = np.ascontiguousarray(tap_weight, np.float64)
    y = np.empty(x.shape, np.float32)
    _call(ctx._lib, 'vnd_convolve_promote_host', ctx.handle, c, _ptr(offs, _i32), _ptr(idx, _i32), _ptr(w, _f64), x.ctypes.data,
          int(x.dtype == np.float64), _ptr(y, _f32), batch, n)
    return y


def haas_host(ctx: 'Context', x: np.ndarray, *, delay: int, delayed_channel: int, ms_mode: bool, width) -> np.ndarray:
    """HaasEffect on the device from host memory: x float32 ``(n, 1|2)`` or ``(batch, n, 1|2)``;
    returns float64 ``(..., n + delay, 2)``."""
    if x.dtype != np.float32 or not x.flags.c_contiguous or x.ndim not in (2, 3):
        raise ValueError('haas_host wants a C-contiguous float32 (n, C) or (batch, n, C) array')
    batch = 1 if x.ndim == 2 else x.shape[0]
    n, c = x.shape[-2:]
    y = np.empty(x.shape[:-2] + (n + int(delay), 2), np.float64)
    _call(ctx._lib, 'vnd_haas_f64_host', ctx.handle, _ptr(x, _f32), _ptr(y, _f64), batch, n, c, int(delay),
          int(delayed_channel), bool(ms_mode), *_width(width))
    return y


def haas_device(ctx: 'Context', x_ptr: int, y_ptr: int, batch: int, n: int, channels: int, *, delay: int,
                delayed_channel: int, ms_mode: bool, width, stream: int = 0):
    _call(ctx._lib, 'vnd_haas_f64_dev', ctx.handle, x_ptr, y_ptr, batch, n, channels, int(delay), int(delayed_channel),
          bool(ms_mode), *_width(width), stream)


def white_noise_device(ctx: 'Context', x_ptr: int, h_ptr: int, y_ptr: int, batch: int, n: int, in_channels: int,
                       channels: int, fir_length: int, *, width, normalize: int, workspace_ptr: int = 0,
                       workspace_bytes: int = 0, eps: float = 1e-10, stream: int = 0):
    """``vnd_white_noise_f32_dev``: WhiteNoise's dense float64 FIR (+ width, + normaliser) on device buffers, enqueued on
    ``stream``.  x float32 ``(batch, n, in_channels)``, h float64 ``(fir_length, channels)``, y float32 ``(batch, n, channels)``."""
    _call(ctx._lib, 'vnd_white_noise_f32_dev', ctx.handle, x_ptr, h_ptr, y_ptr, batch, n, in_channels, channels, fir_length,
          *_width(width, normalize, eps), workspace_ptr, workspace_bytes, stream)


def correlogram_device(ctx: 'Context', x_ptr: int, y_ptr: int, out_ptr: int, batch: int, n: int, stream_stride: int,
                       frame_stride: int, *, window: int, hop: int, num_lags: int, eps: float, stream: int = 0):
    """``vnd_correlogram_f32_dev``: the windowed, normalised cross-correlogram of float32 device signals (sample t of stream
    b at ``b * stream_stride + t * frame_stride``) into float32 ``(batch, windows, num_lags)``, enqueued on ``stream``."""
    _call(ctx._lib, 'vnd_correlogram_f32_dev', ctx.handle, x_ptr, y_ptr, out_ptr, batch, n, stream_stride, frame_stride, window,
          hop, num_lags, float(eps), stream)


def correlogram_stream_state_bytes(batch: int, window: int, max_frames_per_call: int) -> int:
    """``vnd_correlogram_stream_state_bytes``: the ring of a pool of ``batch`` streams."""
    return _query(load_library(), 'vnd_correlogram_stream_state_bytes', batch, window, max_frames_per_call)


def correlogram_stream_device(ctx: 'Context', state_ptr: int, state_bytes: int, max_frames_per_call: int, x_ptr: int,
                              y_ptr: int, stream_stride: int, frame_stride: int, out_ptr: int, batch: int, position: int,
                              n_in: int, *, window: int, hop: int, num_lags: int, eps: float, stream: int = 0) -> int:
    """``vnd_correlogram_stream_f32_dev``: push ``n_in`` frames per stream (frame t of stream b at ``b * stream_stride +
    t * frame_stride``) at ``position``; the rows that became final go to float32 ``(batch, rows, num_lags)`` at
    ``out_ptr``, enqueued on ``stream``.  Returns the row count."""
    return _query(ctx._lib, 'vnd_correlogram_stream_f32_dev', ctx.handle, state_ptr, state_bytes, max_frames_per_call, x_ptr,
                  y_ptr, stream_stride, frame_stride, out_ptr, batch, position, n_in, window, hop, num_lags, float(eps),
                  then=(stream,))


def correlogram_voice_stream_state_bytes(slots: int, window: int, max_frames_per_call: int) -> int:
    """``vnd_correlogram_voice_stream_state_bytes``: one int64 position per slot (padded to 16 bytes), then the ring of a
    pool of ``slots`` voices."""
    return _query(load_library(), 'vnd_correlogram_voice_stream_state_bytes', slots, window, max_frames_per_call)


def correlogram_voice_stream_reset_device(ctx: 'Context', state_ptr: int, state_bytes: int, slots: int, window: int,
                                          max_frames_per_call: int, *, stream: int = 0):
    """``vnd_correlogram_voice_stream_reset_dev``: every position of the pool to 0, enqueued on ``stream``; the ring is
    left alone."""
    _call(ctx._lib, 'vnd_correlogram_voice_stream_reset_dev', ctx.handle, state_ptr, state_bytes, slots, window,
          max_frames_per_call, stream)


def correlogram_voice_stream_device(ctx: 'Context', state_ptr: int, state_bytes: int, max_frames_per_call: int, x_ptr: int,
                                    y_ptr: int, stream_stride: int, frame_stride: int, counts_ptr: int, flags_ptr: int,
                                    out_ptr: int, out_counts_ptr: int, slots: int, *, window: int, hop: int, num_lags: int,
                                    eps: float, float64: bool = False, stream: int = 0):
    """``vnd_correlogram_voice_stream_f32_dev`` (``_f64_dev`` with ``float64``): one call of a correlogram voice pool.
    Frame t of slot b at ``b * stream_stride + t * frame_stride`` elements of ``x_ptr`` / ``y_ptr``, int32 ``(slots,)``
    counts and flags (``VOICE_START``, ``VOICE_END``), the float32 ``(slots, rows_per_call, num_lags)`` result and the
    int32 ``out_counts``, all device memory, enqueued on ``stream``."""
    _call(ctx._lib, _typed('vnd_correlogram_voice_stream_{}_dev', float64), ctx.handle, state_ptr, state_bytes,
          max_frames_per_call, x_ptr, y_ptr, stream_stride, frame_stride, counts_ptr, flags_ptr, out_ptr, out_counts_ptr, slots,
          window, hop, num_lags, float(eps), stream)


def describe_correlogram_voice_stream(slots: int, window: int, hop: int, num_lags: int, max_frames_per_call: int) -> str:
    """The fixed launch of a correlogram voice pool (``vnd_describe_correlogram_voice_stream_launch``):
    ``rows_per_call=``, ``groups=``, ``tiles=``, ``nblocks=``, ``advance_groups=`` among its fields."""
    return _describe(load_library(), 'vnd_describe_correlogram_voice_stream_launch', slots, window, hop, num_lags,
                     max_frames_per_call)


def polar_voice_stream_state_bytes(slots: int, max_frames_per_call: int, sample_bytes: int = 4) -> int:
    """``vnd_polar_voice_stream_state_bytes``: the positions, the reduce-lane sums, the partials of one call and the ring of
    a pool of ``slots`` voices; ``sample_bytes`` 4 for float32 frames, 8 for float64."""
    return _query(load_library(), 'vnd_polar_voice_stream_state_bytes', slots, max_frames_per_call, sample_bytes)


def polar_voice_stream_reset_device(ctx: 'Context', state_ptr: int, state_bytes: int, slots: int, max_frames_per_call: int,
                                    sample_bytes: int = 4, *, stream: int = 0):
    """``vnd_polar_voice_stream_reset_dev``: every position of the pool to 0, enqueued on ``stream``; sums and ring are left
    alone."""
    _call(ctx._lib, 'vnd_polar_voice_stream_reset_dev', ctx.handle, state_ptr, state_bytes, slots, max_frames_per_call,
          sample_bytes, stream)


def polar_voice_stream_device(ctx: 'Context', state_ptr: int, state_bytes: int, max_frames_per_call: int, l_ptr: int,
                              r_ptr: int, stream_stride: int, frame_stride: int, counts_ptr: int, flags_ptr: int,
                              moments_ptr: int, valid_ptr: int, slots: int, *, float64: bool = False, stream: int = 0):
    """``vnd_polar_voice_stream_f32_dev`` (``_f64_dev`` with ``float64``): one call of a polar-moments voice pool.  Frame t
    of slot b at ``b * stream_stride + t * frame_stride`` elements of ``l_ptr`` / ``r_ptr``, int32 ``(slots,)`` counts and
    flags (``VOICE_START``, ``VOICE_END``), the float64 ``(slots, 8)`` moments and the int32 ``valid``, all device memory,
    enqueued on ``stream``."""
    _call(ctx._lib, _typed('vnd_polar_voice_stream_{}_dev', float64), ctx.handle, state_ptr, state_bytes, max_frames_per_call,
          l_ptr, r_ptr, stream_stride, frame_stride, counts_ptr, flags_ptr, moments_ptr, valid_ptr, slots, stream)


def describe_polar_voice_stream(slots: int, max_frames_per_call: int, sample_bytes: int = 4) -> str:
    """The fixed launch of a polar-moments voice pool (``vnd_describe_polar_voice_stream_launch``): ``groups=``,
    ``nblocks=``, ``finish_groups=``, ``threads=`` and ``state_bytes=``."""
    return _describe(load_library(), 'vnd_describe_polar_voice_stream_launch', slots, max_frames_per_call, sample_bytes)


def scope_work_bytes(batch: int) -> int:
    """``vnd_scope_work_bytes``: the work memory of the per-signal maximum for a pool of ``batch`` signals."""
    return _query(load_library(), 'vnd_scope_work_bytes', batch)


def scope_route(bins0: int, bins1: int, used_frames: int) -> int:
    """``vnd_scope_route``: the route (``SCOPE_ROUTE_LDS`` or ``SCOPE_ROUTE_DIRECT``) a histogram of this shape takes now."""
    return _query(load_library(), 'vnd_scope_route', bins0, bins1, used_frames, out=ctypes.c_int32)


def polar_coords_device(ctx: 'Context', l_ptr: int, r_ptr: int, batch: int, n: int, stream_stride: int, frame_stride: int,
                        radii_ptr: int, thetas_ptr: int, *, ms_mode: bool = True, semicircular: bool = True,
                        normalize: bool = True, work_ptr: int = 0, work_bytes: int = 0, float64: bool = False,
                        stream: int = 0):
    """``vnd_polar_coords_f32_dev`` (``_f64_dev`` with ``float64``): the polar sample of every frame of a pool (frame t of
    signal b at ``b * stream_stride + t * frame_stride`` elements of ``l_ptr`` / ``r_ptr``) into ``(batch, n)`` radii and
    thetas of the sample type, all device memory, enqueued on ``stream``."""
    _call(ctx._lib, _typed('vnd_polar_coords_{}_dev', float64), ctx.handle, l_ptr, r_ptr, batch, n, stream_stride, frame_stride,
          bool(ms_mode), bool(semicircular), bool(normalize), radii_ptr, thetas_ptr, work_ptr, work_bytes, stream)


def polar_hist_device(ctx: 'Context', l_ptr: int, r_ptr: int, batch: int, n: int, stream_stride: int, frame_stride: int,
                      angle_edges_ptr: int, num_angle_bins: int, radius_edges_ptr: int, num_radius_bins: int,
                      counts_ptr: int, *, ms_mode: bool = True, semicircular: bool = True, radius_scale: float = 0.0,
                      n_each_ptr: int = 0, accumulate: bool = False, work_ptr: int = 0, work_bytes: int = 0,
                      float64: bool = False, stream: int = 0):
    """``vnd_polar_hist_f32_dev`` (``_f64_dev`` with ``float64``): the polar count grid of a pool, uint32 ``(batch,
    num_angle_bins, num_radius_bins)``, against float64 device edges; ``radius_scale`` 0 is the per-signal maximum."""
    _call(ctx._lib, _typed('vnd_polar_hist_{}_dev', float64), ctx.handle, l_ptr, r_ptr, batch, n, stream_stride, frame_stride,
          bool(ms_mode), bool(semicircular), float(radius_scale), angle_edges_ptr, num_angle_bins, radius_edges_ptr,
          num_radius_bins, n_each_ptr, counts_ptr, bool(accumulate), work_ptr, work_bytes, stream)


def lissajous_hist_device(ctx: 'Context', l_ptr: int, r_ptr: int, batch: int, n: int, stream_stride: int, frame_stride: int,
                          x_edges_ptr: int, x_bins: int, y_edges_ptr: int, y_bins: int, counts_ptr: int, *,
                          frame_step: int = 1, n_each_ptr: int = 0, accumulate: bool = False, float64: bool = False,
                          stream: int = 0):
    """``vnd_lissajous_hist_f32_dev`` (``_f64_dev`` with ``float64``): the L/R count grid of every ``frame_step``-th frame
    of a pool, uint32 ``(batch, x_bins, y_bins)``, L on the first axis."""
    _call(ctx._lib, _typed('vnd_lissajous_hist_{}_dev', float64), ctx.handle, l_ptr, r_ptr, batch, n, stream_stride,
          frame_stride, frame_step, x_edges_ptr, x_bins, y_edges_ptr, y_bins, n_each_ptr, counts_ptr, bool(accumulate), stream)


def scope_voice_stream_state_bytes(slots: int, max_frames_per_call: int, window_frames: int = 0) -> int:
    """``vnd_scope_voice_stream_state_bytes``: the positions and, with ``window_frames`` > 0, the ring of cells of a pool of
    ``slots`` voices."""
    return _query(load_library(), 'vnd_scope_voice_stream_state_bytes', slots, max_frames_per_call, window_frames)


def scope_voice_stream_reset_device(ctx: 'Context', state_ptr: int, state_bytes: int, slots: int, max_frames_per_call: int,
                                    window_frames: int = 0, *, stream: int = 0):
    """``vnd_scope_voice_stream_reset_dev``: every position of the pool to 0, enqueued on ``stream``; the ring and the
    grid are left alone."""
    _call(ctx._lib, 'vnd_scope_voice_stream_reset_dev', ctx.handle, state_ptr, state_bytes, slots, max_frames_per_call,
          window_frames, stream)


def scope_voice_stream_device(ctx: 'Context', state_ptr: int, state_bytes: int, max_frames_per_call: int, window_frames: int,
                              l_ptr: int, r_ptr: int, stream_stride: int, frame_stride: int, counts_ptr: int, flags_ptr: int,
                              edges0_ptr: int, bins0: int, edges1_ptr: int, bins1: int, grid_ptr: int, valid_ptr: int,
                              slots: int, *, polar: bool = True, ms_mode: bool = True, semicircular: bool = True,
                              radius_scale: float = 0.0, float64: bool = False, stream: int = 0):
    """``vnd_polar_hist_voice_stream_f32_dev`` (``polar=False``: ``vnd_lissajous_hist_voice_stream_f32_dev``; ``_f64_dev``
    with ``float64``): one call of a count-grid voice pool.  Frame t of slot b at ``b * stream_stride + t * frame_stride``
    elements of ``l_ptr`` / ``r_ptr``, int32 ``(slots,)`` counts and flags (``VOICE_START``, ``VOICE_END``), float64 device
    edges, the pool's uint32 ``(slots, bins0, bins1)`` grid and the int32 ``valid``, all device memory, enqueued on
    ``stream``."""
    name = _typed('vnd_polar_hist_voice_stream_{}_dev' if polar else 'vnd_lissajous_hist_voice_stream_{}_dev', float64)
    mode = (bool(ms_mode), bool(semicircular), float(radius_scale)) if polar else ()
    _call(ctx._lib, name, ctx.handle, state_ptr, state_bytes, max_frames_per_call, window_frames, l_ptr, r_ptr, stream_stride,
          frame_stride, counts_ptr, flags_ptr, *mode, edges0_ptr, bins0, edges1_ptr, bins1, grid_ptr, valid_ptr, slots, stream)


def polar_level_work_bytes(batch: int, n: int, num_bins: int, num_percentiles: int, float64: bool = False) -> int:
    """``vnd_polar_level_work_bytes``: the work memory of one ``vnd_polar_level_*_dev`` call of this shape."""
    return _query(load_library(), 'vnd_polar_level_work_bytes', batch, n, num_bins, num_percentiles, bool(float64))


def _percentile_args(percentiles):
    """``percentiles, num_percentiles`` of the level calls: a host array of doubles (of one entry for none) and the count."""
    return (ctypes.c_double * max(1, len(percentiles)))(*[float(p) for p in percentiles]), len(percentiles)


def polar_level_device(ctx: 'Context', l_ptr: int, r_ptr: int, batch: int, n: int, stream_stride: int, frame_stride: int,
                       angle_edges_ptr: int, num_bins: int, percentiles, levels_ptr: int, bin_counts_ptr: int, *,
                       work_ptr: int, work_bytes: int, ms_mode: bool = True, semicircular: bool = True,
                       radius_scale: float = 0.0, n_each_ptr: int = 0, float64: bool = False, stream: int = 0):
    """``vnd_polar_level_f32_dev`` (``_f64_dev`` with ``float64``): ``np.percentile`` of the radii of every angular slice
    of every signal of a pool - levels ``(batch, len(percentiles), num_bins)`` of the sample type and uint32 frames per bin
    ``(batch, num_bins)``, against float64 device edges; ``percentiles`` is a host sequence, read at the call;
    ``radius_scale`` 0 is the per-signal maximum."""
    _call(ctx._lib, _typed('vnd_polar_level_{}_dev', float64), ctx.handle, l_ptr, r_ptr, batch, n, stream_stride, frame_stride,
          bool(ms_mode), bool(semicircular), float(radius_scale), angle_edges_ptr, num_bins, *_percentile_args(percentiles),
          n_each_ptr, levels_ptr, bin_counts_ptr, work_ptr, work_bytes, stream)


def level_voice_stream_state_bytes(slots: int, max_frames_per_call: int, window_frames: int, float64: bool = False) -> int:
    """``vnd_polar_level_voice_stream_state_bytes``: the positions, the fills and the rings of keys and slices of a pool of
    ``slots`` voices over ``window_frames`` frames each."""
    return _query(load_library(), 'vnd_polar_level_voice_stream_state_bytes', slots, max_frames_per_call, window_frames,
                  bool(float64))


def level_voice_stream_reset_device(ctx: 'Context', state_ptr: int, state_bytes: int, slots: int, max_frames_per_call: int,
                                    window_frames: int, *, float64: bool = False, stream: int = 0):
    """``vnd_polar_level_voice_stream_reset_dev``: every position and fill of the pool to 0, enqueued on ``stream``; the
    rings are left alone."""
    _call(ctx._lib, 'vnd_polar_level_voice_stream_reset_dev', ctx.handle, state_ptr, state_bytes, slots, max_frames_per_call,
          window_frames, bool(float64), stream)


def level_voice_stream_push_device(ctx: 'Context', state_ptr: int, state_bytes: int, max_frames_per_call: int,
                                   window_frames: int, l_ptr: int, r_ptr: int, stream_stride: int, frame_stride: int,
                                   counts_ptr: int, flags_ptr: int, angle_edges_ptr: int, num_bins: int, valid_ptr: int,
                                   slots: int, *, radius_scale: float, ms_mode: bool = True, semicircular: bool = True,
                                   float64: bool = False, stream: int = 0):
    """``vnd_polar_level_voice_stream_push_f32_dev`` (``_f64_dev`` with ``float64``): one call's frames into the rings of
    a level voice pool.  Frame t of slot b at ``b * stream_stride + t * frame_stride`` elements of ``l_ptr`` / ``r_ptr``,
    int32 ``(slots,)`` counts and flags (``VOICE_START``, ``VOICE_END``), float64 device edges and the int32 ``valid``, all
    device memory, enqueued on ``stream``."""
    _call(ctx._lib, _typed('vnd_polar_level_voice_stream_push_{}_dev', float64), ctx.handle, state_ptr, state_bytes,
          max_frames_per_call, window_frames, l_ptr, r_ptr, stream_stride, frame_stride, counts_ptr, flags_ptr, bool(ms_mode),
          bool(semicircular), float(radius_scale), angle_edges_ptr, num_bins, valid_ptr, slots, stream)


def level_voice_stream_work_bytes(slots: int, window_frames: int, num_bins: int, num_percentiles: int,
                                  float64: bool = False) -> int:
    """``vnd_polar_level_voice_stream_work_bytes``: the work memory of one levels call of a level voice pool."""
    return _query(load_library(), 'vnd_polar_level_voice_stream_work_bytes', slots, window_frames, num_bins, num_percentiles,
                  bool(float64))


def level_voice_stream_levels_device(ctx: 'Context', state_ptr: int, state_bytes: int, max_frames_per_call: int,
                                     window_frames: int, num_bins: int, percentiles, levels_ptr: int, bin_counts_ptr: int,
                                     slots: int, *, work_ptr: int, work_bytes: int, float64: bool = False, stream: int = 0):
    """``vnd_polar_level_voice_stream_levels_f32_dev`` (``_f64_dev`` with ``float64``): the envelope of every slot from the
    pool's state alone - levels ``(slots, len(percentiles), num_bins)`` of the sample type and uint32 frames per slice
    ``(slots, num_bins)``; ``percentiles`` is a host sequence, read at the call."""
    _call(ctx._lib, _typed('vnd_polar_level_voice_stream_levels_{}_dev', float64), ctx.handle, state_ptr, state_bytes,
          max_frames_per_call, window_frames, num_bins, *_percentile_args(percentiles), levels_ptr, bin_counts_ptr, work_ptr,
          work_bytes, slots, stream)


def spectrum_run_length(nfft: int, nperseg: int, hop: int, float64: bool = False, cross_channels: int = 0) -> int:
    """``vnd_spectrum_run_length``: the consecutive segments of one signal a workgroup owns - ``cross_channels`` 0 for the
    spectrogram, 1 or 2 for the cross spectra."""
    return _query(load_library(), 'vnd_spectrum_run_length', nfft, nperseg, hop, bool(float64), cross_channels,
                  out=ctypes.c_int32)


def cross_spectra_work_bytes(batch: int, n: int, channels: int, nperseg: int, hop: int, nfft: int,
                             float64: bool = False) -> int:
    """``vnd_cross_spectra_work_bytes``: the work memory of one ``vnd_cross_spectra_*_dev`` call of this shape."""
    return _query(load_library(), 'vnd_cross_spectra_work_bytes', batch, n, channels, nperseg, hop, nfft, bool(float64))


def _spectrum_args(ctx, frames_ptr, batch, n, stream_stride, frame_stride, channels, window_ptr, twiddles_ptr, nperseg, hop,
                   nfft, detrend, scale, n_each_ptr):
    return (ctx.handle, frames_ptr, batch, n, stream_stride, frame_stride, channels, window_ptr, twiddles_ptr, nperseg, hop,
            nfft, bool(detrend), float(scale), n_each_ptr)


def spectrogram_device(ctx: 'Context', frames_ptr: int, batch: int, n: int, stream_stride: int, frame_stride: int,
                       channels: int, window_ptr: int, twiddles_ptr: int, nperseg: int, hop: int, nfft: int, sxx_ptr: int, *,
                       detrend: bool = True, scale: float = 1.0, n_each_ptr: int = 0, float64: bool = False, stream: int = 0):
    """``vnd_spectrogram_f32_dev`` (``_f64_dev`` with ``float64``): the power columns of every signal and channel of a pool,
    ``(batch, channels, nfft // 2 + 1, (n - nperseg) // hop + 1)`` of the sample type, all device memory, enqueued on
    ``stream``."""
    _call(ctx._lib, _typed('vnd_spectrogram_{}_dev', float64),
          *_spectrum_args(ctx, frames_ptr, batch, n, stream_stride, frame_stride, channels, window_ptr, twiddles_ptr, nperseg,
                          hop, nfft, detrend, scale, n_each_ptr), sxx_ptr, stream)


def cross_spectra_device(ctx: 'Context', frames_ptr: int, batch: int, n: int, stream_stride: int, frame_stride: int,
                         channels: int, window_ptr: int, twiddles_ptr: int, nperseg: int, hop: int, nfft: int, pxx_ptr: int,
                         pyy_ptr: int, pxy_ptr: int, *, work_ptr: int, work_bytes: int, detrend: bool = True,
                         scale: float = 1.0, n_each_ptr: int = 0, float64: bool = False, stream: int = 0):
    """``vnd_cross_spectra_f32_dev`` (``_f64_dev`` with ``float64``): Welch's ``Pxx``, ``Pyy`` ``(batch, F)`` and ``Pxy``
    ``(batch, F, 2)`` of a pool (one channel: ``Pxx`` alone), float64 sums in ascending segment order."""
    _call(ctx._lib, _typed('vnd_cross_spectra_{}_dev', float64),
          *_spectrum_args(ctx, frames_ptr, batch, n, stream_stride, frame_stride, channels, window_ptr, twiddles_ptr, nperseg,
                          hop, nfft, detrend, scale, n_each_ptr), pxx_ptr, pyy_ptr, pxy_ptr, work_ptr, work_bytes, stream)


def spectrum_voice_stream_state_bytes(slots: int, channels: int, nperseg: int, hop: int, nfft: int, max_frames_per_call: int,
                                      float64: bool = False) -> int:
    """``vnd_spectrum_voice_stream_state_bytes``: the positions, the Welch sums, the work of one call and the ring of a pool
    of ``slots`` voices."""
    return _query(load_library(), 'vnd_spectrum_voice_stream_state_bytes', slots, channels, nperseg, hop, nfft,
                  max_frames_per_call, bool(float64))


def spectrum_voice_stream_reset_device(ctx: 'Context', state_ptr: int, state_bytes: int, slots: int, channels: int,
                                       nperseg: int, hop: int, nfft: int, max_frames_per_call: int, float64: bool = False, *,
                                       stream: int = 0):
    """``vnd_spectrum_voice_stream_reset_dev``: every position of the pool to 0, enqueued on ``stream``; sums and ring are
    left alone."""
    _call(ctx._lib, 'vnd_spectrum_voice_stream_reset_dev', ctx.handle, state_ptr, state_bytes, slots, channels, nperseg, hop,
          nfft, max_frames_per_call, bool(float64), stream)


def spectrum_voice_stream_device(ctx: 'Context', state_ptr: int, state_bytes: int, max_frames_per_call: int, frames_ptr: int,
                                 stream_stride: int, frame_stride: int, channels: int, counts_ptr: int, flags_ptr: int,
                                 window_ptr: int, twiddles_ptr: int, nperseg: int, hop: int, nfft: int, cols_ptr: int,
                                 out_counts_ptr: int, pxx_ptr: int, pyy_ptr: int, pxy_ptr: int, segments_ptr: int, slots: int,
                                 *, detrend: bool = True, scale: float = 1.0, float64: bool = False, stream: int = 0):
    """``vnd_spectrum_voice_stream_f32_dev`` (``_f64_dev`` with ``float64``): one call of a spectrum voice pool.  Sample t of
    channel c of slot b at ``b * stream_stride + t * frame_stride + c`` elements of ``frames_ptr``, int32 ``(slots,)`` counts
    and flags (``VOICE_START``, ``VOICE_END``), the ``(slots, rows_per_call, channels, F)`` columns (0: none), the int32
    ``out_counts``, the means ``pxx``, ``pyy`` ``(slots, F)``, ``pxy`` ``(slots, F, 2)`` and the int64 ``segments`` (0 as a
    group: none), all device memory, enqueued on ``stream``."""
    _call(ctx._lib, _typed('vnd_spectrum_voice_stream_{}_dev', float64), ctx.handle, state_ptr, state_bytes,
          max_frames_per_call, frames_ptr, stream_stride, frame_stride, channels, counts_ptr, flags_ptr, window_ptr,
          twiddles_ptr, nperseg, hop, nfft, bool(detrend), float(scale), cols_ptr, out_counts_ptr, pxx_ptr, pyy_ptr, pxy_ptr,
          segments_ptr, slots, stream)


def describe_spectrum_voice_stream(slots: int, channels: int, nperseg: int, hop: int, nfft: int, max_frames_per_call: int,
                                   float64: bool = False) -> str:
    """The fixed launch of a spectrum voice pool (``vnd_describe_spectrum_voice_stream_launch``): ``rows_per_call=``,
    ``run=``, ``groups=``, ``nblocks=``, ``threads=``, ``advance_groups=`` and ``state_bytes=``."""
    return _describe(load_library(), 'vnd_describe_spectrum_voice_stream_launch', slots, channels, nperseg, hop, nfft,
                     max_frames_per_call, bool(float64))


def haas_scan_workspace_bytes(n: int, n_delays: int, max_delay: int) -> int:
    return _query(load_library(), 'vnd_haas_scan_workspace_bytes', n, n_delays, max_delay)


def haas_scan_host(ctx: 'Context', x: np.ndarray, delays, *, delayed_channel: int, ms_mode: bool, width) -> np.ndarray:
    """``vnd_haas_scan_f64_host``: float64 ``(F, 8)`` polar moments of ``HaasEffect(delay d).decorrelate(x)`` for
    each integer delay d, from a C-contiguous float32 ``(n, 1|2)`` signal in host memory."""
    if x.dtype != np.float32 or not x.flags.c_contiguous or x.ndim != 2:
        raise ValueError('haas_scan_host wants a C-contiguous float32 (n, C) array')
    d = np.ascontiguousarray(delays, np.int64)
    if d.ndim != 1 or (d.size and (d.min() < np.iinfo(np.int32).min or d.max() > np.iinfo(np.int32).max)):
        raise ValueError('haas_scan_host wants a 1-D list of int32 delays')
    d = d.astype(np.int32)
    out = np.zeros((d.size, MOMENTS), np.float64)
    _call(ctx._lib, 'vnd_haas_scan_f64_host', ctx.handle, _ptr(x, _f32), x.shape[0], x.shape[1], _ptr(d, _i32), d.size,
          int(delayed_channel), bool(ms_mode), *_width(width), _ptr(out, _f64))
    return out


def haas_scan_device(ctx: 'Context', x_ptr: int, n: int, channels: int, delays_ptr: int, n_delays: int,
                     moments_ptr: int, *, delayed_channel: int, ms_mode: bool, width, workspace_ptr: int,
                     workspace_bytes: int, stream: int = 0):
    """``vnd_haas_scan_f64_dev``: float64 ``(n_delays, 8)`` moments from float32 ``(n, channels)`` and int32 delays,
    all device buffers, enqueued on ``stream``."""
    _call(ctx._lib, 'vnd_haas_scan_f64_dev', ctx.handle, x_ptr, n, channels, delays_ptr, n_delays, int(delayed_channel),
          bool(ms_mode), *_width(width), moments_ptr, workspace_ptr, workspace_bytes, stream)


def haas_pairs_workspace_bytes(n: int, n_pairs: int, max_delay: int) -> int:
    return _query(load_library(), 'vnd_haas_pairs_workspace_bytes', n, n_pairs, max_delay)


def _pair_indices(signals, others, what: str, wants: str = 'signal and candidate indices', unit: str = 'candidates'):
    """The two int32 index lists of a pairs call, one entry per pair, refused in the caller's words."""
    s = np.ascontiguousarray(signals, np.int64)
    c = np.ascontiguousarray(others, np.int64)
    i32 = np.iinfo(np.int32)
    for v in (s, c):
        if v.ndim != 1 or (v.size and (v.min() < i32.min or v.max() > i32.max)):
            raise ValueError(f'{what} wants 1-D lists of int32 {wants}')
    if s.size != c.size:
        raise ValueError(f'{s.size} signal indices for {c.size} {unit}')
    return s.astype(np.int32), c.astype(np.int32)


def haas_pairs_host(ctx: 'Context', x: np.ndarray, signals, delays, *, delayed_channel: int, ms_mode: bool,
                    width) -> np.ndarray:
    """``vnd_haas_pairs_f64_host``: float64 ``(P, 8)`` polar moments of ``HaasEffect(delay d_p).decorrelate(x[s_p])``
    for each pair ``(s_p, d_p)``, from a C-contiguous float32 ``(batch, n, 1|2)`` pool in host memory."""
    if x.dtype != np.float32 or not x.flags.c_contiguous or x.ndim != 3:
        raise ValueError('haas_pairs_host wants a C-contiguous float32 (batch, n, C) array')
    s, d = _pair_indices(signals, delays, 'haas_pairs_host', 'signal indices and delays', 'delays')
    out = np.zeros((d.size, MOMENTS), np.float64)
    _call(ctx._lib, 'vnd_haas_pairs_f64_host', ctx.handle, _ptr(x, _f32), x.shape[0], x.shape[1], x.shape[2], _ptr(s, _i32),
          _ptr(d, _i32), d.size, int(delayed_channel), bool(ms_mode), *_width(width), _ptr(out, _f64))
    return out


def haas_pairs_device(ctx: 'Context', x_ptr: int, batch: int, n: int, channels: int, signals_ptr: int,
                      delays_ptr: int, n_pairs: int, moments_ptr: int, *, delayed_channel: int, ms_mode: bool, width,
                      workspace_ptr: int, workspace_bytes: int, stream: int = 0):
    """``vnd_haas_pairs_f64_dev``: float64 ``(n_pairs, 8)`` moments from a float32 ``(batch, n, channels)`` pool and
    int32 signal indices and delays, all device buffers, enqueued on ``stream``."""
    _call(ctx._lib, 'vnd_haas_pairs_f64_dev', ctx.handle, x_ptr, batch, n, channels, signals_ptr, delays_ptr, n_pairs,
          int(delayed_channel), bool(ms_mode), *_width(width), moments_ptr, workspace_ptr, workspace_bytes, stream)


def velvet_pairs_workspace_bytes(n: int, n_pairs: int) -> int:
    return _query(load_library(), 'vnd_velvet_pairs_workspace_bytes', n, n_pairs)


def velvet_pairs_host(ctx: 'Context', bank: 'TapTable', x: np.ndarray, signals, candidates, *,
                      mode: int = MODE_EXACT) -> np.ndarray:
    """``vnd_velvet_pairs_f32_host``: float64 ``(P, 8)`` polar moments of candidate ``c_p`` of ``bank`` (channels
    ``2c``, ``2c + 1``) convolved with ``x[s_p]`` for each pair ``(s_p, c_p)``, from a C-contiguous float32
    ``(batch, n, 1|2)`` pool in host memory."""
    if x.dtype != np.float32 or not x.flags.c_contiguous or x.ndim != 3:
        raise ValueError('velvet_pairs_host wants a C-contiguous float32 (batch, n, C) array')
    s, c = _pair_indices(signals, candidates, 'velvet_pairs_host')
    out = np.zeros((c.size, MOMENTS), np.float64)
    _call(ctx._lib, 'vnd_velvet_pairs_f32_host', ctx.handle, bank.handle, _ptr(x, _f32), x.shape[0], x.shape[1], x.shape[2],
          _ptr(s, _i32), _ptr(c, _i32), c.size, int(mode), _ptr(out, _f64))
    return out


def velvet_pairs_device(ctx: 'Context', bank: 'TapTable', x_ptr: int, batch: int, n: int, channels: int,
                        signals_ptr: int, candidates_ptr: int, n_pairs: int, moments_ptr: int, *,
                        workspace_ptr: int, workspace_bytes: int, mode: int = MODE_EXACT, stream: int = 0):
    """``vnd_velvet_pairs_f32_dev``: float64 ``(n_pairs, 8)`` moments from a float32 ``(batch, n, channels)`` pool and
    int32 signal and candidate indices, all device buffers, enqueued on ``stream``."""
    _call(ctx._lib, 'vnd_velvet_pairs_f32_dev', ctx.handle, bank.handle, x_ptr, batch, n, channels, signals_ptr, candidates_ptr,
          n_pairs, int(mode), moments_ptr, workspace_ptr, workspace_bytes, stream)


def _each_host_args(x: np.ndarray, per_signal, what: str, name: str):
    if x.dtype != np.float32 or not x.flags.c_contiguous or x.ndim != 3:
        raise ValueError(f'{what} wants a C-contiguous float32 (batch, n, C) array')
    v = np.ascontiguousarray(per_signal, np.int64)
    i32 = np.iinfo(np.int32)
    if v.ndim != 1 or v.size != x.shape[0] or (v.size and (v.min() < i32.min or v.max() > i32.max)):
        raise ValueError(f'{what} wants one int32 {name} per signal: {x.shape[0]} signals, {name} of shape {v.shape}')
    return v.astype(np.int32)


def convolve_each_host(ctx: 'Context', bank: 'TapTable', x: np.ndarray, tables, *, mode: int = MODE_EXACT) -> np.ndarray:
    """``vnd_convolve_each_f32_host``: float32 ``(batch, n, 2)``, row b the convolution of ``x[b]`` with candidate
    ``tables[b]`` of ``bank`` (channels ``2t``, ``2t + 1``), from a C-contiguous float32 ``(batch, n, 1|2)`` pool in
    host memory."""
    t = _each_host_args(x, tables, 'convolve_each_host', 'table index')
    y = np.empty(x.shape[:2] + (2,), np.float32)
    _call(ctx._lib, 'vnd_convolve_each_f32_host', ctx.handle, bank.handle, _ptr(x, _f32), _ptr(t, _i32), _ptr(y, _f32),
          x.shape[0], x.shape[1], x.shape[2], int(mode))
    return y


def convolve_each_device(ctx: 'Context', bank: 'TapTable', x_ptr: int, tables_ptr: int, y_ptr: int, batch: int, n: int,
                         channels: int, *, mode: int = MODE_EXACT, stream: int = 0):
    """``vnd_convolve_each_f32_dev``: float32 ``(batch, n, channels)`` pool, int32 ``(batch,)`` table indices and the
    float32 ``(batch, n, 2)`` result, all device buffers, enqueued on ``stream``."""
    _call(ctx._lib, 'vnd_convolve_each_f32_dev', ctx.handle, bank.handle, x_ptr, tables_ptr, y_ptr, batch, n, channels,
          int(mode), stream)


def decorrelate_each_host(ctx: 'Context', bank: 'TapTable', x: np.ndarray, tables, *, ms_encode: bool, width, normalize,
                          eps: float = 1e-10, mode: int = MODE_EXACT) -> np.ndarray:
    """``vnd_decorrelate_each_f32_host``: :func:`convolve_each_host` and the decorrelate stage behind it (``normalize``:
    False/True or one of the ``NORMALIZE_*`` values); the stage settings are the call's, not per signal."""
    t = _each_host_args(x, tables, 'decorrelate_each_host', 'table index')
    y = np.empty(x.shape[:2] + (2,), np.float32)
    _call(ctx._lib, 'vnd_decorrelate_each_f32_host', ctx.handle, bank.handle, _ptr(x, _f32), _ptr(t, _i32), _ptr(y, _f32),
          x.shape[0], x.shape[1], x.shape[2], int(mode), bool(ms_encode), *_width(width, normalize, eps))
    return y


def decorrelate_each_device(ctx: 'Context', bank: 'TapTable', x_ptr: int, tables_ptr: int, y_ptr: int, batch: int, n: int,
                            channels: int, *, ms_encode: bool, width, normalize, workspace_ptr: int, workspace_bytes: int,
                            eps: float = 1e-10, mode: int = MODE_EXACT, stream: int = 0):
    """``vnd_decorrelate_each_f32_dev``; the workspace is ``decorrelate_workspace_bytes(batch, n, 2)``'s."""
    _call(ctx._lib, 'vnd_decorrelate_each_f32_dev', ctx.handle, bank.handle, x_ptr, tables_ptr, y_ptr, batch, n, channels,
          int(mode), bool(ms_encode), *_width(width, normalize, eps), workspace_ptr, workspace_bytes, stream)


def haas_each_host(ctx: 'Context', x: np.ndarray, delays, *, max_delay: int, delayed_channel: int, ms_mode: bool,
                   width) -> np.ndarray:
    """``vnd_haas_each_f64_host``: float64 ``(batch, n + max_delay, 2)``; rows ``[0, n + delays[b])`` of signal b are
    ``HaasEffect`` with that delay, the rest zeros.  x: a C-contiguous float32 ``(batch, n, 1|2)`` pool."""
    d = _each_host_args(x, delays, 'haas_each_host', 'delay')
    y = np.empty((x.shape[0], x.shape[1] + int(max_delay), 2), np.float64)
    _call(ctx._lib, 'vnd_haas_each_f64_host', ctx.handle, _ptr(x, _f32), _ptr(y, _f64), x.shape[0], x.shape[1], x.shape[2],
          _ptr(d, _i32), int(max_delay), int(delayed_channel), bool(ms_mode), *_width(width))
    return y


def haas_each_device(ctx: 'Context', x_ptr: int, y_ptr: int, batch: int, n: int, channels: int, delays_ptr: int, *,
                     max_delay: int, delayed_channel: int, ms_mode: bool, width, stream: int = 0):
    """``vnd_haas_each_f64_dev``: float32 ``(batch, n, channels)`` pool, int32 ``(batch,)`` delays and the float64
    ``(batch, n + max_delay, 2)`` result, all device buffers, enqueued on ``stream``."""
    _call(ctx._lib, 'vnd_haas_each_f64_dev', ctx.handle, x_ptr, y_ptr, batch, n, channels, delays_ptr, int(max_delay),
          int(delayed_channel), bool(ms_mode), *_width(width), stream)


def each_stream_state_bytes(bank: 'TapTable', batch: int, channels: int, max_frames_per_call: int) -> int:
    """``vnd_each_stream_state_bytes``: the ring of a pool of ``batch`` streams at the bank's latency."""
    return _query(load_library(), 'vnd_each_stream_state_bytes', bank.handle, batch, channels, max_frames_per_call)


def _each_stream_call(name: str, ctx, bank, tables_ptr, state_ptr, state_bytes, max_frames_per_call, x_ptr, y_ptr, batch,
                      position, n_in, channels, final, ms_encode, width, mode, *stream) -> int:
    return _query(ctx._lib, name, ctx.handle, bank.handle, tables_ptr, state_ptr, state_bytes, max_frames_per_call, x_ptr,
                  y_ptr, batch, position, n_in, channels, bool(final), int(mode), bool(ms_encode), *_width(width), then=stream)


def each_stream_device(ctx: 'Context', bank: 'TapTable', tables_ptr: int, state_ptr: int, state_bytes: int,
                       max_frames_per_call: int, x_ptr: int, y_ptr: int, batch: int, position: int, n_in: int, channels: int,
                       *, final: bool, ms_encode: bool, width, mode: int = MODE_EXACT, stream: int = 0) -> int:
    """``vnd_each_stream_f32_dev``: the next float32 ``(batch, n_in, channels)`` block of a pool, stream b through
    candidate ``tables[b]`` of ``bank``; int32 ``(batch,)`` table indices, the state, the block and the float32
    ``(batch, n_out, 2)`` result are device buffers; enqueued on ``stream``.  Returns ``n_out``."""
    return _each_stream_call('vnd_each_stream_f32_dev', ctx, bank, tables_ptr, state_ptr, state_bytes, max_frames_per_call,
                             x_ptr, y_ptr, batch, position, n_in, channels, final, ms_encode, width, mode, stream)


def each_stream_host(ctx: 'Context', bank: 'TapTable', tables, state_ptr: int, state_bytes: int, max_frames_per_call: int,
                     x: np.ndarray, n_out: int, position: int, *, final: bool, ms_encode: bool, width,
                     mode: int = MODE_EXACT) -> np.ndarray:
    """``vnd_each_stream_f32_host``: the same from a C-contiguous float32 ``(batch, n_in, 1|2)`` block and table indices
    in host memory (the state stays on the device), synchronous; float32 ``(batch, n_out, 2)``."""
    t = _each_host_args(x, tables, 'each_stream_host', 'table index')
    y = np.empty((x.shape[0], int(n_out), 2), np.float32)
    got = _each_stream_call('vnd_each_stream_f32_host', ctx, bank, t.ctypes.data, state_ptr, state_bytes, max_frames_per_call,
                            x.ctypes.data, y.ctypes.data, x.shape[0], position, x.shape[1], x.shape[2], final, ms_encode,
                            width, mode)
    if got != n_out:
        raise NativeError(f'vnd_each_stream_f32_host returned {got} frames, the span is {n_out}')
    return y


def voice_stream_state_bytes(bank: 'TapTable', slots: int, channels: int, max_frames_per_call: int) -> int:
    """``vnd_voice_stream_state_bytes``: one int64 position per slot (padded to 16 bytes), then the ring of a pool of
    ``slots`` voices at the bank's latency."""
    return _query(load_library(), 'vnd_voice_stream_state_bytes', bank.handle, slots, channels, max_frames_per_call)


def voice_stream_reset_device(ctx: 'Context', bank: 'TapTable', state_ptr: int, state_bytes: int, slots: int, channels: int,
                              max_frames_per_call: int, *, stream: int = 0):
    """``vnd_voice_stream_reset_dev``: every position of the pool to 0, enqueued on ``stream``; the ring is left alone."""
    _call(ctx._lib, 'vnd_voice_stream_reset_dev', ctx.handle, state_ptr, state_bytes, slots, channels, bank.handle,
          max_frames_per_call, stream)


def _per_slot_host_args(what: str, slots: int, *per_slot):
    """The int32 arrays of a voice pool's host call from ``(name, values)`` pairs, one value per slot each."""
    out = []
    for name, v in per_slot:
        v = np.ascontiguousarray(v, np.int64)
        i32 = np.iinfo(np.int32)
        if v.ndim != 1 or v.size != slots or (v.size and (v.min() < i32.min or v.max() > i32.max)):
            raise ValueError(f'{what} wants one int32 {name} per slot: {slots} slots, shape {v.shape}')
        out.append(v.astype(np.int32))
    return out


def _voice_stream_call(name: str, ctx, bank, state_ptr, state_bytes, max_frames_per_call, x_ptr, counts_ptr, flags_ptr,
                       tables_ptr, y_ptr, out_counts_ptr, slots, channels, ms_encode, width, mode, *stream):
    _call(ctx._lib, name, ctx.handle, bank.handle, state_ptr, state_bytes, max_frames_per_call, x_ptr, counts_ptr, flags_ptr,
          tables_ptr, y_ptr, out_counts_ptr, slots, channels, int(mode), bool(ms_encode), *_width(width), *stream)


def voice_stream_device(ctx: 'Context', bank: 'TapTable', state_ptr: int, state_bytes: int, max_frames_per_call: int,
                        x_ptr: int, counts_ptr: int, flags_ptr: int, tables_ptr: int, y_ptr: int, out_counts_ptr: int,
                        slots: int, channels: int, *, ms_encode: bool, width, mode: int = MODE_EXACT, stream: int = 0):
    """``vnd_voice_stream_f32_dev``: one call of a voice pool.  float32 ``(slots, M, channels)`` blocks, int32 ``(slots,)``
    counts, flags (``VOICE_START``, ``VOICE_END``) and table indices, the float32 ``(slots, M + H, 2)`` result and the
    int32 ``(slots,)`` output counts are device buffers of fixed shape; two kernels enqueued on ``stream``, nothing else."""
    _voice_stream_call('vnd_voice_stream_f32_dev', ctx, bank, state_ptr, state_bytes, max_frames_per_call, x_ptr, counts_ptr,
                       flags_ptr, tables_ptr, y_ptr, out_counts_ptr, slots, channels, ms_encode, width, mode, stream)


def voice_stream_host(ctx: 'Context', bank: 'TapTable', state_ptr: int, state_bytes: int, max_frames_per_call: int,
                      x: np.ndarray, counts, flags, tables, y: np.ndarray, *, ms_encode: bool, width,
                      mode: int = MODE_EXACT) -> np.ndarray:
    """``vnd_voice_stream_f32_host``: the same from host arrays (the state stays on the device), synchronous.  ``x`` is a
    C-contiguous float32 ``(slots, M, 1|2)`` block, ``y`` a C-contiguous float32 ``(slots, M + H, 2)`` array written in
    place: the first ``out_counts[b]`` frames of row b.  Returns the int32 ``out_counts``."""
    if x.dtype != np.float32 or not x.flags.c_contiguous or x.ndim != 3 or x.shape[1] != max_frames_per_call:
        raise ValueError('voice_stream_host wants a C-contiguous float32 (slots, max_frames_per_call, C) block')
    slots = x.shape[0]
    if y.dtype != np.float32 or not y.flags.c_contiguous or y.ndim != 3 or y.shape[0] != slots or y.shape[2] != 2:
        raise ValueError('voice_stream_host wants a C-contiguous float32 (slots, max_frames_per_call + H, 2) result')
    c, f, t = _per_slot_host_args('voice_stream_host', slots, ('count', counts), ('flags value', flags),
                                  ('table index', tables))
    out_counts = np.zeros(slots, np.int32)
    _voice_stream_call('vnd_voice_stream_f32_host', ctx, bank, state_ptr, state_bytes, max_frames_per_call, x.ctypes.data,
                       c.ctypes.data, f.ctypes.data, t.ctypes.data, y.ctypes.data, out_counts.ctypes.data, slots, x.shape[2],
                       ms_encode, width, mode)
    return out_counts


def haas_voice_stream_state_bytes(slots: int, channels: int, max_delay: int, max_frames_per_call: int) -> int:
    """``vnd_haas_voice_stream_state_bytes``: one int64 position per slot (padded to 16 bytes), then the ring of a pool of
    ``slots`` voices delayed by up to ``max_delay`` frames (none for ``max_delay`` 0)."""
    return _query(load_library(), 'vnd_haas_voice_stream_state_bytes', slots, channels, int(max_delay), max_frames_per_call)


def haas_voice_stream_reset_device(ctx: 'Context', state_ptr: int, state_bytes: int, slots: int, channels: int,
                                   max_delay: int, max_frames_per_call: int, *, stream: int = 0):
    """``vnd_haas_voice_stream_reset_dev``: every position of the pool to 0, enqueued on ``stream``; the ring is left alone."""
    _call(ctx._lib, 'vnd_haas_voice_stream_reset_dev', ctx.handle, state_ptr, state_bytes, slots, channels, int(max_delay),
          max_frames_per_call, stream)


def _haas_voice_stream_call(name: str, ctx, state_ptr, state_bytes, max_frames_per_call, x_ptr, counts_ptr, flags_ptr,
                            delays_ptr, y_ptr, out_counts_ptr, slots, channels, max_delay, delayed_channel, ms_mode, width,
                            *stream):
    _call(ctx._lib, name, ctx.handle, state_ptr, state_bytes, max_frames_per_call, x_ptr, counts_ptr, flags_ptr, delays_ptr,
          y_ptr, out_counts_ptr, slots, channels, int(max_delay), int(delayed_channel), bool(ms_mode), *_width(width), *stream)


def haas_voice_stream_device(ctx: 'Context', state_ptr: int, state_bytes: int, max_frames_per_call: int, x_ptr: int,
                             counts_ptr: int, flags_ptr: int, delays_ptr: int, y_ptr: int, out_counts_ptr: int, slots: int,
                             channels: int, *, max_delay: int, delayed_channel: int, ms_mode: bool, width, stream: int = 0):
    """``vnd_haas_voice_stream_f64_dev``: one call of a Haas voice pool.  float32 ``(slots, M, channels)`` blocks, int32
    ``(slots,)`` counts, flags (``VOICE_START``, ``VOICE_END``) and delays, the float64 ``(slots, M + max_delay, 2)``
    result and the int32 ``(slots,)`` output counts are device buffers of fixed shape; two kernels enqueued on ``stream``,
    nothing else."""
    _haas_voice_stream_call('vnd_haas_voice_stream_f64_dev', ctx, state_ptr, state_bytes, max_frames_per_call, x_ptr,
                            counts_ptr, flags_ptr, delays_ptr, y_ptr, out_counts_ptr, slots, channels, max_delay,
                            delayed_channel, ms_mode, width, stream)


def haas_voice_stream_host(ctx: 'Context', state_ptr: int, state_bytes: int, max_frames_per_call: int, x: np.ndarray,
                           counts, flags, delays, y: np.ndarray, *, max_delay: int, delayed_channel: int, ms_mode: bool,
                           width) -> np.ndarray:
    """``vnd_haas_voice_stream_f64_host``: the same from host arrays (the state stays on the device), synchronous.  ``x``
    is a C-contiguous float32 ``(slots, M, 1|2)`` block, ``y`` a C-contiguous float64 ``(slots, M + max_delay, 2)`` array
    written in place: the first ``out_counts[b]`` frames of row b.  Returns the int32 ``out_counts``."""
    if x.dtype != np.float32 or not x.flags.c_contiguous or x.ndim != 3 or x.shape[1] != max_frames_per_call:
        raise ValueError('haas_voice_stream_host wants a C-contiguous float32 (slots, max_frames_per_call, C) block')
    slots = x.shape[0]
    if y.dtype != np.float64 or not y.flags.c_contiguous or y.shape != (slots, max_frames_per_call + int(max_delay), 2):
        raise ValueError('haas_voice_stream_host wants a C-contiguous float64 (slots, max_frames_per_call + max_delay, 2) '
                         'result')
    c, f, d = _per_slot_host_args('haas_voice_stream_host', slots, ('count', counts), ('flags value', flags),
                                  ('delay', delays))
    out_counts = np.zeros(slots, np.int32)
    _haas_voice_stream_call('vnd_haas_voice_stream_f64_host', ctx, state_ptr, state_bytes, max_frames_per_call, x.ctypes.data,
                            c.ctypes.data, f.ctypes.data, d.ctypes.data, y.ctypes.data, out_counts.ctypes.data, slots,
                            x.shape[2], max_delay, delayed_channel, ms_mode, width)
    return out_counts


def haas_each_stream_state_bytes(batch: int, channels: int, max_delay: int, max_frames_per_call: int) -> int:
    """``vnd_haas_each_stream_state_bytes``: the ring of a pool of ``batch`` streams delayed by up to ``max_delay``."""
    return _query(load_library(), 'vnd_haas_each_stream_state_bytes', batch, channels, int(max_delay), max_frames_per_call)


def _haas_each_stream_call(name: str, ctx, state_ptr, state_bytes, max_frames_per_call, x_ptr, y_ptr, batch, position, n_in,
                           channels, final, delays_ptr, max_delay, delayed_channel, ms_mode, width, *stream) -> int:
    return _query(ctx._lib, name, ctx.handle, state_ptr, state_bytes, max_frames_per_call, x_ptr, y_ptr, batch, position, n_in,
                  channels, bool(final), delays_ptr, int(max_delay), int(delayed_channel), bool(ms_mode), *_width(width),
                  then=stream)


def haas_each_stream_device(ctx: 'Context', state_ptr: int, state_bytes: int, max_frames_per_call: int, x_ptr: int, y_ptr: int,
                            batch: int, position: int, n_in: int, channels: int, delays_ptr: int, *, final: bool,
                            max_delay: int, delayed_channel: int, ms_mode: bool, width, stream: int = 0) -> int:
    """``vnd_haas_each_stream_f64_dev``: the next float32 ``(batch, n_in, channels)`` block of a pool, stream b delayed by
    ``delays[b]`` frames; int32 ``(batch,)`` delays, the state, the block and the float64 ``(batch, n_out, 2)`` result are
    device buffers; enqueued on ``stream``.  Returns ``n_out = n_in + (max_delay if final else 0)``."""
    return _haas_each_stream_call('vnd_haas_each_stream_f64_dev', ctx, state_ptr, state_bytes, max_frames_per_call, x_ptr,
                                  y_ptr, batch, position, n_in, channels, final, delays_ptr, max_delay, delayed_channel,
                                  ms_mode, width, stream)


def haas_each_stream_host(ctx: 'Context', state_ptr: int, state_bytes: int, max_frames_per_call: int, x: np.ndarray, delays,
                          position: int, *, final: bool, max_delay: int, delayed_channel: int, ms_mode: bool,
                          width) -> np.ndarray:
    """``vnd_haas_each_stream_f64_host``: the same from a C-contiguous float32 ``(batch, n_in, 1|2)`` block and delays in
    host memory (the state stays on the device), synchronous; float64 ``(batch, n_out, 2)``."""
    d = _each_host_args(x, delays, 'haas_each_stream_host', 'delay')
    n_out = x.shape[1] + (int(max_delay) if final else 0)
    y = np.empty((x.shape[0], n_out, 2), np.float64)
    got = _haas_each_stream_call('vnd_haas_each_stream_f64_host', ctx, state_ptr, state_bytes, max_frames_per_call,
                                 x.ctypes.data, y.ctypes.data, x.shape[0], position, x.shape[1], x.shape[2], final,
                                 d.ctypes.data, max_delay, delayed_channel, ms_mode, width)
    if got != n_out:
        raise NativeError(f'vnd_haas_each_stream_f64_host returned {got} frames, the span is {n_out}')
    return y


def polar_moments_workspace_bytes(n: int, pairs: int) -> int:
    return _query(load_library(), 'vnd_polar_moments_workspace_bytes', n, pairs)


def polar_moments_device(ctx: 'Context', y_ptr: int, n: int, pairs: int, moments_ptr: int, workspace_ptr: int,
                         workspace_bytes: int, stream: int = 0):
    """Reduce a device array ``y[n][2*pairs]`` to ``moments[pairs][8]`` (device doubles) on ``stream``."""
    _call(ctx._lib, 'vnd_polar_moments_f32_dev', ctx.handle, y_ptr, n, pairs, moments_ptr, workspace_ptr, workspace_bytes,
          stream)


def spec_kernel_source(tap_offsets, tap_index, tap_weight, mode: int = MODE_FAST) -> str:
    """HIP source of the per-table fast kernel the library would compile with hipRTC
    (``vnd_spec_kernel_source``; needs no device)."""
    offs = np.ascontiguousarray(tap_offsets, np.int32)
    idx = np.ascontiguousarray(tap_index, np.int32)
    w = np.ascontiguousarray(tap_weight, np.float32)
    lib = load_library()
    args = (len(offs) - 1, _ptr(offs, _i32), _ptr(idx, _i32), _ptr(w, _f32), int(mode))
    need = _query(lib, 'vnd_spec_kernel_source', *args, None, 0)
    buf = ctypes.create_string_buffer(need)
    _query(lib, 'vnd_spec_kernel_source', *args, buf, need)
    return buf.value.decode()


def window_kernel_source(tap_offsets, tap_index, tap_weight, mode: int = MODE_FAST, frames_per_lane: int = 32,
                         threads: int = 256, with_traffic: bool = False, *, seg_offsets=None, seg_end=None,
                         seg_gain=None, apply_gain: bool = False):
    """HIP source of the WINDOW form of the per-table kernel (``vnd_window_kernel_source``; needs no device).
    ``seg_*``: a class-path table as for ``TapTable.create``.  ``with_traffic``: also return (LDS bytes one lane
    reads per tile, (tap, output) products they feed)."""
    offs = np.ascontiguousarray(tap_offsets, np.int32)
    idx = np.ascontiguousarray(tap_index, np.int32)
    w = np.ascontiguousarray(tap_weight, np.float32)
    so = se = sg = None
    if seg_offsets is not None:
        so, se = np.ascontiguousarray(seg_offsets, np.int32), np.ascontiguousarray(seg_end, np.int32)
        sg = np.ascontiguousarray(seg_gain, np.float32)
    lib = load_library()
    need, lb, fm = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    args = (len(offs) - 1, _ptr(offs, _i32), _ptr(idx, _i32), _ptr(w, _f32), _ptr(so, _i32), _ptr(se, _i32), _ptr(sg, _f32),
            bool(apply_gain), int(mode), int(frames_per_lane), int(threads))
    _call(lib, 'vnd_window_kernel_source', *args, None, 0, ctypes.byref(need), ctypes.byref(lb), ctypes.byref(fm))
    buf = ctypes.create_string_buffer(need.value)
    _call(lib, 'vnd_window_kernel_source', *args, buf, need.value, ctypes.byref(need), None, None)
    src = buf.value.decode()
    return (src, lb.value, fm.value) if with_traffic else src


def code_object_private_bytes(image: bytes, kernel: str) -> int:
    """Private (scratch) bytes per lane of ``kernel`` in a gfx950 code object (``vnd_code_object_private_bytes``);
    -1 if the image has no such kernel."""
    return _query(load_library(), 'vnd_code_object_private_bytes', image, len(image), kernel.encode())


def host_buffers_mapped(x: np.ndarray, y: np.ndarray) -> bool:
    """True if a ``*_host`` convolution from ``x`` into ``y`` would run in place on the two buffers (both
    page-locked and mapped: ``vnd_host_buffers_mapped``)."""
    return bool(_query(load_library(), 'vnd_host_buffers_mapped', x.ctypes.data, x.nbytes, y.ctypes.data, y.nbytes,
                       out=ctypes.c_int32))


def device_count() -> int:
    n = ctypes.c_int32()
    rc = load_library().vnd_device_count(ctypes.byref(n))
    return n.value if rc == 0 else 0


_default_ctx: dict = {}
_default_ctx_lock = threading.Lock()


def context_for(device: int) -> Context:
    """The process-wide context of ``device`` (one per device, made on first use; ``multi.DevicePool`` runs one
    host thread per device through these)."""
    dev = int(device)
    with _default_ctx_lock:
        ctx = _default_ctx.get(dev)
        if ctx is None:
            ctx = _default_ctx[dev] = Context(dev)
    return ctx


def default_context() -> Context:
    """Process-wide context on ``VND_DEVICE`` / ``LOCAL_RANK`` / device 0."""
    dev = int(os.environ.get('VND_DEVICE', os.environ.get('LOCAL_RANK', '0')))
    n = device_count()
    if n > 0:
        dev %= n
    return context_for(dev)


def is_torch(x) -> bool:
    """Whether ``x`` is a torch tensor (without importing torch)."""
    return type(x).__module__.split('.')[0] == 'torch'


def torch_module():
    """torch, for device buffers and the current stream; ``RuntimeError`` without it or without a GPU."""
    try:
        import torch
    except ImportError as exc:            # pragma: no cover - the image ships torch
        raise RuntimeError('device-resident chains need torch for device buffers') from exc
    if not torch.cuda.is_available():
        raise RuntimeError('device-resident chains need a GPU (torch.cuda.is_available() is False)')
    return torch

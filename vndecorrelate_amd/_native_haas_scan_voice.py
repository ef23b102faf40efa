"""The wrappers of ``include/vnd_haas_scan_voice_stream.h`` - the voice pool that keeps each voice's last frames in a ring and
scores (slot, delay) pairs against them - on ``_native``'s one call path (``_call`` / ``_query``).

The prototypes are in ``_native.py`` with every other header's (``HAAS_SCAN_VOICE_STREAM_SIGNATURES``).  The wrapper functions
are here because ``tests/golden/native_calls.json`` records the wrappers defined in ``_native.py`` at an earlier commit;
``tests/test_haas_scan_voice_pool_cpu.py`` holds these to the header's prototypes instead, parameter by parameter.
"""
from __future__ import annotations

from ._native import _call, _query, _width, load_library


def haas_scan_voice_stream_state_bytes(slots: int, max_frames_per_call: int, window_frames: int, channels: int) -> int:
    """``vnd_haas_scan_voice_stream_state_bytes``: one int64 position, one int32 fill and one int32 head per slot (each part
    padded to 16 bytes), then the float32 ring of ``window_frames`` frames of ``channels`` values per slot."""
    return _query(load_library(), 'vnd_haas_scan_voice_stream_state_bytes', slots, max_frames_per_call, window_frames,
                  channels)


def haas_scan_voice_stream_reset_device(ctx: 'Context', state_ptr: int, state_bytes: int, slots: int,
                                        max_frames_per_call: int, window_frames: int, channels: int, *, stream: int = 0):
    """``vnd_haas_scan_voice_stream_reset_dev``: every position, fill and head of the pool to 0, enqueued on ``stream``; the
    rings are left alone."""
    _call(ctx._lib, 'vnd_haas_scan_voice_stream_reset_dev', ctx.handle, state_ptr, state_bytes, slots, max_frames_per_call,
          window_frames, channels, stream)


def haas_scan_voice_stream_push_device(ctx: 'Context', state_ptr: int, state_bytes: int, max_frames_per_call: int,
                                       window_frames: int, x_ptr: int, channels: int, counts_ptr: int, flags_ptr: int,
                                       valid_ptr: int, slots: int, *, stream: int = 0):
    """``vnd_haas_scan_voice_stream_push_f32_dev``: one call's frames into the rings.  ``x`` float32
    ``(slots, max_frames_per_call, channels)``, ``counts`` / ``flags`` / ``valid`` int32 ``(slots,)``, all device buffers
    of fixed shape; two kernels enqueued on ``stream``, nothing else."""
    _call(ctx._lib, 'vnd_haas_scan_voice_stream_push_f32_dev', ctx.handle, state_ptr, state_bytes, max_frames_per_call,
          window_frames, x_ptr, channels, counts_ptr, flags_ptr, valid_ptr, slots, stream)


def haas_scan_voice_stream_workspace_bytes(window_frames: int, n_pairs: int, max_delay: int) -> int:
    """``vnd_haas_scan_voice_stream_workspace_bytes``: the workspace of one pairs call of ``n_pairs`` pairs whose delays are
    at most ``max_delay`` frames."""
    return _query(load_library(), 'vnd_haas_scan_voice_stream_workspace_bytes', window_frames, n_pairs, int(max_delay))


def haas_scan_voice_stream_pairs_device(ctx: 'Context', state_ptr: int, state_bytes: int, max_frames_per_call: int,
                                        window_frames: int, channels: int, slots: int, slots_of_pair_ptr: int,
                                        delays_ptr: int, n_pairs: int, moments_ptr: int, *, max_delay: int,
                                        delayed_channel: int, ms_mode: bool, width, workspace_ptr: int, workspace_bytes: int,
                                        stream: int = 0):
    """``vnd_haas_scan_voice_stream_pairs_f64_dev``: the eight float64 moments of ``n_pairs`` (slot, delay) pairs, each
    scored against its slot's window; the int32 pair arrays, ``moments`` ``(n_pairs, 8)`` and the workspace are device
    buffers; two kernels enqueued on ``stream``, nothing else."""
    _call(ctx._lib, 'vnd_haas_scan_voice_stream_pairs_f64_dev', ctx.handle, state_ptr, state_bytes, max_frames_per_call,
          window_frames, channels, slots, slots_of_pair_ptr, delays_ptr, n_pairs, int(max_delay), int(delayed_channel),
          bool(ms_mode), *_width(width), moments_ptr, workspace_ptr, workspace_bytes, stream)

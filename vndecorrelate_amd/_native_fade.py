"""The wrappers of ``include/vnd_voice_fade_stream.h`` - the voice pool whose live voices change their filter, crossfaded -
and of its describe hook, on ``_native``'s one call path (``_call`` / ``_query`` / ``_describe``).

The prototypes and constants are in ``_native.py`` with every other header's (``VOICE_FADE_STREAM_SIGNATURES``,
``VOICE_SWITCH``, ``VOICE_FADE_MAX_FRAMES``).  The wrapper functions are here because ``tests/golden/native_calls.json``
records the wrappers defined in ``_native.py`` at an earlier commit; ``tests/test_voice_fade_pool_cpu.py`` holds these to
the header's prototypes instead, parameter by parameter.
"""
from __future__ import annotations

from . import _native
from ._native import MODE_EXACT, _call, _describe, _query, _width, load_library

VOICE_SWITCH, VOICE_FADE_MAX_FRAMES = _native.VOICE_SWITCH, _native.VOICE_FADE_MAX_FRAMES


def voice_fade_stream_state_bytes(bank: 'TapTable', slots: int, channels: int, max_frames_per_call: int,
                                  fade_frames: int) -> int:
    """``vnd_voice_fade_stream_state_bytes``: one int64 position per slot (padded to 16 bytes), one 16-byte record
    ``(int64 s, int32 old, int32 cur)`` per slot, then the ring of a pool of ``slots`` voices at the bank's latency."""
    return _query(load_library(), 'vnd_voice_fade_stream_state_bytes', bank.handle, slots, channels, max_frames_per_call,
                  fade_frames)


def voice_fade_stream_reset_device(ctx: 'Context', bank: 'TapTable', state_ptr: int, state_bytes: int, slots: int,
                                   channels: int, max_frames_per_call: int, fade_frames: int, *, stream: int = 0):
    """``vnd_voice_fade_stream_reset_dev``: every position of the pool to 0, enqueued on ``stream``; the records and the
    ring are left alone."""
    _call(ctx._lib, 'vnd_voice_fade_stream_reset_dev', ctx.handle, state_ptr, state_bytes, slots, channels, bank.handle,
          max_frames_per_call, fade_frames, stream)


def voice_fade_stream_device(ctx: 'Context', bank: 'TapTable', state_ptr: int, state_bytes: int, max_frames_per_call: int,
                             fade_frames: int, gains_ptr: int, x_ptr: int, counts_ptr: int, flags_ptr: int, tables_ptr: int,
                             y_ptr: int, out_counts_ptr: int, fade_left_ptr: int, slots: int, channels: int, *,
                             ms_encode: bool, width, mode: int = MODE_EXACT, stream: int = 0):
    """``vnd_voice_fade_stream_f32_dev``: one call of a crossfading voice pool.  The buffers of ``voice_stream_device``,
    the float32 ``(2, fade_frames)`` gains (fade-out, fade-in; None only with ``fade_frames == 0``) and the int32
    ``(slots,)`` ``fade_left`` (or None) are device buffers of fixed shape; flags carry ``VOICE_START``, ``VOICE_END`` and
    ``VOICE_SWITCH``; two kernels enqueued on ``stream``, nothing else."""
    _call(ctx._lib, 'vnd_voice_fade_stream_f32_dev', ctx.handle, bank.handle, state_ptr, state_bytes, max_frames_per_call,
          fade_frames, gains_ptr, x_ptr, counts_ptr, flags_ptr, tables_ptr, y_ptr, out_counts_ptr, fade_left_ptr, slots,
          channels, int(mode), bool(ms_encode), *_width(width), stream)


def describe_voice_fade_stream(bank: 'TapTable', max_frames_per_call: int, fade_frames: int, slots: int, channels: int,
                               mode: int = MODE_EXACT, epilogue: bool = False) -> str:
    """The launch of every ``vnd_voice_fade_stream_f32_dev`` call on a pool of ``slots`` voices over ``bank``
    (``vnd_describe_voice_fade_stream_launch``): ``describe_voice_stream``'s fields, then ``fade_frames=``."""
    return _describe(bank._lib, 'vnd_describe_voice_fade_stream_launch', bank.ctx.handle, bank.handle, max_frames_per_call,
                     fade_frames, slots, channels, int(mode), bool(epilogue))


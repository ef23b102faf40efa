"""The wrappers of ``include/vnd_haas_voice_fade_stream.h`` - the Haas voice pool whose live voices change their delay,
crossfaded - on ``_native``'s one call path (``_call`` / ``_query``).

The prototypes are in ``_native.py`` with every other header's (``HAAS_VOICE_FADE_STREAM_SIGNATURES``; ``VOICE_SWITCH`` and
``VOICE_FADE_MAX_FRAMES`` are ``vnd_voice_fade_stream.h``'s).  The wrapper functions are here because
``tests/golden/native_calls.json`` records the wrappers defined in ``_native.py`` at an earlier commit;
``tests/test_haas_voice_fade_pool_cpu.py`` holds these to the header's prototypes instead, parameter by parameter.
"""
from __future__ import annotations

from . import _native
from ._native import _call, _query, _width, load_library

VOICE_SWITCH, VOICE_FADE_MAX_FRAMES = _native.VOICE_SWITCH, _native.VOICE_FADE_MAX_FRAMES


def haas_voice_fade_stream_state_bytes(slots: int, channels: int, max_delay: int, max_frames_per_call: int,
                                       fade_frames: int) -> int:
    """``vnd_haas_voice_fade_stream_state_bytes``: one int64 position per slot (padded to 16 bytes), one 16-byte record
    ``(int64 s, int32 old, int32 cur)`` per slot - the delays in frames - then the ring of a pool of ``slots`` voices with
    delays up to ``max_delay``."""
    return _query(load_library(), 'vnd_haas_voice_fade_stream_state_bytes', slots, channels, int(max_delay),
                  max_frames_per_call, fade_frames)


def haas_voice_fade_stream_reset_device(ctx: 'Context', state_ptr: int, state_bytes: int, slots: int, channels: int,
                                        max_delay: int, max_frames_per_call: int, fade_frames: int, *, stream: int = 0):
    """``vnd_haas_voice_fade_stream_reset_dev``: every position of the pool to 0, enqueued on ``stream``; the records and
    the ring are left alone."""
    _call(ctx._lib, 'vnd_haas_voice_fade_stream_reset_dev', ctx.handle, state_ptr, state_bytes, slots, channels,
          int(max_delay), max_frames_per_call, fade_frames, stream)


def haas_voice_fade_stream_device(ctx: 'Context', state_ptr: int, state_bytes: int, max_frames_per_call: int,
                                  fade_frames: int, gains_ptr: int, x_ptr: int, counts_ptr: int, flags_ptr: int,
                                  delays_ptr: int, y_ptr: int, out_counts_ptr: int, fade_left_ptr: int, slots: int,
                                  channels: int, *, max_delay: int, delayed_channel: int, ms_mode: bool, width,
                                  stream: int = 0):
    """``vnd_haas_voice_fade_stream_f64_dev``: one call of a crossfading Haas voice pool.  The buffers of
    ``haas_voice_stream_device``, the float32 ``(2, fade_frames)`` gains (fade-out, fade-in; None only with
    ``fade_frames == 0``) and the int32 ``(slots,)`` ``fade_left`` (or None) are device buffers of fixed shape; flags
    carry ``VOICE_START``, ``VOICE_END`` and ``VOICE_SWITCH``; two kernels enqueued on ``stream``, nothing else."""
    _call(ctx._lib, 'vnd_haas_voice_fade_stream_f64_dev', ctx.handle, state_ptr, state_bytes, max_frames_per_call,
          fade_frames, gains_ptr, x_ptr, counts_ptr, flags_ptr, delays_ptr, y_ptr, out_counts_ptr, fade_left_ptr, slots,
          channels, int(max_delay), int(delayed_channel), bool(ms_mode), *_width(width), stream)

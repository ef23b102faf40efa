"""CPU tier of the tap-table gate: every refusal of ``vnd_taps_create`` and ``vnd_taps_deserialize``, without a device.
The gate finishes validating before it touches the context, so a context pointer that must never be followed stands in
for one (as in tests/test_white_noise_cpu.py).  What each call must answer comes from the mirror of the contract in
tests/taps_gate.py; only what the mirror refuses is sent here.  The tables the gate admits are the GPU tier's
(tests/test_gpu_taps_gate.py)."""
import ctypes
import struct

import numpy as np
import pytest

import taps_gate as G


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as entry
    entry.build()
    from vndecorrelate_amd import _native
    return _native.load_library()


FAKE_CTX = ctypes.c_void_p(0x1000)
CORPUS = G.refusal_corpus()
LISTED = [c for c in CORPUS if c.group == 'listed']
MUTANTS = [c for c in CORPUS if c.group == 'mutant']


def _replay(lib, cases):
    seen = {}
    for case in cases:
        assert not case.verdict.admitted, case.name                 # nothing admitted may meet the fake context
        status, message, left = G.call_case(lib, FAKE_CTX, case)
        assert status == case.verdict.status, (case.name, status, message)
        assert message, case.name
        assert message == case.verdict.reason, (case.name, message)
        if not case.null_out:
            assert left is None, (case.name, left)                  # *taps == NULL
        seen.setdefault((case.entry, message), case.name)
    return seen


def test_the_mirror_alone_covers_every_refusal_message():
    """Before any native call: the corpus holds a case for every distinct refusal of either entry (the create refusals also
    as images, where an image can express them), of both statuses."""
    of_create = {c.verdict.reason for c in CORPUS if c.entry == 'create'}
    of_image = {c.verdict.reason for c in CORPUS if c.entry == 'image'}
    assert of_create == set(G.CREATE_REASONS)
    image_cannot_say = {G.R_CHANNELS, G.R_NULL_TAP_OFF, G.R_NULL_TAPS, G.R_SEG_INCOMPLETE}      # (null arrays; its C is the header's)
    assert of_image == set(G.IMAGE_REASONS) | (set(G.CREATE_REASONS) - image_cannot_say)
    assert {c.verdict.status for c in CORPUS} == {G.INVALID, G.UNSUPPORTED}
    assert len(MUTANTS) > 500 and len(LISTED) > 100


def test_every_listed_refusal(lib):
    seen = _replay(lib, LISTED)
    # every distinct refusal message of the two entries was produced - the list is this test's own, not the mirror's
    assert {m for e, m in seen if e == 'create'} == {
        'null out pointer', 'null context', 'num_channels # out of range', 'null tap_offsets', 'tap_offsets[#] must be #',
        'tap_offsets not monotone', 'null tap arrays', 'negative tap index at #', 'tap index # at # is beyond #^# frames',
        'segment table incomplete', 'seg_offsets[#] must be #', 'seg_offsets not monotone', 'segment # of channel # out of order',
        'segments of channel # do not cover its taps'}
    assert {m for e, m in seen if e == 'image'} >= {
        'null out pointer', 'tap image too short', 'tap image is not #-byte aligned', 'not a tap image of this format version',
        'corrupt tap image header', 'tap image truncated', 'corrupt tap image', 'null context'}


def test_every_refused_mutant(lib):
    """One word of a valid image changed, or its tail cut: whatever the mirror refuses, the entry refuses alike."""
    seen = _replay(lib, MUTANTS)
    assert {m for _, m in seen} >= {'tap image too short', 'not a tap image of this format version', 'corrupt tap image header',
                                    'tap image truncated', 'corrupt tap image', 'tap_offsets[#] must be #', 'tap_offsets not monotone',
                                    'negative tap index at #', 'tap index # at # is beyond #^# frames', 'seg_offsets[#] must be #',
                                    'seg_offsets not monotone', 'segment # of channel # out of order',
                                    'segments of channel # do not cover its taps'}


def test_mirror_reads_images_as_taps_py_does():
    """The mirror's image layout is the package's own (taps.TapArrays): same bytes out, same arrays back."""
    from vndecorrelate_amd.taps import TapArrays
    for t in G.small_tables() + [t for t in G.edge_tables() if t.total]:
        arrays = TapArrays(t.tap_offsets, t.tap_index, t.tap_weight, t.seg_offsets, t.seg_end, t.seg_gain, t.chan_flags, bool(t.apply_gain))
        image = t.to_bytes()
        assert image == arrays.to_bytes(), t.name
        verdict, back = G.parse_image(image)
        assert verdict.admitted and G.judge_image(image).admitted
        again = TapArrays.from_bytes(image)
        for f in ('tap_offsets', 'tap_index', 'tap_weight', 'seg_offsets', 'seg_end', 'seg_gain', 'chan_flags'):
            a, b = getattr(back, f), getattr(again, f)
            assert (a is None) == (b is None) and (a is None or a.tobytes() == b.tobytes()), (t.name, f)


def test_header_words_are_widened_before_they_are_added(lib):
    """C = INT_MAX with the flags bit set: (C + 3) / 4 and 8 + (C + 1) overflowed in int32 (undefined behaviour that
    happened to answer "truncated"); the channel count is now refused from the header, before any arithmetic."""
    for C in (G.INT_MAX, G.INT_MAX - 1, 65536):
        case = G.image_case('C', G.header_image(C, 0, 0, 1, 1))
        assert G.call_case(lib, FAKE_CTX, case) == (G.INVALID, G.R_IMG_HEADER, None)
    # 65535 channels is the most an image may announce: then the length decides
    case = G.image_case('C', G.header_image(65535, 0, 0, 1, 1))
    assert G.call_case(lib, FAKE_CTX, case) == (G.INVALID, G.R_IMG_TRUNCATED, None)


def test_misaligned_image_is_refused_not_read(lib):
    """include/vnd_amd.h asks for a 4-byte aligned buffer: at any other address INVALID, whatever the bytes hold."""
    image = G.base_stereo().to_bytes()
    for case in (G.image_case('valid', image, misaligned=True), G.image_case('garbage', b'\xff' * 64, misaligned=True)):
        assert G.call_case(lib, FAKE_CTX, case) == (G.INVALID, G.R_IMG_ALIGN, None)


# ---- the Python wrappers --------------------------------------------------------------------------------------------------
class _Lib:
    """Stands in for the library: a wrapper that reaches it has not refused."""
    def __getattr__(self, name):
        raise AssertionError(f'{name} was called')


def test_wrapper_refuses_short_arrays_before_calling_c():
    from vndecorrelate_amd import _native
    ctx = type('C', (), {'_lib': _Lib(), 'handle': None})()
    b = G.base_stereo()
    good = dict(tap_offsets=b.tap_offsets, tap_index=b.tap_index, tap_weight=b.tap_weight, **b.kwargs())
    with pytest.raises(AssertionError, match='vnd_taps_create was called'):       # the valid table does reach the library
        _native.TapTable.create(ctx, **good)
    bad = [dict(tap_index=b.tap_index[:-1]), dict(tap_weight=b.tap_weight[:-1]), dict(tap_index=np.zeros(0, np.int32)),
           dict(tap_index=None), dict(tap_weight=None),
           dict(seg_end=b.seg_end[:-1]), dict(seg_gain=b.seg_gain[:-1]), dict(seg_end=None), dict(seg_gain=None),
           dict(seg_offsets=b.seg_offsets[:-1]), dict(seg_offsets=np.append(b.seg_offsets, 4)),
           dict(chan_flags=b.chan_flags[:-1]), dict(chan_flags=np.zeros(0, np.uint8)),
           dict(tap_offsets=np.zeros(1, np.int32)), dict(tap_offsets=np.zeros(0, np.int32))]
    for change in bad:
        with pytest.raises(ValueError):
            _native.TapTable.create(ctx, **{**good, **change})
    for image in (b'', bytearray(), memoryview(b'')):
        with pytest.raises(ValueError):
            _native.TapTable.from_bytes(ctx, image)


def test_wrapper_maps_the_gate_to_valueerror(lib):
    """With the real library behind a context that is never reached: INVALID is ValueError, UNSUPPORTED NativeError."""
    from vndecorrelate_amd import _native
    ctx = type('C', (), {'_lib': lib, 'handle': FAKE_CTX})()
    b = G.base_stereo()
    with pytest.raises(ValueError, match='do not cover'):
        _native.TapTable.create(ctx, b.tap_offsets, b.tap_index, b.tap_weight, **{**b.kwargs(), 'seg_end': [2, 3, 4, 5]})
    far = b.tap_index.copy()
    far[-1] = G.MAX_INDEX + 1
    with pytest.raises(_native.NativeError, match='beyond 2\\^30'):
        _native.TapTable.create(ctx, b.tap_offsets, far, b.tap_weight, **b.kwargs())
    with pytest.raises(ValueError, match='truncated'):
        _native.TapTable.from_bytes(ctx, b.to_bytes()[:-4])
    with pytest.raises(ValueError, match='too short'):
        _native.TapTable.from_bytes(ctx, struct.pack('<7i', G.MAGIC, G.IMAGE_VERSION, 1, 0, 0, 0, 0))

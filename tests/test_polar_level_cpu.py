"""CPU tier of the polar level envelope (include/vnd_level.h, vectorscope.polar_level_batched): NumPy's percentile rule in
one pure function against np.percentile bit for bit, the NumPy route against the fixture recorded from the reference's
_build_pseudo_hull, the argument errors, the routing, and the header against its binding and its refusals - no device
call."""
import ctypes
import json
import pathlib
import re

import numpy as np
import pytest

REPO = pathlib.Path(__file__).resolve().parents[1]
HEADER = REPO / 'include' / 'vnd_level.h'
GOLDEN = REPO / 'tests' / 'golden'
NAMES = ['vnd_polar_level_f32_dev', 'vnd_polar_level_f64_dev', 'vnd_polar_level_work_bytes']
INVALID, UNSUPPORTED = 1, 4
PS = (0, 12.5, 50, 95, 99.9, 100)


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as entry
    entry.build()
    from vndecorrelate_amd import _native
    return _native.load_library()


@pytest.fixture
def vs():
    from vndecorrelate_amd import vectorscope
    vectorscope.set_scope_device(False)
    yield vectorscope
    vectorscope.set_scope_device(None)


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN / 'polar_level.npz'), json.loads((GOLDEN / 'polar_level_manifest.json').read_text())


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- the percentile rule ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_the_rule_and_a_sort_are_np_percentile(vs, dtype):
    rng = np.random.default_rng(0)
    sizes = list(range(1, 40)) + [63, 64, 65, 100, 101, 255, 256, 257, 999, 1000, 1001, 2047, 2048, 2049, 4999, 5000]
    checked = 0
    for m in sizes:
        for ties in (False, True):
            a = rng.standard_normal(m).astype(dtype) ** 2
            if ties:
                a = np.round(a * 4).astype(dtype) / dtype(4)       # a handful of distinct values
            s = np.sort(a)
            for p in PS:
                want = np.percentile(a, p)
                got = vs.percentile_of_sorted(s, p)
                assert type(want) is type(got) and _same_bits(got, want), (m, ties, p, got, want)
                prev, nxt, g = vs.percentile_rule(m, p, dtype)
                assert 0 <= prev <= nxt <= m - 1 and nxt - prev <= 1 and type(g) is dtype and 0 <= g < 1
                checked += 1
    assert checked == len(sizes) * 2 * len(PS)
    assert vs.percentile_rule(1, 95.0, dtype) == (0, 0, 0) and vs.percentile_rule(5, 100, dtype) == (4, 4, 0)
    assert vs.percentile_rule(5, 50, dtype) == (2, 3, 0) and vs.percentile_rule(4, 50, dtype) == (1, 2, 0.5)
    for bad in (-0.001, 100.001, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='Percentiles must be in the range'):
            vs.percentile_rule(10, bad, dtype)
        with pytest.raises(ValueError, match='Percentiles must be in the range'):
            np.percentile(np.ones(3, dtype), bad)
    for bad in (0, -1, True, 2.0):
        with pytest.raises(ValueError, match='positive integer'):
            vs.percentile_rule(bad, 50, dtype)


def test_the_rule_above_two_to_the_24_float32_values(vs):
    """m - 1 = 2^24 + 3 is no float32: T(m - 1) is rounded to nearest before the multiply, as NumPy rounds it."""
    m = 16777220
    assert int(np.float32(m - 1)) != m - 1
    a = np.random.default_rng(1).random(m, dtype=np.float32)
    for p in (12.5, 50, 95, 99.9, 100):
        want = np.percentile(a, p)
        prev, nxt, g = vs.percentile_rule(m, p, np.float32)
        assert 0 <= prev <= nxt <= m - 1
        part = np.partition(a, [prev, nxt])
        d = part[nxt] - part[prev]
        got = part[nxt] - d * (np.float32(1) - g) if g >= np.float32(0.5) else part[prev] + d * g
        assert _same_bits(got, want), (p, got, want)


# ---- the NumPy route -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['f32', 'f64'])
def test_the_numpy_route_is_the_references_envelope(vs, golden, name):
    arrays, manifest = golden
    frames, want = arrays[f'{name}__frames'], arrays[f'{name}__levels']
    case = manifest['cases'][name]
    assert frames.dtype == np.dtype(case['dtype']) and frames.shape == (manifest['frames'], 2)
    levels, counts, edges, centers = vs.polar_level_batched(frames, manifest['num_bins'], manifest['percentiles'])
    assert levels.dtype == np.float64 and counts.dtype == np.int64
    assert _same_bits(levels, want)
    assert _same_bits(edges, np.linspace(-90.0, 90.0, 361)) and _same_bits(centers, 0.5 * (edges[:-1] + edges[1:]))
    # the empty slices are 0.0, the anti-phase frames at +90.0 are in no slice, -90.0 is in slice 0, mono frames in slice 180
    assert int((counts == 0).sum()) == case['empty_bins'] == 20 and (levels[:, counts == 0] == 0).all()
    assert (levels[:, counts > 0] > 0).all()
    assert case['frames_at_plus_90'] == 2 and counts.sum() == len(frames) - 2
    one = frames.copy()
    one[:] = (0.25, -0.25)
    assert vs.polar_level_batched(one)[1].sum() == 0 and not vs.polar_level_batched(one)[0].any()
    one[:] = (-0.25, 0.25)
    assert vs.polar_level_batched(one)[1][0] == len(one)
    one[:] = (-0.5, -0.5)
    assert vs.polar_level_batched(one)[1][180] == len(one)
    # the values are sample-type values held in float64
    assert _same_bits(levels.astype(frames.dtype).astype(np.float64), levels)
    # the defaults are the reference's two calls
    assert _same_bits(vs.polar_level_batched(frames)[0], want)


def test_the_numpy_route_against_the_rule(vs):
    """Every slice by the mask, a sort and percentile_rule, for a batch, a fixed scale, LR and the whole circle."""
    from oracle import vnd_oracle as O
    rng = np.random.default_rng(3)
    pool = np.stack([rng.standard_normal((700, 2)) * s for s in (0.02, 0.2, 2.0)]).astype(np.float32)
    ps = (0, 50, 95, 99.9, 100)
    for kw, okw in ((dict(), dict()), (dict(radius_scale=1.5), dict(normalize=False)), (dict(mode='LR'), dict(mode='LR')),
                    (dict(semicircular=False), dict(semicircular=False))):
        levels, counts, edges, _ = vs.polar_level_batched(pool, 36, ps, **kw)
        assert levels.shape == (3, 5, 36) and counts.shape == (3, 36)
        for b in range(3):
            radii, thetas, _ = O.polar_coordinates(pool[b, :, 0], pool[b, :, 1], **okw)
            if 'radius_scale' in kw:
                radii = radii / np.float32(1.5)
            degrees = np.degrees(thetas)
            for k in range(36):
                inside = np.sort(radii[(degrees >= edges[k]) & (degrees < edges[k + 1])])
                assert counts[b, k] == len(inside)
                for i, p in enumerate(ps):
                    want = vs.percentile_of_sorted(inside, p) if len(inside) else 0.0
                    assert levels[b, i, k] == np.float64(want)
    assert counts.sum() < 3 * 700                                  # the whole circle: frames outside [-90, 90) are dropped


def test_shapes_counts_and_argument_errors(vs):
    sig = (np.random.default_rng(4).standard_normal((500, 2)) * 0.3).astype(np.float32)
    levels, counts, edges, centers = vs.polar_level_batched(sig, 12, (95.0,))
    assert levels.shape == (1, 12) and counts.shape == (12,) and edges.shape == (13,) and centers.shape == (12,)
    batched = vs.polar_level_batched(sig[None], 12, (95.0,))
    assert batched[0].shape == (1, 1, 12) and _same_bits(batched[0][0], levels) and _same_bits(batched[1][0], counts)
    assert _same_bits(vs.polar_level_batched(sig, 12, 95.0)[0], levels)              # a scalar percentile
    # counts outside [0, n] contribute no frame
    pool = np.stack([sig] * 5)
    got, got_counts, _, _ = vs.polar_level_batched(pool, 12, (95.0, 50.0), counts=np.array([0, 17, 500, 501, -1], np.int32))
    assert [int(c.sum()) for c in got_counts] == [0, 17, 500, 0, 0]
    assert not got[0].any() and not got[3].any() and not got[4].any()
    assert _same_bits(got[1], vs.polar_level_batched(sig[:17], 12, (95.0, 50.0))[0])  # its own maximum over 17 frames
    assert _same_bits(got[2], vs.polar_level_batched(sig, 12, (95.0, 50.0))[0])
    with pytest.raises(ValueError, match='one entry per signal'):
        vs.polar_level_batched(pool, 12, counts=np.array([1, 2], np.int32))
    for bad in ((101.0,), (-1.0, 50.0), (float('nan'),)):
        with pytest.raises(ValueError, match='Percentiles must be in the range'):
            vs.polar_level_batched(sig, 12, bad)
    with pytest.raises(ValueError, match='at least one'):
        vs.polar_level_batched(sig, 12, ())
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError, match='num_bins'):
            vs.polar_level_batched(sig, bad)
    for bad in (0.0, -1.0, float('inf'), float('nan')):
        with pytest.raises(ValueError, match='radius_scale'):
            vs.polar_level_batched(sig, 12, radius_scale=bad)
    with pytest.raises(ValueError, match='mode'):
        vs.polar_level_batched(sig, 12, mode='XY')
    with pytest.raises(ValueError, match='pool must be'):
        vs.polar_level_batched(sig[:, :1], 12)
    with pytest.raises(TypeError):
        vs.polar_level_batched(sig, 12, accumulate=True)            # percentiles of blocks do not add up


def test_uncovered_calls_keep_the_numpy_loop(vs):
    """With the device demanded, a call the device does not cover still takes the NumPy loop; a covered one needs a device."""
    assert vs.level_covers(np.float32, 3, 1000, 360, 2) and vs.level_covers(np.float64, 1, 1, 1024, 4)
    assert not vs.level_covers(np.float32, 3, 1000, 1025, 2) and not vs.level_covers(np.float32, 3, 1000, 360, 5)
    assert not vs.level_covers(np.float16, 3, 1000, 360, 2) and not vs.level_covers(np.int16, 3, 1000, 360, 2)
    assert not vs.level_covers(np.float32, 65536, 1000, 360, 2) and not vs.level_covers(np.float32, 1, 2 ** 32, 360, 2)
    sig = (np.random.default_rng(5).standard_normal((300, 2)) * 0.3).astype(np.float32)
    want5 = vs.polar_level_batched(sig, 8, (0, 25, 50, 75, 100))
    want_wide = vs.polar_level_batched(sig, 1025, (50,))
    halves = sig.astype(np.float16)
    want_halves = vs.polar_level_batched(halves, 8)
    vs.set_scope_device(True)
    got5 = vs.polar_level_batched(sig, 8, (0, 25, 50, 75, 100))     # five percentiles
    assert _same_bits(got5[0], want5[0]) and _same_bits(got5[1], want5[1])
    assert _same_bits(vs.polar_level_batched(sig, 1025, (50,))[0], want_wide[0])
    assert _same_bits(vs.polar_level_batched(halves, 8)[0], want_halves[0]) and want_halves[1].sum() > 0
    from vndecorrelate_amd.analysis import _gpu_present
    if not _gpu_present():
        with pytest.raises(RuntimeError, match='set_scope_device'):
            vs.polar_level_batched(sig, 8)


def test_the_package_exports_it():
    import vndecorrelate_amd
    from vndecorrelate_amd import analysis, vectorscope
    assert vndecorrelate_amd.polar_level_batched is vectorscope.polar_level_batched is analysis.polar_level_batched
    assert 'polar_level_batched' in vectorscope.__all__ and 'percentile_rule' in vectorscope.__all__


# ---- the header and its binding --------------------------------------------------------------------------------------
def test_header_binding_and_library_agree(lib):
    from vndecorrelate_amd import vectorscope
    text = re.sub(r'/\*.*?\*/', '', HEADER.read_text(), flags=re.S)
    assert sorted(set(re.findall(r'\b(vnd_[a-z0-9_]+)\s*\(', text))) == NAMES
    for name in NAMES:
        assert hasattr(lib, name)
    for define, value in (('VND_LEVEL_MAX_BINS', vectorscope.LEVEL_MAX_BINS),
                          ('VND_LEVEL_MAX_PERCENTILES', vectorscope.LEVEL_MAX_PERCENTILES),
                          ('VND_LEVEL_SPAN_FRAMES', vectorscope.LEVEL_SPAN_FRAMES)):
        assert int(re.search(r'#define %s (\d+)' % define, text).group(1)) == value
    assert vectorscope.LEVEL_MAX_PERCENTILES == 4 and 360 <= vectorscope.LEVEL_MAX_BINS <= vectorscope.MAX_BINS
    assert 'accumulate' in HEADER.read_text()                       # the header says why there is none


P = 1 << 24            # a made-up device address: nothing below reaches a device
HOST_PS = (ctypes.c_double * 8)(95.0, 50.0, 0.0, 100.0, 99.9, 12.5, 1.0, 2.0)


def _level(lib, f64=False, *, ctx=0, l=P, r=P + 8, batch=3, n=100, ss=200, fs=2, ms=1, semi=1, scale=0.0, edges=5 * P, bins=360,
           ps=HOST_PS, num_p=2, each=0, levels=2 * P, counts=3 * P, work=8 * P, work_bytes=None):
    if work_bytes is None:
        need = ctypes.c_int64()
        ok = lib.vnd_polar_level_work_bytes(batch, n, bins, num_p, int(f64), ctypes.byref(need))
        work_bytes = need.value if ok == 0 else 1 << 40
    fn = lib.vnd_polar_level_f64_dev if f64 else lib.vnd_polar_level_f32_dev
    return fn(ctx, l, r, batch, n, ss, fs, ms, semi, scale, edges, bins, ps, num_p, each, levels, counts, work, work_bytes, None)


@pytest.mark.parametrize('f64', [False, True])
def test_checks_that_need_no_device(lib, f64):
    err = lib.vnd_last_error
    # valid arguments reach the last check: the context
    assert _level(lib, f64) == INVALID and b'null context' in err()
    assert _level(lib, f64, scale=1.5, each=7 * P, num_p=4, bins=1024) == INVALID and b'null context' in err()
    assert _level(lib, f64, bins=1, num_p=1) == INVALID and b'null context' in err()
    # null pointers
    for name in ('l', 'r', 'edges', 'ps', 'levels', 'counts', 'work'):
        assert _level(lib, f64, **{name: None if name == 'ps' else 0}) == INVALID and b'null' in err() \
            and b'context' not in err(), name
    # sizes below 1
    for name in ('batch', 'n', 'ss', 'fs', 'bins', 'num_p'):
        for bad in (0, -1):
            assert _level(lib, f64, **{name: bad}, work_bytes=1 << 40) == INVALID and b'>= 1' in err(), (name, bad)
    # percentiles
    for bad in (-0.5, 100.5, float('nan'), float('inf')):
        assert _level(lib, f64, ps=(ctypes.c_double * 2)(50.0, bad)) == INVALID and b'percentile' in err(), bad
    # scales
    assert _level(lib, f64, scale=float('nan')) == INVALID and b'NaN' in err()
    assert _level(lib, f64, scale=float('inf')) == INVALID and b'radius_scale' in err()
    if not f64:
        assert _level(lib, f64, scale=1e-60) == INVALID and b'radius_scale' in err()
        assert _level(lib, f64, scale=1e60) == INVALID and b'radius_scale' in err()
    # work memory
    need = ctypes.c_int64()
    assert lib.vnd_polar_level_work_bytes(3, 100, 360, 2, int(f64), ctypes.byref(need)) == 0
    assert _level(lib, f64, work_bytes=need.value - 1) == INVALID and b'work of' in err()
    assert _level(lib, f64, work_bytes=need.value) == INVALID and b'null context' in err()
    assert _level(lib, f64, work=8 * P + 4) == INVALID and b'aligned' in err()
    # overlapping buffers: the frames span 3 * 200 samples from P
    inside = P + 100 * (8 if f64 else 4)
    for name in ('levels', 'counts', 'work'):
        assert _level(lib, f64, **{name: inside}) == INVALID and b'overlap' in err(), name
    assert _level(lib, f64, levels=5 * P + 8) == INVALID and b'edges' in err()
    assert _level(lib, f64, counts=5 * P + 361 * 8 - 4) == INVALID and b'overlap' in err()
    assert _level(lib, f64, counts=5 * P + 361 * 8) == INVALID and b'null context' in err()     # just past the edges: clean
    assert _level(lib, f64, each=3 * P + 64) == INVALID and b'n_each' in err()
    assert _level(lib, f64, counts=2 * P + 8) == INVALID and b'one another' in err()
    assert _level(lib, f64, work=3 * P + 16) == INVALID and b'one another' in err()
    assert _level(lib, f64, levels=8 * P + need.value - 8) == INVALID and b'one another' in err()
    # what the launch does not take
    big = 2 ** 32
    assert _level(lib, f64, n=big, ss=2 * big) == UNSUPPORTED and b'uint32' in err()
    assert _level(lib, f64, bins=1025) == UNSUPPORTED and b'bins' in err()
    assert _level(lib, f64, num_p=5) == UNSUPPORTED and b'percentiles' in err()
    assert _level(lib, f64, batch=65536, ss=1, fs=1, n=1) == UNSUPPORTED
    assert _level(lib, f64, batch=65535, n=2 ** 24, ss=1, fs=1) == UNSUPPORTED and b'workgroups' in err()
    # an invalid argument is reported before an unsupported shape
    assert _level(lib, f64, bins=1025, scale=float('nan')) == INVALID
    assert _level(lib, f64, num_p=5, ps=(ctypes.c_double * 5)(1, 2, 3, 4, 101)) == INVALID


def test_work_bytes(lib):
    from vndecorrelate_amd import _native
    got = ctypes.c_int64(-7)
    sizes = {}
    for f64 in (0, 1):
        # the maximum, three 8-byte words and two 4-byte words a cell, 2^d counters a cell, a key and a uint16 a frame; the
        # digit width d is 5 where 360 x 2 x 2^5 counters fit LDS, less where a signal has fewer than 8 frames a counter
        cells = 3 * 360 * 2
        for n, d in ((100, 1), (359, 1), (360, 2), (1000, 3), (2879, 4), (2880, 5), (100000, 5)):
            assert lib.vnd_polar_level_work_bytes(3, n, 360, 2, f64, ctypes.byref(got)) == 0
            frames = 3 * n
            assert got.value == 24 + cells * (24 + 8 + 4 * 2 ** d) + (frames * (8 if f64 else 4) + 7) // 8 * 8 \
                + (frames * 2 + 7) // 8 * 8, (n, d)
            assert got.value % 8 == 0
        assert lib.vnd_polar_level_work_bytes(3, 1000, 360, 2, f64, ctypes.byref(got)) == 0
        sizes[f64] = got.value
    assert lib.vnd_polar_level_work_bytes(1, 10 ** 6, 1, 1, 0, ctypes.byref(got)) == 0             # one cell: d = 8, the widest
    assert got.value == 8 + (24 + 2 * 8 + 4 * 256) + 4 * 10 ** 6 + 2 * 10 ** 6                     # (each section 8-byte aligned)
    assert _native.polar_level_work_bytes(3, 1000, 360, 2, True) == sizes[1] > sizes[0]
    for bad in ((0, 10, 360, 2), (1, 0, 360, 2), (1, 10, 0, 2), (1, 10, 360, 0)):
        assert lib.vnd_polar_level_work_bytes(*bad, 0, ctypes.byref(got)) == INVALID and got.value == 0
    assert lib.vnd_polar_level_work_bytes(1, 10, 360, 2, 0, None) == INVALID
    for bad in ((65536, 10, 360, 2), (1, 2 ** 32, 360, 2), (1, 10, 1025, 2), (1, 10, 360, 5)):
        assert lib.vnd_polar_level_work_bytes(*bad, 0, ctypes.byref(got)) == UNSUPPORTED and got.value == 0

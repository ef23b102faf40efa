"""CPU tier of the vectorscope (include/vnd_scope.h, vndecorrelate_amd/vectorscope.py): the binning rule's NumPy mirror
against np.histogram2d cell for cell, the planted edge frames, np.degrees' float32 constant, the host route against the
oracle's polar_coordinates followed by np.histogram2d, and the header against its binding - no device call."""
import ctypes
import pathlib
import re
import subprocess

import numpy as np
import pytest

REPO = pathlib.Path(__file__).resolve().parents[1]
HEADER = REPO / 'include' / 'vnd_scope.h'
NAMES = ['vnd_lissajous_hist_f32_dev', 'vnd_lissajous_hist_f64_dev', 'vnd_polar_coords_f32_dev', 'vnd_polar_coords_f64_dev',
         'vnd_polar_hist_f32_dev', 'vnd_polar_hist_f64_dev', 'vnd_scope_route', 'vnd_scope_work_bytes']
INVALID, UNSUPPORTED = 1, 4


def _declared(header):
    text = re.sub(r'/\*.*?\*/', '', header.read_text(), flags=re.S)
    return sorted(set(re.findall(r'\b(vnd_[a-z0-9_]+)\s*\(', text)))


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


def _gauss(n, dtype, seed=0, scale=0.3):
    return (np.random.default_rng(seed).standard_normal((n, 2)) * scale).astype(dtype)


def _oracle_polar(sig, **kw):
    from oracle import vnd_oracle as O
    radii, thetas, _ = O.polar_coordinates(sig[:, 0], sig[:, 1], **kw)
    return radii, thetas


# ---- the binning rule ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_the_mirror_is_histogram2d_on_the_polar_grid(vs, dtype):
    sig = _gauss(48000, dtype)
    radii, thetas = _oracle_polar(sig)
    assert radii.dtype == dtype and thetas.dtype == dtype
    ae, re_ = vs.polar_edges(240, 150)
    want = np.histogram2d(np.degrees(thetas), radii, bins=[ae, re_])[0]
    got = vs.histogram_counts(np.degrees(thetas), radii, ae, re_)
    assert got.shape == (240, 150) and got.sum() == 48000
    assert np.array_equal(got, want)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_the_mirror_is_histogram2d_on_the_lissajous_grid(vs, dtype):
    sig = _gauss(48000, dtype, seed=1, scale=0.5)                 # a few frames leave [-1.1, 1.1]
    xe, ye = vs.lissajous_edges(512, ((-1.1, 1.1), (-1.1, 1.1)))
    want, wx, wy = np.histogram2d(sig[:, 0], sig[:, 1], bins=512, range=[[-1.1, 1.1], [-1.1, 1.1]])
    assert np.array_equal(xe, wx) and np.array_equal(ye, wy)      # the edges are np.histogram2d's own
    got = vs.histogram_counts(sig[:, 0], sig[:, 1], xe, ye)
    assert 0 < got.sum() < 48000
    assert np.array_equal(got, want)


def _planted_polar(dtype, n=4096, seed=3):
    """A random signal with the edge frames planted: [0] L = R > 0, [1] L = -R > 0, [2] -L = R > 0, [3] the max radius."""
    sig = _gauss(n, dtype, seed=seed, scale=0.2)
    sig[0] = (0.25, 0.25)
    sig[1] = (0.25, -0.25)
    sig[2] = (-0.25, 0.25)
    sig[3] = (3.0, 1.0)
    return sig


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_planted_polar_edge_frames(vs, dtype):
    sig = _planted_polar(dtype)
    radii, thetas = _oracle_polar(sig)
    deg = np.degrees(thetas)
    ae, re_ = vs.polar_edges()
    assert ae[120] == 0.0 and ae[-1] == 90.0 and ae[0] == -90.0 and re_[-1] == 1.0
    assert deg[0] == 0.0 and deg[1] == 90.0 and deg[2] == -90.0
    ka, kr = vs.histogram_bins(deg, ae), vs.histogram_bins(radii, re_)
    assert ka[0] == 120                                           # exactly edge 120: the bin that starts there
    assert ka[1] == 239                                           # exactly the last edge: the last bin
    assert ka[2] == 0
    if dtype == np.float32:                                       # max / (max + float32(1e-10)) is exactly 1
        assert radii[3] == 1.0 and kr[3] == 149
    assert np.array_equal(vs.histogram_counts(deg, radii, ae, re_), np.histogram2d(deg, radii, bins=[ae, re_])[0])


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_planted_lissajous_edge_frames(vs, dtype):
    sig = _gauss(1000, dtype, seed=4, scale=0.3)
    sig[0] = (-1.0, 0.0)
    sig[1] = (1.0, 0.0)
    sig[2] = (np.nextafter(dtype(1), dtype(2)), 0.0)
    sig[3] = (np.nan, 0.0)
    sig[4] = (np.inf, 0.0)
    sig[5] = (0.0, -np.inf)
    xe, ye = vs.lissajous_edges(16, ((-1, 1), (-1, 1)))
    kx = vs.histogram_bins(sig[:, 0], xe)
    assert list(kx[:5]) == [0, 15, -1, -1, -1] and vs.histogram_bins(sig[:, 1], ye)[5] == -1
    inside = sig[6:][np.all(np.abs(sig[6:]) <= 1, axis=1)]
    want = np.histogram2d(np.concatenate([sig[:2, 0], inside[:, 0]]), np.concatenate([sig[:2, 1], inside[:, 1]]),
                          bins=16, range=[[-1, 1], [-1, 1]])[0]
    got = vs.histogram_counts(sig[:, 0], sig[:, 1], xe, ye)
    assert np.array_equal(got, want) and got.sum() == 2 + len(inside)


def test_degrees_is_one_float32_multiply():
    th = np.random.default_rng(5).uniform(-np.pi, np.pi, 200000).astype(np.float32)
    k = np.float32(180) / np.float32(np.pi)
    assert k == np.float32(57.2957763671875) and k != np.float32(180 / np.pi)
    assert np.degrees(th).dtype == np.float32
    assert np.array_equal(np.degrees(th), th * k)
    assert not np.array_equal(np.degrees(th), th * np.float32(180 / np.pi))
    th64 = th.astype(np.float64) * 1.0000001
    assert np.array_equal(np.degrees(th64), th64 * (180.0 / np.pi))


# ---- the host route --------------------------------------------------------------------------------------------------
def _pool(dtype, n=6000):
    """B = 3 signals whose maxima are a factor of 10 apart."""
    return np.stack([_gauss(n, dtype, seed=10 + b, scale=0.02 * 10 ** b) for b in range(3)])


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_host_route_is_the_reference(vs, dtype):
    pool = _pool(dtype)
    radii, thetas = vs.polar_coordinates_batched(pool)
    grid, ae, re_ = vs.polar_histogram_batched(pool)
    liss, xe, ye = vs.lissajous_histogram_batched(pool, bins=64, range=((-0.5, 0.5), (-0.5, 0.5)))
    assert radii.dtype == dtype and radii.shape == (3, 6000) and grid.dtype == np.float64 and grid.shape == (3, 240, 150)
    for b in range(3):
        wr, wt = _oracle_polar(pool[b])
        assert np.array_equal(radii[b], wr) and np.array_equal(thetas[b], wt)
        assert np.array_equal(grid[b], np.histogram2d(np.degrees(wt), wr, bins=[ae, re_])[0])
        assert np.array_equal(liss[b], np.histogram2d(pool[b, :, 0], pool[b, :, 1], bins=64, range=[[-0.5, 0.5], [-0.5, 0.5]])[0])
        assert grid[b].sum() == 6000                              # its OWN maximum: a pool-wide one would empty the outer bins
        assert grid[b][:, 100:].sum() > 0
    # one signal, and the other options
    r1, t1 = vs.polar_coordinates_batched(pool[1], mode='LR', semicircular=False, normalize=False)
    wr, wt = _oracle_polar(pool[1], mode='LR', semicircular=False, normalize=False)
    assert r1.shape == (6000,) and np.array_equal(r1, wr) and np.array_equal(t1, wt)
    g1 = vs.polar_histogram_batched(pool[1])[0]
    assert g1.shape == (240, 150) and np.array_equal(g1, grid[1])


def test_host_route_max_points_counts_and_accumulate(vs):
    pool = _pool(np.float32, n=5003)
    rng = ((-0.5, 0.5), (-0.5, 0.5))
    got = vs.lissajous_histogram_batched(pool, bins=32, range=rng, max_points=700)[0]
    step = 5003 // 700
    for b in range(3):
        assert np.array_equal(got[b], np.histogram2d(pool[b, ::step, 0], pool[b, ::step, 1], bins=32, range=rng)[0])
    assert np.array_equal(vs.lissajous_histogram_batched(pool, bins=32, range=rng, max_points=5003)[0],
                          vs.lissajous_histogram_batched(pool, bins=32, range=rng)[0])
    # a fixed scale: two halves add up to the whole
    whole = vs.polar_histogram_batched(pool, radius_scale=1.5)[0]
    acc = np.zeros_like(whole)
    vs.polar_histogram_batched(pool[:, :2500], radius_scale=1.5, out=acc, accumulate=True)
    vs.polar_histogram_batched(pool[:, 2500:], radius_scale=1.5, out=acc, accumulate=True)
    assert np.array_equal(acc, whole)
    assert whole[:2].sum() == 2 * 5003 and 0 < whole[2].sum() < 5003      # the loud signal leaves the range: frames dropped
    for b in range(3):
        wr, wt = _oracle_polar(pool[b], normalize=False)
        ae, re_ = vs.polar_edges()
        assert np.array_equal(whole[b], np.histogram2d(np.degrees(wt), wr / np.float32(1.5), bins=[ae, re_])[0])
    with pytest.raises(ValueError, match='radius_scale'):
        vs.polar_histogram_batched(pool, out=acc, accumulate=True)
    with pytest.raises(ValueError, match='out='):
        vs.polar_histogram_batched(pool, radius_scale=1.5, accumulate=True)
    # counts: the first counts[b] frames; outside [0, n]: none
    each = vs.polar_histogram_batched(pool, radius_scale=1.5, counts=np.array([17, 5003, 5004], np.int32))[0]
    assert np.array_equal(each[0], vs.polar_histogram_batched(pool[0, :17], radius_scale=1.5)[0])
    assert np.array_equal(each[1], whole[1]) and each[2].sum() == 0
    with pytest.raises(ValueError, match='pool must be'):
        vs.polar_histogram_batched(np.zeros((4, 3), np.float32))
    with pytest.raises(ValueError, match='mode'):
        vs.polar_coordinates_batched(pool, mode='XY')


def test_routing_and_exports(vs):
    import vndecorrelate_amd
    from vndecorrelate_amd import analysis
    names = {'polar_coordinates_batched', 'polar_histogram_batched', 'lissajous_histogram_batched', 'set_scope_device',
             'scope_covers'}
    assert names <= set(analysis.__all__)
    for name in names:
        assert getattr(vndecorrelate_amd, name) is getattr(vs, name) is getattr(analysis, name)
    assert vs.scope_covers(np.float32, 3, 48000, 240, 150) and vs.scope_covers('float64', 1, 1, 512, 512)
    assert not vs.scope_covers(np.float16, 3, 48000) and not vs.scope_covers(np.int16, 3, 48000)
    assert not vs.scope_covers(np.float32, 0, 48000) and not vs.scope_covers(np.float32, 3, 0)
    assert not vs.scope_covers(np.float32, 3, 2 ** 32) and vs.scope_covers(np.float32, 1, 2 ** 32 - 1)
    assert not vs.scope_covers(np.float32, 65536, 10) and not vs.scope_covers(np.float32, 3, 10, 4097, 1)
    assert not vs.scope_covers(np.float32, 65535, 2 ** 20)
    with pytest.raises(TypeError):
        vs.set_scope_device(1)
    assert vs.use_device(np.float32, 3, 48000) is False            # the fixture's set_scope_device(False)


# ---- header and binding ----------------------------------------------------------------------------------------------
def test_header_is_plain_c():
    src = ('#include "vnd_scope.h"\n'
           'int main(void){return VND_SCOPE_MAX_BINS == 4096 && VND_SCOPE_ROUTE_LDS == 1 && VND_SCOPE_ROUTE_DIRECT == 2 ? 0 : 1;}\n')
    r = subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-pedantic', '-fsyntax-only', '-I', str(REPO / 'include'),
                        '-x', 'c', '-'], input=src.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()


def test_every_declared_symbol_is_exported_and_bound(lib):
    from vndecorrelate_amd import _native, vectorscope
    names = _declared(HEADER)
    assert names == NAMES
    for name in names:
        assert hasattr(lib, name), f'{name} declared in vnd_scope.h but not exported'
    assert not set(names) & set(_declared(REPO / 'include' / 'vnd_amd.h'))            # vnd_amd.h keeps its fixed set
    text = re.sub(r'/\*.*?\*/', '', HEADER.read_text(), flags=re.S)
    for define, value in (('VND_SCOPE_MAX_BINS', vectorscope.MAX_BINS), ('VND_SCOPE_SPAN_FRAMES', vectorscope.SPAN_FRAMES),
                          ('VND_SCOPE_DIRECT_SPAN_FRAMES', vectorscope.DIRECT_SPAN_FRAMES),
                          ('VND_SCOPE_LDS_BYTES', vectorscope.LDS_BYTES)):
        assert int(re.search(r'#define %s (\d+)' % define, text).group(1)) == value
    for wrapper in ('scope_work_bytes', 'scope_route', 'polar_coords_device', 'polar_hist_device', 'lissajous_hist_device'):
        assert callable(getattr(_native, wrapper))


P = 1 << 20            # a made-up device address: nothing below reaches a device


def _coords(lib, f64=False, *, ctx=0, l=P, r=P + 8, batch=3, n=100, ss=200, fs=2, ms=1, semi=1, norm=1, radii=2 * P,
            thetas=3 * P, work=4 * P, work_bytes=24):
    fn = lib.vnd_polar_coords_f64_dev if f64 else lib.vnd_polar_coords_f32_dev
    return fn(ctx, l, r, batch, n, ss, fs, ms, semi, norm, radii, thetas, work, work_bytes, None)


def _polar(lib, f64=False, *, ctx=0, l=P, r=P + 8, batch=3, n=100, ss=200, fs=2, ms=1, semi=1, scale=0.0, ae=5 * P, na=240,
           re_=6 * P, nr=150, each=0, counts=2 * P, acc=0, work=4 * P, work_bytes=24):
    fn = lib.vnd_polar_hist_f64_dev if f64 else lib.vnd_polar_hist_f32_dev
    return fn(ctx, l, r, batch, n, ss, fs, ms, semi, scale, ae, na, re_, nr, each, counts, acc, work, work_bytes, None)


def _liss(lib, f64=False, *, ctx=0, l=P, r=P + 8, batch=3, n=100, ss=200, fs=2, step=1, xe=5 * P, nx=512, ye=6 * P, ny=512,
          each=0, counts=2 * P, acc=0):
    fn = lib.vnd_lissajous_hist_f64_dev if f64 else lib.vnd_lissajous_hist_f32_dev
    return fn(ctx, l, r, batch, n, ss, fs, step, xe, nx, ye, ny, each, counts, acc, None)


@pytest.mark.parametrize('f64', [False, True])
def test_checks_that_need_no_device(lib, f64):
    err = lib.vnd_last_error
    # valid arguments reach the last check: the context
    for call in (_coords, _polar, _liss):
        assert call(lib, f64) == INVALID and b'null context' in err()
    assert _polar(lib, f64, scale=1.5, work=0, work_bytes=0, acc=1, each=7 * P) == INVALID and b'null context' in err()
    assert _coords(lib, f64, norm=0, work=0, work_bytes=0) == INVALID and b'null context' in err()
    # null pointers
    for call, names in ((_coords, ('l', 'r', 'radii', 'thetas', 'work')), (_polar, ('l', 'r', 'ae', 're_', 'counts', 'work')),
                        (_liss, ('l', 'r', 'xe', 'ye', 'counts'))):
        for name in names:
            assert call(lib, f64, **{name: 0}) == INVALID and b'null' in err() and b'context' not in err(), name
    # sizes below 1
    for call, names in ((_coords, ('batch', 'n', 'ss', 'fs')), (_polar, ('batch', 'n', 'ss', 'fs', 'na', 'nr')),
                        (_liss, ('batch', 'n', 'ss', 'fs', 'step', 'nx', 'ny'))):
        for name in names:
            for bad in (0, -1):
                assert call(lib, f64, **{name: bad}) == INVALID and b'>= 1' in err(), (name, bad)
    # work memory
    assert _coords(lib, f64, work_bytes=23) == INVALID and b'work of 23 bytes' in err()
    assert _polar(lib, f64, work=4 * P + 4) == INVALID and b'aligned' in err()
    # accumulate with the per-signal maximum; scales
    assert _polar(lib, f64, acc=1) == INVALID and b'accumulate' in err()
    assert _polar(lib, f64, acc=1, scale=-1.0) == INVALID and b'accumulate' in err()
    assert _polar(lib, f64, scale=float('nan')) == INVALID and b'NaN' in err()
    assert _polar(lib, f64, scale=float('inf')) == INVALID and b'radius_scale' in err()
    if not f64:
        assert _polar(lib, f64, scale=1e-60) == INVALID and b'radius_scale' in err()          # float32(1e-60) == 0
        assert _polar(lib, f64, scale=1e60) == INVALID and b'radius_scale' in err()           # float32(1e60) == inf
    # overlapping buffers: the frames span 3 * 200 samples from P
    size = 8 if f64 else 4
    inside = P + 100 * size
    for call, names in ((_coords, ('radii', 'thetas', 'work')), (_polar, ('counts', 'work')), (_liss, ('counts',))):
        for name in names:
            assert call(lib, f64, **{name: inside}) == INVALID and b'overlap' in err(), name
    assert _coords(lib, f64, thetas=2 * P + 8) == INVALID and b'one another' in err()
    assert _coords(lib, f64, work=3 * P + 16) == INVALID and b'one another' in err()
    assert _polar(lib, f64, counts=5 * P + 8) == INVALID and b'edges' in err()                # counts over the angle edges
    assert _polar(lib, f64, counts=6 * P - 16) == INVALID and b'overlap' in err()             # ... reaching the radius edges
    assert _polar(lib, f64, each=2 * P + 64) == INVALID and b'n_each' in err()
    assert _polar(lib, f64, work=2 * P + 8) == INVALID and b'one another' in err()
    assert _liss(lib, f64, counts=6 * P + 513 * 8 - 4) == INVALID and b'overlap' in err()
    assert _liss(lib, f64, counts=6 * P + 513 * 8) == INVALID and b'null context' in err()    # just past the edges: clean
    # what the launch does not take
    big = 2 ** 32
    assert _coords(lib, f64, n=big, ss=2 * big, radii=1 << 40, thetas=1 << 42, work=1 << 44) == UNSUPPORTED and b'uint32' in err()
    assert _polar(lib, f64, n=big, ss=2 * big, counts=1 << 40, work=1 << 44, ae=1 << 45, re_=1 << 46) == UNSUPPORTED \
        and b'uint32' in err()
    assert _liss(lib, f64, n=big, ss=2 * big, counts=1 << 40, xe=1 << 45, ye=1 << 46) == UNSUPPORTED and b'uint32' in err()
    assert _polar(lib, f64, n=big - 1, ss=2 * big, scale=1.0, counts=1 << 40, ae=1 << 45, re_=1 << 46) == INVALID \
        and b'null context' in err()                                                          # 2^32 - 1 frames are taken
    assert _polar(lib, f64, na=4097, counts=1 << 40) == UNSUPPORTED and b'bins' in err()
    assert _liss(lib, f64, ny=4097, counts=1 << 40) == UNSUPPORTED and b'bins' in err()
    assert _polar(lib, f64, batch=65536, ss=1, fs=1, n=1, work_bytes=8 * 65536, counts=1 << 40) == UNSUPPORTED
    assert _liss(lib, f64, batch=65535, n=2 ** 20, ss=1, fs=1, counts=1 << 40) == UNSUPPORTED and b'workgroups' in err()


def test_work_bytes_and_route(lib, monkeypatch):
    from vndecorrelate_amd import _native
    got = ctypes.c_int64(-7)
    assert lib.vnd_scope_work_bytes(3, ctypes.byref(got)) == 0 and got.value == 24
    assert _native.scope_work_bytes(256) == 2048
    assert lib.vnd_scope_work_bytes(0, ctypes.byref(got)) == INVALID and got.value == 0
    assert lib.vnd_scope_work_bytes(3, None) == INVALID
    assert lib.vnd_scope_work_bytes(65536, ctypes.byref(got)) == UNSUPPORTED
    monkeypatch.delenv('VND_SCOPE_ROUTE', raising=False)
    LDS, DIRECT = _native.SCOPE_ROUTE_LDS, _native.SCOPE_ROUTE_DIRECT
    assert _native.scope_route(240, 150, 480000) == LDS           # the grid the LDS-private route is sized for
    assert _native.scope_route(512, 512, 480000) == DIRECT        # 1 MiB: does not fit
    assert _native.scope_route(512, 150, 480000) == DIRECT
    assert _native.scope_route(240, 150, 480) == DIRECT           # too few frames for 36 000 cells of clearing and flushing
    assert _native.scope_route(4, 3, 100) == LDS
    monkeypatch.setenv('VND_SCOPE_ROUTE', '2')                    # read at the call (the test tier is a tuning session)
    assert _native.scope_route(240, 150, 480000) == DIRECT and _native.scope_route(4, 3, 100) == DIRECT
    monkeypatch.setenv('VND_SCOPE_ROUTE', '1')
    assert _native.scope_route(240, 150, 480) == LDS
    assert _native.scope_route(512, 512, 480000) == DIRECT        # pinned, but it does not fit
    route = ctypes.c_int32(9)
    assert lib.vnd_scope_route(0, 3, 1, ctypes.byref(route)) == INVALID and route.value == 0
    assert lib.vnd_scope_route(4097, 3, 1, ctypes.byref(route)) == UNSUPPORTED
    assert lib.vnd_scope_route(4, 3, 1, None) == INVALID

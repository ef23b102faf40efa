"""GPU tier of the vectorscope (include/vnd_scope.h).  The main contract has no tolerance: a count grid equals
np.histogram2d of the thetas and radii that vnd_polar_coords_*_dev writes for the same pool, cell for cell, on both routes -
which takes the last bits of atan2 out of the comparison and leaves the fold, the degrees constant, the per-signal maximum
and divide, the edge rule, the merging of partial grids and the batch indexing in it.  Every call here runs between guard
bands, with its inputs compared afterwards."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 512                      # elements of sentinel either side of every output
LDS, DIRECT = 1, 2
ROUTES = (LDS, DIRECT)


@pytest.fixture(scope='module')
def gpu():
    import torch
    import __graft_entry__ as entry
    entry.build()
    from vndecorrelate_amd import _native, vectorscope
    ctx = _native.default_context()

    class G:
        pass
    g = G()
    g.torch, g.native, g.vs, g.ctx = torch, _native, vectorscope, ctx
    g.device = torch.device('cuda', ctx.device)
    return g


@pytest.fixture
def route(monkeypatch):
    """Pin a route for the calls that follow (VND_SCOPE_ROUTE is read at the call in this tuning session)."""
    def pin(which):
        if which is None:
            monkeypatch.delenv('VND_SCOPE_ROUTE', raising=False)
        else:
            monkeypatch.setenv('VND_SCOPE_ROUTE', str(which))
    yield pin
    monkeypatch.delenv('VND_SCOPE_ROUTE', raising=False)


class Guarded:
    """A device buffer of `count` elements between two guard bands of a sentinel."""

    def __init__(self, g, count, dtype, fill):
        self.fill, self.count = fill, count
        self.whole = g.torch.full((count + 2 * GUARD,), fill, dtype=dtype, device=g.device)
        self.view = self.whole[GUARD:GUARD + count]

    def ptr(self):
        return self.view.data_ptr()

    def check(self):
        w = self.whole.cpu().numpy()
        assert (w[:GUARD] == self.fill).all() and (w[GUARD + self.count:] == self.fill).all(), 'a guard band was written'
        return w[GUARD:GUARD + self.count]


def _upload(g, a):
    return g.torch.from_numpy(np.ascontiguousarray(a)).to(g.device)


def _pool_ptrs(g, pool):
    d = _upload(g, pool)
    batch, n, _ = pool.shape
    return d, d.data_ptr(), d.data_ptr() + pool.itemsize, batch, n


def dev_coords(g, pool, *, mode='MS', semicircular=True, normalize=True, work_fill=0):
    tdt = g.torch.float32 if pool.dtype == np.float32 else g.torch.float64
    d, lp, rp, batch, n = _pool_ptrs(g, pool)
    radii, thetas = Guarded(g, batch * n, tdt, -777.0), Guarded(g, batch * n, tdt, -777.0)
    work = Guarded(g, batch, g.torch.int64, work_fill)
    g.native.polar_coords_device(g.ctx, lp, rp, batch, n, 2 * n, 2, radii.ptr(), thetas.ptr(), ms_mode=mode == 'MS',
                                 semicircular=semicircular, normalize=normalize, work_ptr=work.ptr() if normalize else 0,
                                 work_bytes=8 * batch if normalize else 0, float64=pool.dtype == np.float64,
                                 stream=g.torch.cuda.current_stream(g.device).cuda_stream)
    g.torch.cuda.synchronize()
    work.check()
    assert np.array_equal(d.cpu().numpy(), pool, equal_nan=True), 'the frames changed'
    return radii.check().reshape(batch, n), thetas.check().reshape(batch, n)


def dev_hist(g, pool, e0, e1, *, polar, mode='MS', semicircular=True, scale=None, step=1, n_each=None, start=None,
             accumulate=False, work_fill=0):
    """One histogram call between guard bands: uint32 (batch, bins0, bins1)."""
    d, lp, rp, batch, n = _pool_ptrs(g, pool)
    b0, b1 = len(e0) - 1, len(e1) - 1
    d0, d1 = _upload(g, e0), _upload(g, e1)
    counts = Guarded(g, batch * b0 * b1, g.torch.int32, 0x5a5a5a5a)
    if start is not None:
        counts.view.copy_(_upload(g, start.astype(np.uint32).view(np.int32).reshape(-1)))
    work = Guarded(g, batch, g.torch.int64, work_fill)
    each = None if n_each is None else _upload(g, np.asarray(n_each, np.int32))
    kw = dict(n_each_ptr=0 if each is None else each.data_ptr(), accumulate=accumulate, float64=pool.dtype == np.float64,
              stream=g.torch.cuda.current_stream(g.device).cuda_stream)
    if polar:
        by_max = scale is None
        g.native.polar_hist_device(g.ctx, lp, rp, batch, n, 2 * n, 2, d0.data_ptr(), b0, d1.data_ptr(), b1, counts.ptr(),
                                   ms_mode=mode == 'MS', semicircular=semicircular, radius_scale=0.0 if by_max else scale,
                                   work_ptr=work.ptr() if by_max else 0, work_bytes=8 * batch if by_max else 0, **kw)
    else:
        g.native.lissajous_hist_device(g.ctx, lp, rp, batch, n, 2 * n, 2, d0.data_ptr(), b0, d1.data_ptr(), b1, counts.ptr(),
                                       frame_step=step, **kw)
    g.torch.cuda.synchronize()
    work.check()
    assert np.array_equal(d.cpu().numpy(), pool, equal_nan=True), 'the frames changed'
    assert np.array_equal(d0.cpu().numpy(), e0) and np.array_equal(d1.cpu().numpy(), e1), 'the edges changed'
    if each is not None:
        assert np.array_equal(each.cpu().numpy(), np.asarray(n_each, np.int32))
    return counts.check().view(np.uint32).reshape(batch, b0, b1)


def make_pool(dtype, n, batch=3, seed=0, plant=True):
    """`batch` Gaussian signals with maxima a factor of 10 apart, the CPU tier's edge frames planted where they fit."""
    rng = np.random.default_rng(seed)
    pool = np.stack([rng.standard_normal((n, 2)) * (0.02 * 10 ** b) for b in range(batch)]).astype(dtype)
    if plant and n >= 8:
        for b in range(batch):
            s = dtype(0.25 * 10 ** b)
            pool[b, n // 2] = (s, s)             # theta = 0: exactly edge 120 of the default grid
            pool[b, 1] = (s, -s)                 # +90 degrees: the last edge
            pool[b, n - 1] = (-s, s)             # -90 degrees
            pool[b, 3] = (12 * s, 4 * s)         # the signal's largest radius: normalises to the last radius edge
    return pool


def grid_of(g, radii, thetas, e0, e1):
    return np.stack([np.histogram2d(np.degrees(thetas[b]), radii[b], bins=[e0, e1])[0] for b in range(len(radii))])


def numpy_polar(pool, **kw):
    from oracle import vnd_oracle as O
    out = [O.polar_coordinates(pool[b, :, 0], pool[b, :, 1], **kw) for b in range(len(pool))]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


GRIDS = [(4, 3), (240, 150), (512, 150)]


def _frame_counts(g):
    return [1, 255, 256, 257, 2 * g.vs.SPAN_FRAMES + 1]          # the last: three workgroups a signal on the LDS route


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('which', range(5))
def test_counts_are_the_grid_of_the_devices_own_coordinates(gpu, route, dtype, which):
    g = gpu
    n = _frame_counts(g)[which]
    pool = make_pool(dtype, n, seed=which)
    radii, thetas = dev_coords(g, pool)
    assert radii.dtype == dtype and thetas.dtype == dtype
    want_radii, _ = numpy_polar(pool)
    assert np.array_equal(radii.view(np.uint8), want_radii.view(np.uint8)), 'radii differ from NumPy bit for bit'
    if n >= 8:
        deg = np.degrees(thetas)
        assert (deg[:, n // 2] == 0).all() and (deg[:, 1] == 90).all() and (deg[:, n - 1] == -90).all()
        if dtype == np.float32:
            assert (radii[:, 3] == 1).all()
    for bins in GRIDS:
        e0, e1 = g.vs.polar_edges(*bins)
        want = grid_of(g, radii, thetas, e0, e1)
        assert want.sum() == 3 * n
        got = {}
        for r in ROUTES:
            route(r)
            if bins == (512, 150):
                assert g.native.scope_route(*bins, n) == DIRECT    # does not fit LDS, whatever is pinned
            else:
                assert g.native.scope_route(*bins, n) == r
            got[r] = dev_hist(g, pool, e0, e1, polar=True)
            assert np.array_equal(got[r], want), (bins, r, int(np.abs(got[r].astype(np.int64) - want).sum()))
        assert np.array_equal(got[LDS], got[DIRECT])
        if n >= 8 and bins == (240, 150):
            for b in range(3):
                assert got[LDS][b, 120].sum() >= 1 and got[LDS][b, 239].sum() >= 1 and got[LDS][b, 0].sum() >= 1
                assert got[LDS][b, :, 149].sum() >= 1


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('options', [dict(mode='LR'), dict(semicircular=False)])
def test_the_other_layout_and_the_whole_circle(gpu, route, dtype, options):
    g = gpu
    pool = make_pool(dtype, 1000, seed=7)
    radii, thetas = dev_coords(g, pool, **options)
    want_radii, want_thetas = numpy_polar(pool, **options)
    assert np.array_equal(radii, want_radii)
    assert np.abs(thetas.astype(np.float64) - want_thetas).max() <= (1e-6 if dtype == np.float32 else 4e-15)
    if 'semicircular' in options:
        assert np.abs(thetas).max() > 2.0                          # nothing folded
    e0, e1 = g.vs.polar_edges(240, 150)
    if 'semicircular' in options:
        e0 = np.linspace(-180.0, 180.0, 241)
    want = grid_of(g, radii, thetas, e0, e1)
    for r in ROUTES:
        route(r)
        assert np.array_equal(dev_hist(g, pool, e0, e1, polar=True, **options), want)


def test_raw_coordinates_and_a_fixed_scale(gpu, route):
    """normalize=False writes the radius itself; a fixed scale divides by float32(scale) and needs no work memory."""
    g = gpu
    pool = make_pool(np.float32, 3000, seed=8)
    radii, thetas = dev_coords(g, pool, normalize=False)
    want_radii, _ = numpy_polar(pool, normalize=False)
    assert np.array_equal(radii, want_radii)
    e0, e1 = g.vs.polar_edges()
    scaled = radii / np.float32(1.5)
    want = grid_of(g, scaled, thetas, e0, e1)
    assert 0 < want[2].sum() < 3000                                # the loud signal leaves [0, 1]: frames dropped
    for r in ROUTES:
        route(r)
        assert np.array_equal(dev_hist(g, pool, e0, e1, polar=True, scale=1.5), want)


def test_contention_and_repeatability(gpu, route):
    g = gpu
    n = 100000
    pool = np.full((1, n, 2), 0.25, np.float32)
    e0, e1 = g.vs.polar_edges()
    for r in ROUTES:
        route(r)
        got = dev_hist(g, pool, e0, e1, polar=True)
        assert got[0, 120, 149] == n and got.sum() == n            # theta = 0 and radius max / (max + eps) = 1: one cell
        again = dev_hist(g, pool, e0, e1, polar=True)
        assert got.tobytes() == again.tobytes()


def test_the_work_memory_may_hold_anything(gpu, route):
    g = gpu
    pool = make_pool(np.float32, 5000, seed=9)
    e0, e1 = g.vs.polar_edges()
    for r in ROUTES:
        route(r)
        a = dev_hist(g, pool, e0, e1, polar=True, work_fill=0x0123456789abcdef)
        b = dev_hist(g, pool, e0, e1, polar=True, work_fill=-1)
        assert np.array_equal(a, b) and a.sum() == 3 * 5000
    ra, ta = dev_coords(g, pool, work_fill=0x7fffffff7fffffff)
    rb, tb = dev_coords(g, pool, work_fill=-1)
    assert np.array_equal(ra, rb) and np.array_equal(ta, tb)


def _ulps32(got, ref64):
    spacing = np.spacing(np.abs(ref64).astype(np.float32)).astype(np.float64)
    return float(np.max(np.abs(got.astype(np.float64) - ref64) / spacing))


def test_thetas_stay_within_libm_distance(gpu):
    """A sanity bound beside the exact contract: the device's atan2f may sit as far from the float64 angle as twice what
    NumPy's float32 arctan2 does on this input (both are few-ulp libm implementations)."""
    g = gpu
    pool = make_pool(np.float32, 48000, batch=1, seed=11, plant=False)
    left, right = pool[0, :, 0], pool[0, :, 1]
    # the float32 arguments l - r and l + r are rounded before atan2 sees them: compare on those
    ref = np.arctan2((left - right).astype(np.float64), (left + right).astype(np.float64))
    numpy_ulps = _ulps32(np.arctan2(left - right, left + right), ref)
    _, thetas = dev_coords(g, pool, semicircular=False, normalize=False)
    device_ulps = _ulps32(thetas[0], ref)
    print(f'float32 atan2 against float64, in float32 ulps: NumPy {numpy_ulps:.3f}, device {device_ulps:.3f}')
    assert numpy_ulps >= 0.5
    assert device_ulps <= 2 * numpy_ulps
    pool64 = pool.astype(np.float64)
    _, thetas64 = dev_coords(g, pool64, semicircular=False, normalize=False)
    worst = float(np.abs(thetas64[0] - np.arctan2(pool64[0, :, 0] - pool64[0, :, 1], pool64[0, :, 0] + pool64[0, :, 1])).max())
    print(f'float64 atan2 against NumPy: {worst:.3e}')
    assert worst <= 4e-15                                          # THETA_ABS of tests/test_gpu_haas_scan.py


def test_against_the_references_own_thetas(gpu, route):
    g = gpu
    n = 48000
    pool = (np.random.default_rng(12).standard_normal((1, n, 2)) * 0.3).astype(np.float32)
    radii, thetas = numpy_polar(pool)
    e0, e1 = g.vs.polar_edges()
    ref = np.histogram2d(np.degrees(thetas[0]), radii[0], bins=[e0, e1])[0]
    ka, kr = g.vs.histogram_bins(np.degrees(thetas[0]), e0), g.vs.histogram_bins(radii[0], e1)
    step = 8 * np.spacing(np.abs(thetas[0]))
    up, down = g.vs.histogram_bins(np.degrees(thetas[0] + step), e0), g.vs.histogram_bins(np.degrees(thetas[0] - step), e0)
    ambiguous = np.flatnonzero((up != ka) | (down != ka))
    print(f'{len(ambiguous)} of {n} frames are ambiguous at 8 ulps')
    assert len(ambiguous) * 10000 <= n                             # the condition on the input
    for r in ROUTES:
        route(r)
        got = dev_hist(g, pool, e0, e1, polar=True)[0].astype(np.int64)
        diff = got - ref.astype(np.int64)
        print(f'route {r}: sum |device - reference| = {int(np.abs(diff).sum())}')
        assert np.abs(diff).sum() <= 2 * len(ambiguous)
        for a, rad in zip(*np.nonzero(diff)):
            assert any(kr[f] == rad and abs(ka[f] - a) <= 1 for f in ambiguous), (a, rad)


def _lissajous_pool(dtype, n, seed):
    pool = make_pool(dtype, n, seed=seed, plant=False)
    pool[:, 0] = (-1.0, 0.5)
    pool[:, 7] = (1.0, -1.0)
    pool[:, 14] = (np.nextafter(dtype(1), dtype(2)), 0.0)
    pool[:, 21] = (np.nan, 0.0)
    pool[:, 28] = (0.0, np.inf)
    pool[:, 35] = (-np.inf, np.nan)
    return pool


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('step', [1, 7])
def test_lissajous_is_histogram2d(gpu, route, dtype, step):
    g = gpu
    n = 1003                                                       # not a multiple of 7; frames 0, 7, ..., 35 are planted
    pool = _lissajous_pool(dtype, n, seed=13)
    for bins, rng, routes in ((16, ((-1, 1), (-1, 1)), ROUTES), (512, ((-1.1, 1.1), (-1.1, 1.1)), (None, LDS))):
        e0, e1 = g.vs.lissajous_edges(bins, rng)
        want = np.stack([np.histogram2d(pool[b, ::step, 0], pool[b, ::step, 1], bins=bins, range=rng)[0] for b in range(3)])
        assert want[0].sum() > 0
        if bins == 16:                                             # -1.0 and +1.0 are kept: the first bin, and the last
            assert (want[:, 0].sum(axis=1) >= 1).all() and (want[:, 15, 0] >= 1).all()
        for r in routes:
            route(r)
            assert g.native.scope_route(bins, bins, -(-n // step)) == (DIRECT if bins == 512 else r)
            assert np.array_equal(dev_hist(g, pool, e0, e1, polar=False, step=step), want), (bins, r)
    # one signal that spans three workgroups of the LDS route, decimated
    n = 7 * 2 * g.vs.SPAN_FRAMES + 5
    big = _lissajous_pool(dtype, n, seed=14)[:1]
    e0, e1 = g.vs.lissajous_edges(16, ((-1, 1), (-1, 1)))
    want = np.histogram2d(big[0, ::7, 0], big[0, ::7, 1], bins=16, range=((-1, 1), (-1, 1)))[0][None]
    for r in ROUTES:
        route(r)
        assert np.array_equal(dev_hist(g, big, e0, e1, polar=False, step=7), want)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_blocks_accumulate_to_the_one_shot_grid(gpu, route, dtype):
    g = gpu
    n = 9000
    pool = make_pool(dtype, n, seed=15)
    e0, e1 = g.vs.polar_edges()
    x0, x1 = g.vs.lissajous_edges(64, ((-0.5, 0.5), (-0.5, 0.5)))
    cuts = np.cumsum([0, 1, 255, 4800, n - 5056])
    for r in ROUTES + (None,):
        route(r)
        whole = dev_hist(g, pool, e0, e1, polar=True, scale=1.5)
        grid = np.zeros_like(whole)
        lwhole = dev_hist(g, pool, x0, x1, polar=False)
        lgrid = np.zeros_like(lwhole)
        for a, b in zip(cuts[:-1], cuts[1:]):
            block = np.ascontiguousarray(pool[:, a:b])
            grid = dev_hist(g, block, e0, e1, polar=True, scale=1.5, start=grid, accumulate=True)
            lgrid = dev_hist(g, block, x0, x1, polar=False, start=lgrid, accumulate=True)
        assert np.array_equal(grid, whole) and n < whole.sum() < 3 * n          # (loud frames leave [0, 1] and are dropped)
        assert np.array_equal(lgrid, lwhole)
    with pytest.raises(ValueError, match='accumulate'):
        dev_hist(g, pool, e0, e1, polar=True, start=whole, accumulate=True)


def test_n_each_is_read_on_the_device(gpu, route):
    g = gpu
    n = 300
    pool = make_pool(np.float32, n, batch=5, seed=16)
    each = [0, 17, n, n + 1, -1]
    e0, e1 = g.vs.polar_edges()
    x0, x1 = g.vs.lissajous_edges(16, ((-1, 1), (-1, 1)))
    for r in ROUTES:
        route(r)
        got = dev_hist(g, pool, e0, e1, polar=True, n_each=each)
        lgot = dev_hist(g, pool, x0, x1, polar=False, n_each=each, step=3)
        for b, m in enumerate([0, 17, n, 0, 0]):
            if m == 0:
                assert got[b].sum() == 0 and lgot[b].sum() == 0
                continue
            head = np.ascontiguousarray(pool[b:b + 1, :m])
            assert np.array_equal(got[b], dev_hist(g, head, e0, e1, polar=True)[0])       # its own maximum over m frames
            assert np.array_equal(lgot[b], dev_hist(g, head, x0, x1, polar=False, step=3)[0])
            assert got[b].sum() == m


def test_python_layer_and_graph_capture(gpu, route):
    g = gpu
    torch, vs = g.torch, g.vs
    route(None)
    pool = make_pool(np.float32, 20000, seed=17)
    e0, e1 = vs.polar_edges()
    want = dev_hist(g, pool, e0, e1, polar=True)
    vs.set_scope_device(True)
    try:
        host_grid, ae, re_ = vs.polar_histogram_batched(pool)                              # NumPy in, NumPy out
        assert isinstance(host_grid, np.ndarray) and host_grid.dtype == np.float64 and np.array_equal(host_grid, want)
        assert np.array_equal(ae, e0) and np.array_equal(re_, e1)
        t = _upload(g, pool)
        grid, tae, tre = vs.polar_histogram_batched(t)                                     # tensor in, tensors out
        assert grid.device == t.device and grid.dtype == torch.int32 and tae.dtype == torch.float64
        assert np.array_equal(grid.cpu().numpy().view(np.uint32), want) and np.array_equal(tae.cpu().numpy(), e0)
        radii, thetas = vs.polar_coordinates_batched(t)
        wr, wt = dev_coords(g, pool)
        assert np.array_equal(radii.cpu().numpy(), wr) and np.array_equal(thetas.cpu().numpy(), wt)
        one = vs.polar_histogram_batched(t[1])[0]
        assert tuple(one.shape) == (240, 150) and np.array_equal(one.cpu().numpy().view(np.uint32), want[1])
        lwant = np.stack([np.histogram2d(pool[b, ::6, 0], pool[b, ::6, 1], bins=512, range=((-1.1, 1.1), (-1.1, 1.1)))[0]
                          for b in range(3)])
        lgrid = vs.lissajous_histogram_batched(t, max_points=3000)[0]                      # 20000 // 3000 = 6
        assert np.array_equal(lgrid.cpu().numpy().view(np.uint32), lwant)
        each = _upload(g, np.array([5, 20000, 77], np.int32))
        acc = torch.zeros((3, 240, 150), dtype=torch.int32, device=g.device)
        for lo, hi in ((0, 12000), (12000, 20000)):
            vs.polar_histogram_batched(t[:, lo:hi], radius_scale=1.5, out=acc, accumulate=True)
        assert np.array_equal(acc.cpu().numpy().view(np.uint32), dev_hist(g, pool, e0, e1, polar=True, scale=1.5))
        part = vs.polar_histogram_batched(t, counts=each)[0].cpu().numpy()
        assert [int(part[b].sum()) for b in range(3)] == [5, 20000, 77]
        # "zero, then bin" captured once and replayed
        out = torch.full((3, 240, 150), 7, dtype=torch.int32, device=g.device)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            vs.polar_histogram_batched(t, out=out)
        for _ in range(2):
            out.fill_(9)
            graph.replay()
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy().view(np.uint32), want)
    finally:
        vs.set_scope_device(None)

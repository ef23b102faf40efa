"""GPU tier of the polar level envelope (include/vnd_level.h).  The main contract has no tolerance: levels and bin_counts
equal the reference's mask and np.percentile applied to the thetas and radii that vnd_polar_coords_*_dev writes for the same
pool, byte for byte - which takes the last bits of atan2 out of the comparison and leaves the mask rule, the staging, the
radix select, the merging of partial histograms, the rank rule and the lerp in it.  Every call here runs between guard
bands, over work memory pre-filled with garbage, with its inputs compared afterwards."""
import ctypes
import json
import pathlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 512                      # elements of sentinel either side of every output
GOLDEN = pathlib.Path(__file__).resolve().parent / 'golden'
INVALID, UNSUPPORTED = 1, 4
GARBAGE = (-1, 0x0123456789abcdef)


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
    g.span = vectorscope.LEVEL_SPAN_FRAMES
    return g


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

    def untouched(self):
        return bool((self.whole == self.fill).all())


def _upload(g, a):
    return g.torch.from_numpy(np.ascontiguousarray(a)).to(g.device)


def dev_coords(g, pool, *, mode='MS', semicircular=True, normalize=True):
    tdt = g.torch.float32 if pool.dtype == np.float32 else g.torch.float64
    d = _upload(g, pool)
    batch, n, _ = pool.shape
    radii, thetas = Guarded(g, batch * n, tdt, -777.0), Guarded(g, batch * n, tdt, -777.0)
    work = Guarded(g, batch, g.torch.int64, -1)
    g.native.polar_coords_device(g.ctx, d.data_ptr(), d.data_ptr() + pool.itemsize, batch, n, 2 * n, 2, radii.ptr(), thetas.ptr(),
                                 ms_mode=mode == 'MS', semicircular=semicircular, normalize=normalize,
                                 work_ptr=work.ptr() if normalize else 0, work_bytes=8 * batch if normalize else 0,
                                 float64=pool.dtype == np.float64, stream=g.torch.cuda.current_stream(g.device).cuda_stream)
    g.torch.cuda.synchronize()
    return radii.check().reshape(batch, n), thetas.check().reshape(batch, n)


def dev_level(g, pool, bins=360, ps=(95.0, 50.0), *, mode='MS', semicircular=True, scale=None, n_each=None, garbage=-1):
    """One level call between guard bands: (levels (batch, P, bins) of the pool's dtype, uint32 counts (batch, bins))."""
    f64 = pool.dtype == np.float64
    tdt = g.torch.float64 if f64 else g.torch.float32
    d = _upload(g, pool)
    batch, n, _ = pool.shape
    edges = np.linspace(-90.0, 90.0, bins + 1)
    de = _upload(g, edges)
    levels = Guarded(g, batch * len(ps) * bins, tdt, -777.0)
    counts = Guarded(g, batch * bins, g.torch.int32, 0x5a5a5a5a)
    need = g.native.polar_level_work_bytes(batch, n, bins, len(ps), f64)
    assert need % 8 == 0
    work = Guarded(g, need // 8, g.torch.int64, garbage)
    each = None if n_each is None else _upload(g, np.asarray(n_each, np.int32))
    g.native.polar_level_device(g.ctx, d.data_ptr(), d.data_ptr() + pool.itemsize, batch, n, 2 * n, 2, de.data_ptr(), bins,
                                list(ps), levels.ptr(), counts.ptr(), work_ptr=work.ptr(), work_bytes=need,
                                ms_mode=mode == 'MS', semicircular=semicircular, radius_scale=0.0 if scale is None else scale,
                                n_each_ptr=0 if each is None else each.data_ptr(), float64=f64,
                                stream=g.torch.cuda.current_stream(g.device).cuda_stream)
    g.torch.cuda.synchronize()
    work.check()
    assert np.array_equal(d.cpu().numpy(), pool, equal_nan=True), 'the frames changed'
    assert np.array_equal(de.cpu().numpy(), edges), 'the edges changed'
    if each is not None:
        assert np.array_equal(each.cpu().numpy(), np.asarray(n_each, np.int32))
    return levels.check().reshape(batch, len(ps), bins), counts.check().view(np.uint32).reshape(batch, bins)


def mask_levels(radii, thetas, bins, ps):
    """The reference's rule on one signal's coordinates: its mask per slice, np.percentile inside."""
    edges = np.linspace(-90.0, 90.0, bins + 1)
    degrees = np.degrees(thetas)
    levels, counts = np.zeros((len(ps), bins), radii.dtype), np.zeros(bins, np.uint32)
    for k in range(bins):
        mask = (degrees >= edges[k]) & (degrees < edges[k + 1])
        counts[k] = np.count_nonzero(mask)
        if counts[k]:
            inside = radii[mask]
            for i, p in enumerate(ps):
                levels[i, k] = np.percentile(inside, float(p))
    return levels, counts


def want_level(g, pool, bins=360, ps=(95.0, 50.0), *, mode='MS', semicircular=True, scale=None, n_each=None):
    batch, n, _ = pool.shape
    levels, counts = np.zeros((batch, len(ps), bins), pool.dtype), np.zeros((batch, bins), np.uint32)
    kw = dict(mode=mode, semicircular=semicircular, normalize=scale is None)
    whole = dev_coords(g, pool, **kw) if n_each is None else None
    for b in range(batch):
        if whole is not None:
            radii, thetas = whole[0][b], whole[1][b]
        else:
            m = int(n_each[b]) if 0 <= n_each[b] <= n else 0
            if m == 0:
                continue
            radii, thetas = (v[0] for v in dev_coords(g, np.ascontiguousarray(pool[b:b + 1, :m]), **kw))   # its own maximum
        if scale is not None:
            radii = radii / pool.dtype.type(scale)
        levels[b], counts[b] = mask_levels(radii, thetas, bins, ps)
    return levels, counts


def same(got, want):
    (gl, gc), (wl, wc) = got, want
    assert gl.dtype == wl.dtype and gc.dtype == wc.dtype == np.uint32
    assert np.array_equal(gc, wc), f'bin_counts differ in {int((gc != wc).sum())} slices'
    bits = np.uint32 if gl.itemsize == 4 else np.uint64
    bad = np.flatnonzero(np.ascontiguousarray(gl).view(bits).reshape(-1) != np.ascontiguousarray(wl).view(bits).reshape(-1))
    assert len(bad) == 0, f'levels differ in {len(bad)} places, first at {np.unravel_index(bad[0], gl.shape)}: ' \
                          f'{gl.reshape(-1)[bad[0]]!r} for {wl.reshape(-1)[bad[0]]!r}'


def make_pool(dtype, n, batch=3, seed=0, plant=True):
    """`batch` Gaussian signals with maxima a factor of 10 apart; mono and anti-phase frames of both signs where they fit."""
    rng = np.random.default_rng(seed)
    pool = np.stack([rng.standard_normal((n, 2)) * (0.02 * 10 ** b) for b in range(batch)]).astype(dtype)
    if plant and n >= 8:
        for b in range(batch):
            s = dtype(0.25 * 10 ** b)
            pool[b, n // 2] = (s, s)             # theta = 0: exactly the edge between slices 179 and 180, in 180
            pool[b, 5] = (-s, -s)                # theta = pi - pi = 0
            pool[b, 1] = (s, -s)                 # +90 degrees: the last edge, in no slice
            pool[b, 6] = (s / 2, -s / 2)
            pool[b, n - 1] = (-s, s)             # -90 degrees: slice 0
            pool[b, 3] = (12 * s, 4 * s)         # the signal's largest radius
    return pool


def _frame_counts(g):
    return [1, 2, 1000, g.span - 1, g.span, g.span + 1, 3 * g.span + 17]


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('which', range(7))
def test_levels_are_np_percentile_of_the_devices_own_coordinates(gpu, dtype, which):
    g = gpu
    n = _frame_counts(g)[which]
    pool = make_pool(dtype, n, seed=which)
    want = want_level(g, pool)
    got = dev_level(g, pool, garbage=GARBAGE[which % 2])
    same(got, want)
    planted = 2 if n >= 8 else 0
    assert (got[1].sum(axis=1) == n - planted).all()               # the two frames at +90.0 are in no slice
    if n >= 8:
        assert (got[1][:, 0] >= 1).all() and (got[1][:, 180] >= 2).all()
    if n == 1000:                                                  # sparse: slices with no, one and two frames
        for c in (0, 1, 2):
            assert (got[1] == c).any(), c
        assert (got[0].transpose(0, 2, 1)[got[1] == 0] == 0).all()
    again = dev_level(g, pool, garbage=GARBAGE[(which + 1) % 2])   # another run, other garbage: identical bytes
    assert again[0].tobytes() == got[0].tobytes() and again[1].tobytes() == got[1].tobytes()


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('n', [359, 360, 719, 720, 1439, 1440, 2879, 2880])
def test_either_side_of_every_digit_width(gpu, dtype, n):
    """A short signal selects with narrower digits (8 n >= 720 x 2^d at 360 slices and two percentiles: d = 1 ... 5 from 360,
    720, 1440 and 2880 frames on), so with more passes: the same levels either side of each step."""
    g = gpu
    pool = make_pool(dtype, n, seed=n)
    same(dev_level(g, pool), want_level(g, pool))


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('bins', [1, 360, 1024])
@pytest.mark.parametrize('ps', [(50.0,), (0.0, 50.0, 99.9, 100.0), (95.0, 95.0, 12.5)])
def test_bin_counts_and_percentile_lists(gpu, dtype, bins, ps):
    g = gpu
    assert bins <= g.vs.LEVEL_MAX_BINS and len(ps) <= g.vs.LEVEL_MAX_PERCENTILES
    pool = make_pool(dtype, 5000, seed=20 + bins)
    same(dev_level(g, pool, bins, ps), want_level(g, pool, bins, ps))


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('options', [dict(scale=1.5), dict(mode='LR'), dict(semicircular=False),
                                     dict(mode='LR', semicircular=False, scale=0.7)])
def test_fixed_scale_the_other_layout_and_the_whole_circle(gpu, dtype, options):
    g = gpu
    pool = make_pool(dtype, 3000, seed=30)
    want = want_level(g, pool, **options)
    got = dev_level(g, pool, **options)
    same(got, want)
    if not options.get('semicircular', True):
        assert (got[1].sum(axis=1) < 3000 - 2).all()               # nothing folded: frames outside [-90, 90) are dropped
    if 'scale' in options and 'mode' not in options:
        assert got[0][2].max() > 1.0                               # the loud signal is not normalised by its own maximum


def _crafted(dtype):
    """Radius lists, one signal each: LR frames (0, v) have theta 0 and radius v exactly."""
    t = dtype
    chain = [t(0.3)]
    for _ in range(49):
        chain.append(np.nextafter(chain[-1], t(1)))
    rng = np.random.default_rng(40)
    return {
        'one frame': [0.5],
        'two frames': [0.25, 0.75],
        'neighbours in the lowest bit': list(rng.permutation(chain)),
        'two neighbours': [chain[0], chain[1]] * 3,
        'top digit apart': [1e-15] * 5 + [1e15] * 5,
        'top digit apart, odd': [1e15] * 4 + [1e-15] * 3,
        'duplicates straddle': [1.0, 2.0, 2.0, 3.0],
        'duplicates below': [1.0, 1.0, 2.0, 3.0],
        'duplicates above': [1.0, 2.0, 3.0, 3.0],
        'all equal': [0.125] * 7,
        'zeros and one': [0.0] * 9 + [1.0],
        'no frame': [],
    }


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_crafted_radii(gpu, dtype):
    """Keys that differ only in their lowest bit, only in their top digit, duplicates that straddle prev / next, bins of one
    and two frames, in one batch by n_each; fixed scale 1, LR, four slices: every frame in slice 2."""
    g = gpu
    cases = _crafted(dtype)
    n = max(len(v) for v in cases.values())
    pool = np.full((len(cases), n, 2), 0.5, dtype)
    each = []
    for b, values in enumerate(cases.values()):
        pool[b, :len(values), 0] = 0
        pool[b, :len(values), 1] = values
        each.append(len(values))
    ps = (0.0, 50.0, 95.0, 100.0)
    opts = dict(mode='LR', scale=1.0, n_each=each)
    got = dev_level(g, pool, 4, ps, **opts)
    same(got, want_level(g, pool, 4, ps, **opts))
    for b, (name, values) in enumerate(cases.items()):
        assert got[1][b].tolist() == [0, 0, len(values), 0], name
        if values:                                                 # and against NumPy on NumPy's own radii
            v = np.array(values, dtype)
            radii = np.sqrt(v * v)
            want = [np.percentile(radii, p) for p in ps]
            assert got[0][b, :, 2].tobytes() == np.array(want, dtype).tobytes(), name
            if 'lowest bit' in name:
                keys = np.unique(radii.view(np.uint32 if dtype == np.float32 else np.uint64))
                assert len(keys) >= 25 and (np.diff(keys.astype(np.int64)) == 1).any()


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_one_slice_signals_longer_than_a_span(gpu, dtype):
    """A mono signal with all radii distinct (one slice, one digit path), all-equal frames (every pass degenerate, sorted[next]
    == sorted[prev]) and digital silence (maximum 0, every radius 0): whole waves count into one counter."""
    g = gpu
    n = g.span + 1000
    pool = np.zeros((3, n, 2), dtype)
    ramp = (np.random.default_rng(41).permutation(n) + 1).astype(dtype) / dtype(n)
    pool[0, :, 0] = pool[0, :, 1] = ramp
    pool[1] = 0.25
    ps = (0.0, 50.0, 95.0, 100.0)
    got = dev_level(g, pool, 360, ps)
    same(got, want_level(g, pool, 360, ps))
    assert (got[1][:, 180] == n).all() and got[1].sum() == 3 * n
    assert len(np.unique(got[0][0, :, 180])) == 4 and len(np.unique(got[0][1, :, 180])) == 1 and not got[0][2].any()


def test_n_each_is_read_on_the_device(gpu):
    g = gpu
    n = 300
    pool = make_pool(np.float32, n, batch=5, seed=42)
    each = [0, 17, n, n + 1, -1]
    got = dev_level(g, pool, n_each=each)
    same(got, want_level(g, pool, n_each=each))
    assert [int(c.sum()) for c in got[1]] == [0, 17 - 2, n - 2, 0, 0]
    for b in (0, 3, 4):
        assert not got[0][b].any()
    mid = dev_level(g, np.ascontiguousarray(pool[1:2, :17]))
    assert mid[0].tobytes() == got[0][1:2].tobytes()


@pytest.mark.parametrize('name', ['f32', 'f64'])
def test_the_fixture_of_the_reference(gpu, name):
    """The reference's own _build_pseudo_hull output, exact because no frame of the fixture lies near a slice edge."""
    g = gpu
    arrays = np.load(GOLDEN / 'polar_level.npz')
    manifest = json.loads((GOLDEN / 'polar_level_manifest.json').read_text())
    frames, want = arrays[f'{name}__frames'], arrays[f'{name}__levels']
    levels, counts = dev_level(g, frames[None], manifest['num_bins'], manifest['percentiles'])
    assert levels[0].astype(np.float64).tobytes() == want.tobytes()
    assert counts.sum() == len(frames) - 2 and (counts == 0).sum() == 20 and counts[0, 180] >= 3
    g.vs.set_scope_device(True)
    try:
        host = g.vs.polar_level_batched(frames, manifest['num_bins'], manifest['percentiles'])    # NumPy in, NumPy out
        assert host[0].dtype == np.float64 and host[0].tobytes() == want.tobytes()
        assert host[1].dtype == np.int64 and np.array_equal(host[1], counts[0])
    finally:
        g.vs.set_scope_device(None)


def test_python_layer_and_graph_capture(gpu):
    g = gpu
    torch, vs = g.torch, g.vs
    pool = make_pool(np.float32, 20000, seed=43)
    want = dev_level(g, pool)
    vs.set_scope_device(True)
    try:
        t = _upload(g, pool)
        levels, counts, edges, centers = vs.polar_level_batched(t)                           # tensor in, tensors out
        assert levels.device == t.device and levels.dtype == torch.float32 and tuple(levels.shape) == (3, 2, 360)
        assert counts.device == t.device and counts.dtype == torch.int32 and edges.dtype == centers.dtype == torch.float64
        same((levels.cpu().numpy(), counts.cpu().numpy().view(np.uint32)), want)
        e = np.linspace(-90.0, 90.0, 361)
        assert np.array_equal(edges.cpu().numpy(), e) and np.array_equal(centers.cpu().numpy(), 0.5 * (e[:-1] + e[1:]))
        one = vs.polar_level_batched(t[1])
        assert tuple(one[0].shape) == (2, 360) and one[0].cpu().numpy().tobytes() == want[0][1].tobytes()
        t64 = _upload(g, pool.astype(np.float64))
        l64 = vs.polar_level_batched(t64, 90, (50.0,), radius_scale=2.0, mode='LR')[0]
        assert l64.dtype == torch.float64
        assert l64.cpu().numpy().tobytes() == dev_level(g, pool.astype(np.float64), 90, (50.0,), scale=2.0, mode='LR')[0].tobytes()
        each = _upload(g, np.array([5000, 20000, 77], np.int32))
        part = vs.polar_level_batched(t, counts=each)
        same((part[0].cpu().numpy(), part[1].cpu().numpy().view(np.uint32)), dev_level(g, pool, n_each=[5000, 20000, 77]))
        host = vs.polar_level_batched(pool)                                                  # NumPy in, NumPy out
        assert host[0].dtype == np.float64 and np.array_equal(host[0], want[0].astype(np.float64))
        assert host[1].dtype == np.int64 and np.array_equal(host[1], want[1])
        # one capture after the warm-up calls above; a synchronising or host-reading call would end the capture with an error
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            glevels, gcounts, _, _ = vs.polar_level_batched(t)
        for seed in (43, 44):
            fresh = make_pool(np.float32, 20000, seed=seed)
            t.copy_(_upload(g, fresh))
            glevels.fill_(-1.0)
            gcounts.fill_(9)
            graph.replay()
            torch.cuda.synchronize()
            same((glevels.cpu().numpy(), gcounts.cpu().numpy().view(np.uint32)), dev_level(g, fresh))
    finally:
        vs.set_scope_device(None)


def test_refusals_write_nothing(gpu):
    """Every refusal of the header returns its status with outputs and work memory untouched, guard bands included."""
    g = gpu
    torch, lib = g.torch, g.ctx._lib
    batch, n, bins, num_p = 3, 100, 360, 2
    pool = _upload(g, make_pool(np.float32, n, seed=45))
    edges = _upload(g, np.concatenate([np.linspace(-90.0, 90.0, bins + 1), np.full(1026 - bins - 1, 90.0)]))   # room for 1025 slices
    each = _upload(g, np.array([n, n, n], np.int32))
    levels = Guarded(g, batch * 5 * 1025, torch.float32, -777.0)
    counts = Guarded(g, batch * 1025, torch.int32, 0x5a5a5a5a)
    need = g.native.polar_level_work_bytes(batch, n, 1024, 4)
    work = Guarded(g, need // 8, torch.int64, 0x0123456789abcdef)
    ps = (ctypes.c_double * 5)(95.0, 50.0, 0.0, 100.0, 12.5)
    stream = torch.cuda.current_stream(g.device).cuda_stream
    base = dict(ctx=g.ctx.handle, l=pool.data_ptr(), r=pool.data_ptr() + 4, batch=batch, n=n, ss=2 * n, fs=2, ms=1, semi=1,
                scale=0.0, edges=edges.data_ptr(), bins=bins, ps=ps, num_p=num_p, each=each.data_ptr(), levels=levels.ptr(),
                counts=counts.ptr(), work=work.ptr(), work_bytes=need)

    def call(**kw):
        a = dict(base, **kw)
        return lib.vnd_polar_level_f32_dev(a['ctx'], a['l'], a['r'], a['batch'], a['n'], a['ss'], a['fs'], a['ms'], a['semi'],
                                           a['scale'], a['edges'], a['bins'], a['ps'], a['num_p'], a['each'], a['levels'],
                                           a['counts'], a['work'], a['work_bytes'], stream)
    bad_p = (ctypes.c_double * 2)(50.0, 100.5)
    nan_p = (ctypes.c_double * 2)(float('nan'), 50.0)
    exact = g.native.polar_level_work_bytes(batch, n, bins, num_p)
    refusals = [
        (INVALID, dict(ctx=None)), (INVALID, dict(l=None)), (INVALID, dict(r=None)), (INVALID, dict(edges=None)),
        (INVALID, dict(ps=None)), (INVALID, dict(levels=None)), (INVALID, dict(counts=None)), (INVALID, dict(work=None)),
        (INVALID, dict(batch=0)), (INVALID, dict(n=0)), (INVALID, dict(ss=0)), (INVALID, dict(fs=0)), (INVALID, dict(bins=0)),
        (INVALID, dict(num_p=0)), (INVALID, dict(ps=bad_p)), (INVALID, dict(ps=nan_p)), (INVALID, dict(scale=float('nan'))),
        (INVALID, dict(scale=float('inf'))), (INVALID, dict(scale=1e-60)),
        (INVALID, dict(work_bytes=exact - 1)), (INVALID, dict(work=work.ptr() + 4)),
        (INVALID, dict(levels=pool.data_ptr() + 16)), (INVALID, dict(counts=edges.data_ptr() + 8)),
        (INVALID, dict(work=each.data_ptr())), (INVALID, dict(counts=levels.ptr() + 64)), (INVALID, dict(levels=work.ptr() + 128)),
        (UNSUPPORTED, dict(bins=1025)), (UNSUPPORTED, dict(num_p=5)), (UNSUPPORTED, dict(n=2 ** 32, ss=2 ** 33)),
        (UNSUPPORTED, dict(batch=65536, n=1, ss=1, fs=1)), (UNSUPPORTED, dict(batch=65535, n=2 ** 24, ss=1, fs=1)),
    ]
    for status, kw in refusals:
        assert call(**kw) == status, kw
    torch.cuda.synchronize()
    assert levels.untouched() and counts.untouched() and work.untouched()
    assert call(work_bytes=exact) == 0                              # and the same arguments, valid, run
    torch.cuda.synchronize()
    got = levels.check()[:batch * num_p * bins].reshape(batch, num_p, bins)
    assert got.tobytes() == dev_level(g, pool.cpu().numpy())[0].tobytes()
    with pytest.raises(ValueError, match='percentile'):
        g.native.polar_level_device(g.ctx, base['l'], base['r'], batch, n, 2 * n, 2, base['edges'], bins, [101.0], levels.ptr(),
                                    counts.ptr(), work_ptr=work.ptr(), work_bytes=need)
    with pytest.raises(g.native.NativeError, match='percentiles'):
        g.native.polar_level_device(g.ctx, base['l'], base['r'], batch, n, 2 * n, 2, base['edges'], bins, [1.0] * 5, levels.ptr(),
                                    counts.ptr(), work_ptr=work.ptr(), work_bytes=need)

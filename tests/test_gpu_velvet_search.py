"""GPU tier of the batched velvet-noise optimiser (vnd_velvet_pairs_f32_*, include/vnd_velvet_search.h, and
optimize_velvet_noise_batched): the kernel's frames against the oracle's class-path convolution exactly, its moments
against float64 NumPy and against the existing single-signal scan, the determinism contract bit for bit, bad pairs,
the device scorer through SciPy, the reference's objective fixtures, pool independence, and that the work stays on the
device."""
import contextlib
import io
import warnings

import numpy as np
import pytest

import scan_ref
from conftest import make_input
from oracle import vnd_oracle as O

pytestmark = pytest.mark.gpu

SCORE_TOL = 2e-4          # tests/test_gpu_optimization.py's constant: absolute, on scores of ~619
WEIGHTS = dict(angle_limit=np.pi / 4, lambda_mean=5.0, lambda_skew=2.0, lambda_correlation=15.0, lambda_penalty=1e3)
FS, DURATION, IMPULSES, SEED = 16000, 0.02, 15, 1        # a small filter: 320 frames, 15 taps
TILE = 2048


def quiet(fn, *args, **kwargs):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*args, **kwargs)


@pytest.fixture(scope='module')
def ctx():
    from vndecorrelate_amd import _native
    context = _native.default_context()
    assert 'gfx950' in context.info()['name']
    return context


@pytest.fixture
def opt(ctx):
    from vndecorrelate_amd import optimization
    optimization.set_velvet_search_device(True)
    yield optimization
    optimization.set_velvet_search_device(None)


def _taps(kappa, *, filtered=(0,), envelope=O.DEFAULT_ENVELOPE, seed=SEED):
    return O.generate_class_taps(sample_rate_hz=FS, duration_seconds=DURATION, num_impulses=IMPULSES,
                                 segment_envelope=envelope, log_distribution_strength=kappa,
                                 filtered_channels=filtered, seed=seed)


def _class_bank(ctx, members, envelope):
    """A class-path bank of oracle tap lists, and the oracle's own convolution of a stereo signal per member."""
    from vndecorrelate_amd import _native
    from vndecorrelate_amd.taps import class_path_bank_arrays
    env = tuple(envelope)
    arrays = class_path_bank_arrays([(taps, env, env != (1.0,)) for taps in members])
    return _native.TapTable.create(ctx, arrays.tap_offsets, arrays.tap_index, arrays.tap_weight, **arrays.kwargs())


def _stereo(x):
    return np.repeat(x, 2, axis=1) if x.shape[1] == 1 else x


_moments64 = scan_ref.moments64      # tests/test_gpu_optimization.py's reference: float32 element maths as NumPy, float64 sums
_term_sums = scan_ref.term_sums      # sum of |term| of every summed slot (slot 4, a maximum, gets 0)


# ---- 1. frames, exactly ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('channels', [1, 2])
@pytest.mark.parametrize('envelope', [(1.0,), (1.0, 0.5, 0.25)])
def test_frames_are_the_oracles_exactly(ctx, channels, envelope):
    """Integer samples in [-3, 3] and power-of-two gains: L*R, L^2 and R^2 are exact in float32 and their float64 sums
    exact in any order, so slots 5, 6, 7 equal NumPy's on the oracle's frames bit for bit - any wrong frame shows."""
    from vndecorrelate_amd import _native
    rng = np.random.default_rng(100 + channels + len(envelope))
    members = [_taps(0.0, envelope=envelope), _taps(0.4, envelope=envelope), _taps(1.0, envelope=envelope),
               _taps(0.7, filtered=(0, 1), envelope=envelope, seed=5),        # both channels filtered
               _taps(0.2, filtered=(0, 1), envelope=envelope, seed=9)]
    bank = _class_bank(ctx, members, envelope)
    try:
        assert bank.max_index > 200
        for n in (1, 200, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 5000):   # 200: shorter than the largest tap index
            pool = rng.integers(-3, 4, (3, n, channels)).astype(np.float32)
            sig = np.repeat(np.arange(3), len(members))
            cand = np.tile(np.arange(len(members)), 3)
            got = _native.velvet_pairs_host(ctx, bank, pool, sig, cand)
            for p, (s, c) in enumerate(zip(sig, cand)):
                y = O.class_convolve(_stereo(pool[s]), members[c], envelope, 2)
                want = _moments64(y)
                assert got[p][5:].tobytes() == want[5:].tobytes(), (n, int(s), int(c), got[p][5:], want[5:])
                assert np.all(np.isfinite(got[p]))
    finally:
        bank.close()


@pytest.mark.parametrize('channels', [1, 2])
def test_function_path_bank_frames_exactly(ctx, channels):
    from vndecorrelate_amd import _native
    from vndecorrelate_amd.taps import function_path_arrays
    rng = np.random.default_rng(7 + channels)
    fir = O.generate_velvet_noise(duration_seconds=DURATION, num_impulses=IMPULSES, num_outs=6, sample_rate_hz=FS,
                                  segment_envelope=(1.0, 0.5, 0.25), log_distribution_strength=0.6, seed=3)
    arrays = function_path_arrays(fir)
    bank = _native.TapTable.create(ctx, arrays.tap_offsets, arrays.tap_index, arrays.tap_weight)
    try:
        for n in (150, TILE, TILE + 77, 4500):
            pool = rng.integers(-3, 4, (2, n, channels)).astype(np.float32)
            sig, cand = np.array([0, 0, 0, 1, 1, 1]), np.array([0, 1, 2, 0, 1, 2])
            got = _native.velvet_pairs_host(ctx, bank, pool, sig, cand)
            for p, (s, c) in enumerate(zip(sig, cand)):
                y = O.convolve_velvet_noise(_stereo(pool[s]), fir[:, 2 * c:2 * c + 2])
                assert got[p][5:].tobytes() == _moments64(y)[5:].tobytes(), (n, int(s), int(c))
    finally:
        bank.close()


# ---- 2. moments, general input ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('channels', [1, 2])
def test_moments_against_numpy(ctx, channels):
    from vndecorrelate_amd import _native
    rng = np.random.default_rng(20 + channels)
    envelope = O.DEFAULT_ENVELOPE
    members = [_taps(0.0), _taps(0.55), _taps(1.0), _taps(0.3, filtered=(0, 1), seed=4)]
    bank = _class_bank(ctx, members, envelope)
    try:
        for n in (777, TILE, 3 * TILE + 5):
            pool = rng.uniform(-1, 1, (2, n, channels)).astype(np.float32)
            pool[1, n // 2] = 0.0
            sig, cand = np.repeat(np.arange(2), 4), np.tile(np.arange(4), 2)
            got = _native.velvet_pairs_host(ctx, bank, pool, sig, cand)
            for p, (s, c) in enumerate(zip(sig, cand)):
                y = O.class_convolve(_stereo(pool[s]), members[c], envelope, 2)
                want = _moments64(y)
                # the bounds of test_gpu_optimization.py's moments test: 3e-8 * the scale of the sum's terms
                # (atan2f and NumPy's float32 arctan2 differ by an ulp on some samples), one float32 ulp on max |theta|
                scale = _moments64(np.abs(y) * np.array([1.0, 0.5], np.float32))
                scale[1:4] = want[0] * np.array([np.pi / 2, (np.pi / 2) ** 2, (np.pi / 2) ** 3])
                assert np.all(np.abs(got[p] - want) <= 3e-8 * np.maximum(scale, 1.0)), (n, p, got[p], want)
                assert got[p][4] == want[4] or abs(got[p][4] - want[4]) <= 2.4e-7
    finally:
        bank.close()


# ---- 3. against the existing scan ------------------------------------------------------------------------------------
@pytest.mark.parametrize('channels', [1, 2])
def test_rows_equal_the_single_signal_scan_up_to_summation_order(ctx, channels):
    from vndecorrelate_amd import _native
    rng = np.random.default_rng(30 + channels)
    members = [_taps(k) for k in (0.0, 0.25, 0.5, 0.75, 1.0)]
    bank = _class_bank(ctx, members, O.DEFAULT_ENVELOPE)
    try:
        for n in (1500, 3 * TILE + 9, 50001):
            x = rng.uniform(-1, 1, (n, channels)).astype(np.float32)
            want = bank.scan_host(x, _native.MODE_EXACT)
            got = _native.velvet_pairs_host(ctx, bank, x[None], np.zeros(5, np.int64), np.arange(5))
            for c in range(5):
                y = O.class_convolve(_stereo(x), members[c], O.DEFAULT_ENVELOPE, 2)
                bound = (n - 1) * 2.0 ** -52 * _term_sums(y)     # the float64 reordering bound: equal elements
                assert got[c][4].tobytes() == want[c][4].tobytes(), (n, c)
                assert np.all(np.abs(got[c] - want[c]) <= bound), (n, c, got[c] - want[c], bound)
    finally:
        bank.close()


# ---- 4. invariance, bit for bit --------------------------------------------------------------------------------------
def _device_rows(ctx, bank, pool, sig, cand, *, side=True):
    import torch
    from vndecorrelate_amd import _native
    dev = torch.device('cuda', ctx.device)
    xd = torch.from_numpy(pool).to(dev)
    pairs = torch.from_numpy(np.stack([sig, cand]).astype(np.int32)).to(dev)
    ws = _native.velvet_pairs_workspace_bytes(pool.shape[1], len(sig))
    wd = torch.empty(max(ws, 1), dtype=torch.uint8, device=dev)
    md = torch.full((len(sig), 8), -7.0, dtype=torch.float64, device=dev)
    stream = torch.cuda.Stream(dev) if side else torch.cuda.current_stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        _native.velvet_pairs_device(ctx, bank, xd.data_ptr(), pool.shape[0], pool.shape[1], pool.shape[2],
                                    pairs[0].data_ptr(), pairs[1].data_ptr(), len(sig), md.data_ptr(),
                                    workspace_ptr=wd.data_ptr(), workspace_bytes=ws, stream=stream.cuda_stream)
    stream.synchronize()
    return md.cpu().numpy()


@pytest.mark.parametrize('channels', [1, 2])
def test_rows_depend_on_signal_and_candidate_only(ctx, channels):
    from vndecorrelate_amd import _native
    rng = np.random.default_rng(50 + channels)
    a, b, c = _taps(0.1), _taps(0.6), _taps(0.9, filtered=(0, 1), seed=2)
    members = [a, b, c, a, b]                              # candidates 0 and 3, 1 and 4: one table at two positions
    bank = _class_bank(ctx, members, O.DEFAULT_ENVELOPE)
    alone = {k: _class_bank(ctx, [m], O.DEFAULT_ENVELOPE) for k, m in enumerate((a, b, c))}
    try:
        n = 2 * TILE + 333
        pool = rng.uniform(-1, 1, (4, n, channels)).astype(np.float32)
        pool[3] = pool[0]                                  # one signal at two pool indices
        base = {(s, k): _native.velvet_pairs_host(ctx, alone[k], np.ascontiguousarray(pool[s:s + 1]), [0], [0])[0]
                for s in range(3) for k in range(3)}
        sig = np.repeat(np.arange(4), 5)
        cand = np.tile(np.arange(5), 4)
        perm = rng.permutation(sig.size)
        sig = np.concatenate([sig[perm], sig[:7], sig[perm][:3]])           # shuffled, with duplicate pairs
        cand = np.concatenate([cand[perm], cand[:7], cand[perm][:3]])
        got = _native.velvet_pairs_host(ctx, bank, pool, sig, cand)
        for p, (s, k) in enumerate(zip(sig, cand)):
            assert got[p].tobytes() == base[(int(s) % 3, int(k) % 3)].tobytes(), (p, int(s), int(k))
        cuts = [0, 1, 16, 17, 23, sig.size]                # the same pairs split into several calls
        parts = np.concatenate([_native.velvet_pairs_host(ctx, bank, pool, sig[i:j], cand[i:j])
                                for i, j in zip(cuts, cuts[1:])])
        assert parts.tobytes() == got.tobytes()
        assert _device_rows(ctx, bank, pool, sig, cand).tobytes() == got.tobytes()      # _dev on a side stream
    finally:
        bank.close()
        for t in alone.values():
            t.close()


# ---- 5. bad pairs, refusals ------------------------------------------------------------------------------------------
def test_bad_pairs(ctx):
    from vndecorrelate_amd import _native
    lib = _native.load_library()
    rng = np.random.default_rng(8)
    B, n = 3, 5000
    pool = rng.uniform(-1, 1, (B, n, 2)).astype(np.float32)
    bank = _class_bank(ctx, [_taps(0.2), _taps(0.8)], O.DEFAULT_ENVELOPE)
    try:
        for sig, cand, word in (([0, 3], [1, 1], 'signal 3 of pair 1'), ([0, -1], [1, 1], 'signal -1 of pair 1'),
                                ([1, 1, 1], [0, 1, 2], 'candidate 2 of pair 2'), ([2], [-1], 'candidate -1 of pair 0')):
            with pytest.raises(ValueError, match=word):
                _native.velvet_pairs_host(ctx, bank, pool, sig, cand)
            assert word.encode() in lib.vnd_last_error()
        with pytest.raises(_native.NativeError, match='VND_MODE_EXACT only'):         # VND_ERR_UNSUPPORTED
            _native.velvet_pairs_host(ctx, bank, pool, [0], [0], mode=_native.MODE_FAST)
        with pytest.raises(ValueError, match='mono or stereo'):
            _native.velvet_pairs_host(ctx, bank, np.zeros((1, 10, 3), np.float32), [0], [0])
        odd = _native.TapTable.create(ctx, [0, 1, 2, 3], [0, 1, 2], [1.0, 1.0, 1.0])
        try:
            with pytest.raises(ValueError, match='stereo pairs'):
                _native.velvet_pairs_host(ctx, odd, pool, [0], [0])
        finally:
            odd.close()
        # on _dev: NaN rows for a bad signal or candidate from the kernel's bounds checks; the others as alone
        sig = np.array([0, 3, 1, -1, 2, 1, 2, 0], np.int32)
        cand = np.array([0, 1, 2, 1, 1, -5, 0, 1], np.int32)
        got = _device_rows(ctx, bank, pool, sig, cand)
        for p in (1, 2, 3, 5):
            assert np.isnan(got[p]).all(), p
        for p in (0, 4, 6, 7):
            want = _native.velvet_pairs_host(ctx, bank, pool, [sig[p]], [cand[p]])
            assert got[p].tobytes() == want[0].tobytes(), p
    finally:
        bank.close()


def test_bank_beyond_the_staged_window_takes_the_host_route(ctx, opt):
    """The documented treatment of tables whose largest tap index exceeds the staged window: VND_ERR_UNSUPPORTED from
    the library, and the batched optimiser takes the host route for that call."""
    from vndecorrelate_amd import _native
    bank = _native.TapTable.create(ctx, [0, 1, 2], [_native.VELVET_PAIRS_MAX_TAP_INDEX + 1, 0], [1.0, 1.0])
    inside = _native.TapTable.create(ctx, [0, 1, 2], [_native.VELVET_PAIRS_MAX_TAP_INDEX, 0], [1.0, 1.0])
    try:
        x = np.random.default_rng(3).integers(-3, 4, (1, 6000, 2)).astype(np.float32)
        with pytest.raises(_native.NativeError, match='largest tap index'):
            _native.velvet_pairs_host(ctx, bank, x, [0], [0])
        got = _native.velvet_pairs_host(ctx, inside, x, [0], [0])[0]      # the largest window the kernel stages
        y = x[0].copy()
        y[:, 0] = 0.0
        y[:6000 - _native.VELVET_PAIRS_MAX_TAP_INDEX, 0] = x[0, _native.VELVET_PAIRS_MAX_TAP_INDEX:, 0]
        assert got[5:].tobytes() == _moments64(y)[5:].tobytes()
    finally:
        bank.close()
        inside.close()
    pool = np.random.default_rng(4).uniform(-1, 1, (2, 900, 2)).astype(np.float32)
    kw = dict(sample_rate_hz=44100, duration_seconds=0.1, num_impulses=30, seed=1, grid_size=5)   # 4410-frame filters
    printed, loop = io.StringIO(), io.StringIO()
    with contextlib.redirect_stdout(printed):
        got = opt.optimize_velvet_noise_batched(input_signals=pool, **kw)
    assert opt.last_velvet_search.route == 'host'
    with contextlib.redirect_stdout(loop):
        want = [opt.optimize_velvet_noise(input_signal=pool[b], **kw) for b in range(2)]
    assert got.tobytes() == np.asarray(want, np.float64).tobytes()
    assert printed.getvalue() == loop.getvalue()            # the host route's lines, no device-route lines before them


# ---- 6. through SciPy ------------------------------------------------------------------------------------------------
KW = dict(sample_rate_hz=FS, duration_seconds=DURATION, num_impulses=IMPULSES, seed=SEED)


def _pool(batch, n, channels=2, seed=0):
    rng = np.random.default_rng(seed)
    base = rng.uniform(-1, 1, (batch, n, 1))
    x = (base * np.array([1.0, 0.6]) + 0.4 * rng.uniform(-1, 1, (batch, n, 2))).astype(np.float32)
    return x[..., 0].copy() if channels == 1 else x


def test_batched_equals_scipy_driven_by_the_device_score(ctx, opt):
    from scipy.optimize import minimize_scalar
    from vndecorrelate_amd import _native
    grid = 21
    pool = _pool(16, 3000, seed=6)
    pool[5, :, 1] = pool[5, :, 0]                          # one signal with identical channels
    got = quiet(opt.optimize_velvet_noise_batched, input_signals=pool, grid_size=grid, **KW)
    stats = opt.last_velvet_search
    assert stats.route == 'device' and got.shape == (16,) and got.dtype == np.float64
    bank = opt.VelvetBank(**KW)
    kappas = np.linspace(0.0, 1.0, grid)
    memo = {}

    def score(b, kappa):
        key = (b, bank.keys([kappa]).tobytes())
        if key not in memo:
            arrays = bank.arrays([kappa])
            table = _native.TapTable.create(ctx, arrays.tap_offsets, arrays.tap_index, arrays.tap_weight,
                                            **arrays.kwargs())
            try:
                m = _native.velvet_pairs_host(ctx, table, np.ascontiguousarray(pool[b:b + 1]), [0], [0])
            finally:
                table.close()
            memo[key] = float(opt.scores_from_moments(m, **WEIGHTS)[0])
        return memo[key]

    for b in range(16):
        scores = np.array([score(b, k) for k in kappas])
        minima = opt.get_local_minima(scores, grid)
        nfev = []

        def f(kappa, b=b):
            return score(b, kappa)
        for i in minima:
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                nfev.append(minimize_scalar(f, bounds=(kappas[max(0, i - 1)], kappas[min(grid - 1, i + 1)]),
                                            method='bounded', options={'xatol': 1e-4}).nfev)
        want = quiet(opt.optimize_local_minima, minima, kappas, grid, f)
        assert got[b].tobytes() == np.float64(want).tobytes(), (b, got[b], want)
        assert stats.minimum_nfev[stats.minimum_signal == b].tolist() == nfev, b
        assert stats.evaluations[b] == sum(nfev), b


# ---- 7. against the reference's objective ----------------------------------------------------------------------------
def _fixture_signal(golden, meta):
    return golden.arrays[meta['input']] if isinstance(meta['input'], str) else make_input(meta['input'])


def _device_scores(ctx, opt, bank, x, kappas, weights):
    from vndecorrelate_amd import _native
    keys, inverse = opt._distinct_rows(bank.keys(kappas))
    arrays = bank.arrays_of_keys(keys)
    table = _native.TapTable.create(ctx, arrays.tap_offsets, arrays.tap_index, arrays.tap_weight, **arrays.kwargs())
    try:
        pool = np.ascontiguousarray(x.reshape(1, x.shape[0], -1), np.float32)
        m = _native.velvet_pairs_host(ctx, table, pool, np.zeros(len(keys), np.int64), np.arange(len(keys)))
    finally:
        table.close()
    return opt.scores_from_moments(m, **weights)[inverse]


def test_grid_scores_against_the_reference(ctx, opt, golden):
    for name, meta in golden.manifest['objective'].items():
        sig = _fixture_signal(golden, meta)
        bank = opt.VelvetBank(sample_rate_hz=meta['sample_rate_hz'], duration_seconds=0.03, num_impulses=30, seed=1)
        got = _device_scores(ctx, opt, bank, np.asarray(sig, np.float32), meta['kappas'], meta['kwargs'])
        want = golden.arrays[f'obj_{name}_scores']
        print(f'{name}: max |device - reference| grid score {np.max(np.abs(got - want)):.3e}')
        assert got.shape == want.shape and np.max(np.abs(got - want)) <= SCORE_TOL, (name, got - want)
        assert opt.get_local_minima(got, len(got)) == meta['local_minima'], name


def test_refinement_scores_against_the_host_objective_on_viola(ctx, opt, golden):
    """Every kappa the refinement evaluated has a device score within SCORE_TOL of the host objective (bit-identical to
    the reference's).  The returned kappa itself is recorded, not asserted: the objective is piecewise constant and
    Brent's parabolic steps use the score values, so a 1e-5 score difference changes the path."""
    from vndecorrelate_amd.decorrelation import VelvetNoise
    meta = golden.manifest['objective']['viola_excerpt']
    sig = golden.arrays['viola_excerpt_in']
    kw = dict(sample_rate_hz=44100, duration_seconds=0.03, num_impulses=30, seed=1)
    host_kappa = quiet(opt.optimize_velvet_noise, input_signal=sig, grid_size=9, **kw)
    assert abs(host_kappa - meta['optimize_velvet_noise_grid9']) <= 1e-6      # the host search is what it was
    got = quiet(opt.optimize_velvet_noise_batched, input_signals=sig[None], grid_size=9, **kw)
    stats = opt.last_velvet_search
    assert stats.route == 'device' and stats.grid_tables == 9
    evaluated = np.concatenate([k for _, k in stats.evaluated])
    assert evaluated.size == stats.evaluations.sum() > 0

    def host(kappa):
        return opt.symmetry_aware_objective(sig, VelvetNoise(log_distribution_strength=kappa, normalizer=None,
                                                             filtered_channels=(0,), mode='LR', **kw), **meta['kwargs'])
    bank = opt.VelvetBank(**kw)
    device = _device_scores(ctx, opt, bank, sig, evaluated, meta['kwargs'])
    worst = max(abs(device[j] - host(k)) for j, k in enumerate(evaluated))
    print(f'viola grid 9: batched kappa {got[0]!r} (host / reference kappa {host_kappa!r}, distance '
          f'{abs(got[0] - host_kappa):.3e}); host scores {host(got[0])!r} (batched) / {host(host_kappa)!r} (host); '
          f'nfev {stats.minimum_nfev.tolist()}; worst |device - host| over {evaluated.size} evaluated kappa {worst:.3e}')
    assert worst <= SCORE_TOL


# ---- 8. pools --------------------------------------------------------------------------------------------------------
def test_pools(ctx, opt, monkeypatch):
    grid = 17
    pool = _pool(6, 2600, seed=11)
    got = quiet(opt.optimize_velvet_noise_batched, input_signals=pool, grid_size=grid, **KW)
    assert opt.last_velvet_search.pool_uploads == 1
    perm = np.array([4, 0, 5, 2, 1, 3])
    assert quiet(opt.optimize_velvet_noise_batched, input_signals=pool[perm], grid_size=grid, **KW).tobytes() \
        == got[perm].tobytes()
    assert quiet(opt.optimize_velvet_noise_batched, input_signals=pool[1:4], grid_size=grid, **KW).tobytes() \
        == got[1:4].tobytes()
    monkeypatch.setattr(opt, '_VELVET_POOL_BYTES', 2 * pool[0].nbytes)          # a small upload budget: 3 chunks
    small = quiet(opt.optimize_velvet_noise_batched, input_signals=pool, grid_size=grid, **KW)
    assert small.tobytes() == got.tobytes() and opt.last_velvet_search.pool_uploads == 3
    assert opt.last_velvet_search.evaluations.size == 6
    monkeypatch.undo()
    opt.set_velvet_search_device(True)
    mono = _pool(4, 2600, channels=1, seed=12)
    many = quiet(opt.optimize_velvet_noise_batched, input_signals=mono, grid_size=grid, **KW)
    one = quiet(opt.optimize_velvet_noise_batched, input_signals=mono[2:3], grid_size=grid, **KW)
    assert one.tobytes() == many[2:3].tobytes()
    as_float64 = quiet(opt.optimize_velvet_noise_batched, input_signals=mono.astype(np.float64), grid_size=grid, **KW)
    assert as_float64.tobytes() == many.tobytes()


# ---- 9. work stays on the device -------------------------------------------------------------------------------------
def test_work_stays_on_the_device(ctx, opt, monkeypatch):
    import torch
    import vndecorrelate_amd.decorrelation as dec
    grid = 17
    pool = _pool(5, 2600, seed=13)
    before = quiet(opt.optimize_velvet_noise, input_signal=pool[1], grid_size=grid, **KW)
    want = quiet(opt.optimize_velvet_noise_batched, input_signals=pool, grid_size=grid, **KW)

    def refuse(*args, **kwargs):
        raise AssertionError('the host objective ran')
    monkeypatch.setattr(opt, 'symmetry_aware_objective', refuse)
    tensor = torch.from_numpy(pool).to(torch.device('cuda', ctx.device))
    dec.set_default_mode(dec.MODE_FAST)                    # the batched search is VND_MODE_EXACT whatever this says
    try:
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            got = opt.optimize_velvet_noise_batched(input_signals=tensor, grid_size=grid, **KW)
    finally:
        dec.set_default_mode(dec.MODE_EXACT)
    assert buf.getvalue() == 'Starting Grid Scan\nStarting Local Minima optimization\n'
    stats = opt.last_velvet_search
    assert got.tobytes() == want.tobytes()
    assert stats.route == 'device' and stats.pool_uploads == 0
    assert stats.grid_launches == 1 and stats.launches == stats.grid_launches + stats.rounds
    assert stats.launch_pool == [tensor.data_ptr()] * stats.launches          # read in place
    assert stats.launch_pairs[0] == stats.grid_pairs and stats.launch_pairs[1:] == stats.pairs_per_round
    assert len(stats.launch_ms) == stats.launches and all(ms > 0 for ms in stats.launch_ms)
    monkeypatch.undo()
    opt.set_velvet_search_device(True)
    after = quiet(opt.optimize_velvet_noise, input_signal=pool[1], grid_size=grid, **KW)
    assert np.float64(after).tobytes() == np.float64(before).tobytes()       # the host search is untouched

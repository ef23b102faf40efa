"""GPU tier of the tap-table gate: what ``vnd_taps_create`` ADMITS at its edges - any tap order, duplicate indices, zero
weights, empty channels and segments, a table without taps, indices up to 2^30, copy-through channels that carry taps,
gains that are ignored, zero or not finite - handed raw to ``TapTable.create`` and run through every kernel family the
library can pick or be told to pick, against the C oracle of the same table: VND_MODE_EXACT and VND_MODE_FMA bit for bit,
VND_MODE_FAST within the fuzz tier's bound for cancelling taps.  Then the images: serialise / rebuild / serialise is the
identity, mutated images the contract's mirror (tests/taps_gate.py) admits run as the mutated table, those it refuses are
refused.  No kernel here meets a table the mirror calls invalid.

One test per (table, family): at most two run-time kernel builds each (fast and exact form)."""
import numpy as np
import pytest

import taps_gate as G
from oracle import c_oracle
from test_gpu_fuzz import FORCE, GENERIC, WIN, span_bits
from test_gpu_fuzz_hypothesis import _term_scale

pytestmark = pytest.mark.gpu

N = 10000                 # a multiple of 4: the smallest length at which the forced family is known to run (tests/test_gpu_fuzz.py)
SHAPES = [(N, 1), (N, 3), (37, 1), (37, 3)]
FAMILIES = {
    'automatic': (-1, {}),
    'generic': (GENERIC, {}),
    'pair-read': (FORCE | WIN[0] | span_bits(1, 3), {}),
    'window 32': (FORCE | WIN[32] | span_bits(1, 3), {}),
    'window 16': (FORCE | WIN[16] | span_bits(2, 1), {}),
    'window 64 split': (FORCE | WIN[64] | span_bits(1, 3), {'VND_WIN_SPLIT': '2', 'VND_SPEC_NT': '256'}),
}
TABLES = {t.name: t for t in G.edge_tables(N)}
FANNED_OUT = [name for name, t in TABLES.items() if t.C == 2 and name.startswith(('unsorted', 'duplicate'))]


def _cases():
    """(table, input channels, family): the per-table families only where the table is within their scope."""
    out = []
    for name, t in TABLES.items():
        for cx in [t.C] + ([1] if name in FANNED_OUT else []):
            families = ['automatic', 'generic']
            if G.per_table_scope(t, mode_exact=False):
                families += ['pair-read', 'window 32', 'window 16'] + (['window 64 split'] if t.C == 2 and cx == 2 else [])
            out += [pytest.param(name, cx, f, id=f'{name}{" (mono in)" if cx != t.C else ""}-{f}'.replace(' ', '_')) for f in families]
    return out


_REFERENCE = {}


def reference(name, cx, n, batch):
    """Input and the oracle's outputs for one (table, input channels, shape): computed once, shared by the families, read-only."""
    key = (name, cx, n, batch)
    if key not in _REFERENCE:
        t = TABLES[name].filled()
        rng = np.random.default_rng([list(TABLES).index(name), n, batch, cx])
        x = rng.uniform(-1, 1, (batch, n, cx)).astype(np.float32)
        x[rng.integers(0, batch, 20), rng.integers(0, n, 20), rng.integers(0, cx, 20)] = 0.0
        full = np.ascontiguousarray(np.repeat(x, t.C // cx, axis=2))          # a mono input feeds both channels
        with np.errstate(all='ignore'):
            want = c_oracle.convolve(full, t.tap_offsets, t.tap_index, t.tap_weight, **t.oracle_kwargs())
            want_fma = c_oracle.convolve_fma(full, t.tap_offsets, t.tap_index, t.tap_weight, **t.oracle_kwargs())
        for a in (x, want, want_fma):
            a.flags.writeable = False
        _REFERENCE[key] = (x, want, want_fma)
    return _REFERENCE[key]


@pytest.fixture(scope='module')
def ctx():
    from vndecorrelate_amd import _native
    c = _native.default_context()
    yield c
    c.set_variant(-1)


def _create(ctx, t):
    from vndecorrelate_amd import _native
    assert G.judge_create(t).admitted, t.name                  # nothing the mirror calls invalid reaches a kernel
    return _native.TapTable.create(ctx, t.tap_offsets, t.tap_index, t.tap_weight, **t.kwargs())


def _same_bits(got, want):
    return got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def _differ(got, want):
    bad = got.view(np.uint32) != want.view(np.uint32)
    return f'{int(bad.sum())} words differ, {int((bad & (got == want)).sum())} of them in the sign of a zero; largest distance ' \
           f'{float(np.max(np.abs(got.astype(np.float64) - want))):.3e}'


def _finite_gains(t):
    return t.seg_offsets is None or not t.apply_gain or bool(np.isfinite(t.seg_gain).all())


@pytest.mark.parametrize('name, cx, family', _cases())
def test_admitted_table_in_every_family(ctx, name, cx, family, monkeypatch, record_property):
    import vndecorrelate_amd.decorrelation as d
    t = TABLES[name]
    variant, env = FAMILIES[family]
    table = _create(ctx, t)
    ordinary = t.total > 0 and t.max_index <= G.SPAN + 16        # (a halo every per-table form holds)
    ran = {}
    try:
        ctx.set_variant(variant)
        for key in ('VND_WIN_SPLIT', 'VND_SPEC_NT'):
            monkeypatch.delenv(key, raising=False)
        for key, value in env.items():
            monkeypatch.setenv(key, value)
        for mode in (d.MODE_EXACT, d.MODE_FMA, d.MODE_FAST):
            for n, batch in SHAPES:
                x, want, want_fma = reference(name, cx, n, batch)
                text = table.describe(batch, n, cx, mode)
                where = f'{name} C={t.C} in={cx} {family} mode={mode} n={n} batch={batch}: {text[:70]}'
                # ---- which kernel: the family asked for, or the generic kernel describe() names -----------------------
                per_table = text.startswith('conv_spec')
                assert per_table or text.startswith(('conv_ordered', 'conv_fast', 'conv_direct')), where
                kernel = ' '.join(w for w in text.split(' ') if w.startswith(('conv_', 'frames_per_lane=', 'pairs_per_lane=')))
                ran[kernel] = ran.get(kernel, 0) + 1
                if mode == d.MODE_FMA or family in ('automatic', 'generic') or not G.per_table_scope(t, mode == d.MODE_EXACT):
                    assert not per_table, where                            # (automatic: far too little work for persistent workgroups)
                if t.total and t.max_index >= 1 << 24:                     # byte offsets no LDS kernel can hold
                    assert text.startswith('conv_direct'), where
                if per_table:
                    assert ('_window' in text) == family.startswith('window'), where
                    if family == 'window 64 split':
                        assert 'waves=split-by-channel' in text, where
                elif family not in ('automatic', 'generic') and mode != d.MODE_FMA and n == N and ordinary and \
                        G.per_table_scope(t, mode == d.MODE_EXACT):
                    pytest.fail(f'{where}: the family asked for did not run')
                # ---- what it computed ------------------------------------------------------------------------------------
                table.convolve_host(np.full_like(x, np.nan), mode)           # a frame nobody writes must not read back right
                got = table.convolve_host(x, mode)
                assert got.shape == want.shape and got.dtype == np.float32, where
                if not _finite_gains(t):
                    # as for a non-finite weight (tests/test_gpu_robustness.py): the oracle's NaN / inf pattern in every mode -
                    # the gain multiplies the segment's sum, dropped terms left out
                    assert np.array_equal(np.isnan(got), np.isnan(want)), where
                    assert np.array_equal(np.isinf(got), np.isinf(want)), where
                    fin = np.isfinite(want)
                    if mode == d.MODE_FMA:
                        assert np.array_equal(got[fin], want_fma[fin]), where
                    if mode == d.MODE_EXACT:
                        assert np.array_equal(got, want, equal_nan=True), where
                    assert np.allclose(got[fin], want[fin], rtol=1e-6, atol=1e-6), where
                    assert text.startswith('conv_direct'), where          # routed like a non-finite weight: the index-testing kernel
                elif mode == d.MODE_EXACT:
                    assert _same_bits(got, want), f'{where}: {_differ(got, want)}'
                elif mode == d.MODE_FMA:
                    assert _same_bits(got, want_fma), f'{where}: {_differ(got, want_fma)}'
                else:
                    peak = max(float(np.max(np.abs(want))) if want.size else 0.0, 1e-30)
                    floor = 2.0 ** -24 * _term_scale(t.filled(), x)
                    err = float(np.max(np.abs(got.astype(np.float64) - want)))
                    assert err <= 1e-6 * peak + floor + 1e-30, f'{where}: {err:.3e} against {1e-6 * peak + floor:.3e}'
    finally:
        ctx.set_variant(-1)
        table.close()
    record_property('kernels', ran)
    print(f'{name} (in={cx}) {family}: {ran}')


# ---- images ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(TABLES))
def test_image_round_trip_is_the_identity(ctx, name):
    """to_bytes -> from_bytes -> to_bytes gives the same bytes - the mirror's layout, and taps.TapArrays' - and the rebuilt
    table the same exact-mode output bits."""
    from vndecorrelate_amd import _native
    from vndecorrelate_amd.taps import TapArrays
    t = TABLES[name]
    table = _create(ctx, t)
    try:
        image = table.to_bytes()
        assert image == t.to_bytes(), name
        f = t.filled()
        assert image == TapArrays(f.tap_offsets, f.tap_index, f.tap_weight, f.seg_offsets, f.seg_end, f.seg_gain, f.chan_flags,
                                  bool(f.apply_gain)).to_bytes(), name
        assert G.judge_image(image).admitted
        rebuilt = _native.TapTable.from_bytes(ctx, image)
        try:
            assert rebuilt.to_bytes() == image, name
            assert (rebuilt.num_channels, rebuilt.total_taps, rebuilt.max_index) == (t.C, t.total, t.max_index)
            x, want, _ = reference(name, t.C, N, 1)
            for tab in (table, rebuilt):
                tab.convolve_host(np.full_like(x, np.nan), 0)
                assert np.array_equal(tab.convolve_host(x, 0), want, equal_nan=True), name
        finally:
            rebuilt.close()
    finally:
        table.close()


MUTANTS = G.mutated_images()


def test_admitted_mutants_run_as_the_mutated_table(ctx):
    """One word of a valid image changed and still a valid image (another weight, an index in range, another gain or
    flag, an ignored header word): admitted, and the output is the oracle's for the table the mirror reads from it."""
    from vndecorrelate_amd import _native
    admitted = [m for m in MUTANTS if m.verdict.admitted]
    regions = {m.name.split(': ')[1].split('[')[0] for m in admitted}
    assert {'w', 'idx', 'seg_gain', 'flags'} <= regions and len(admitted) > 300, regions
    rng = np.random.default_rng(11)
    inputs = {C: rng.uniform(-1, 1, (2, 61, C)).astype(np.float32) for C in (1, 2, 8)}
    for m in admitted:
        verdict, t = G.parse_image(m.image)
        assert verdict.admitted and G.judge_create(t).admitted, m.name
        x = inputs[t.C]
        with np.errstate(all='ignore'):
            want = c_oracle.convolve(x, t.tap_offsets, t.tap_index, t.tap_weight, **t.oracle_kwargs())
        table = _native.TapTable.from_bytes(ctx, m.image)
        try:
            assert (table.num_channels, table.total_taps, table.max_index) == (t.C, t.total, t.max_index), m.name
            table.convolve_host(np.full_like(x, np.nan), 0)
            assert np.array_equal(table.convolve_host(x, 0), want, equal_nan=True), m.name
        finally:
            table.close()


def test_refused_mutants_are_refused_with_a_real_context(ctx):
    """The CPU tier's refusals again, with a context that could build a table: status, message, ``*taps == NULL``."""
    from vndecorrelate_amd import _native
    lib = _native.load_library()
    refused = [m for m in MUTANTS if not m.verdict.admitted]
    assert len(refused) > 500
    for m in refused + [c for c in G.refusal_corpus() if c.group == 'listed' and not c.null_ctx]:
        status, message, left = G.call_case(lib, ctx.handle, m)
        assert (status, message) == (m.verdict.status, m.verdict.reason), m.name
        assert m.null_out or left is None, m.name

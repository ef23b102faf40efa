"""CPU tier of the count-grid voice pool (include/vnd_scope_voice_stream.h; vectorscope.ScopeVoicePool): the host mirror of
the slot rule against a scalar restatement, a NumPy model of the ring against histogram_counts of the window's frames, the
Python refusals that need no device, and the header against the library and the binding."""
import ctypes
import pathlib
import re
import subprocess

import numpy as np
import pytest

REPO = pathlib.Path(__file__).resolve().parents[1]
HEADER = REPO / 'include' / 'vnd_scope_voice_stream.h'
START, END = 1, 2
INVALID, UNSUPPORTED = 1, 4
NAMES = sorted(['vnd_scope_voice_stream_state_bytes', 'vnd_scope_voice_stream_reset_dev', 'vnd_polar_hist_voice_stream_f32_dev',
                'vnd_polar_hist_voice_stream_f64_dev', 'vnd_lissajous_hist_voice_stream_f32_dev',
                'vnd_lissajous_hist_voice_stream_f64_dev'])


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as entry
    entry.build()
    from vndecorrelate_amd import _native
    return _native.load_library()


@pytest.fixture(scope='module')
def vs():
    from vndecorrelate_amd import vectorscope
    return vectorscope


# ---- the slot rule ---------------------------------------------------------------------------------------------------
def scalar_span(pos, count, flags, M):
    """include/vnd_scope_voice_stream.h, one slot, in Python integers: (valid, new position)."""
    p = 0 if flags & START else pos
    if count < 0 or count > M or p < 0 or p > 2 ** 60:
        return -1, pos
    if count == 0 and not flags & (START | END):
        return 0, pos
    return 1, (0 if flags & END else p + count)


def test_spans_against_the_scalar_rule_on_the_corner_grid(vs):
    M = 37
    counts = [-1, 0, M, M + 1, 5]
    positions = [0, 7, 2 ** 31 - 7, 2 ** 32 - 300, 2 ** 40 + 3, 2 ** 60, 2 ** 60 + 1, -3]
    flags = [0, START, END, START | END, 4, 4 | START]
    grid = [(p, c, f) for p in positions for c in counts for f in flags]
    pos, cnt, flg = (np.array(v, np.int64) for v in zip(*grid))
    valid, new = vs.scope_voice_spans(pos, cnt, flg, M)
    assert valid.dtype == new.dtype == np.int64
    for i, (p, c, f) in enumerate(grid):
        assert (int(valid[i]), int(new[i])) == scalar_span(p, c, f, M), (p, c, f)
    assert set(valid.tolist()) == {-1, 0, 1}
    # without a limit a count above M passes
    assert vs.scope_voice_spans([0], [M + 1], [0])[0].tolist() == [1]


def test_window(vs):
    assert vs.scope_voice_window(100, 64) == (36, 100)
    assert vs.scope_voice_window(50, 64) == (0, 50)
    assert vs.scope_voice_window(2 ** 40 + 3, 64) == (2 ** 40 - 61, 2 ** 40 + 3)
    assert vs.scope_voice_window(100, None) == (0, 100) == vs.scope_voice_window(100, 0)
    assert vs.scope_voice_window(0, 5) == (0, 0)
    with pytest.raises(ValueError):
        vs.scope_voice_window(-1, 5)
    with pytest.raises(ValueError):
        vs.scope_voice_window(1, -5)


# ---- the ring, modelled ----------------------------------------------------------------------------------------------
class RingModel:
    """One slot of the device's rule in NumPy: the grid row, the ring of cells (pre-filled with a valid cell, as the GPU
    tier's poisoned state is, and never cleared) and the position."""

    def __init__(self, vs, e0, e1, W):
        self.vs, self.e0, self.e1, self.W = vs, e0, e1, W
        self.bins1 = len(e1) - 1
        self.cells = (len(e0) - 1) * self.bins1
        self.grid = np.full(self.cells, 12345, np.uint32)            # never initialised: the first voice clears it
        self.ring = np.full(W or 1, self.cells - 1, np.int32)
        self.pos = 0

    def call(self, v0, v1, flags):
        valid, new = self.vs.scope_voice_spans([self.pos], [len(v0)], [flags], 37)
        if valid[0] != 1:
            return int(valid[0])
        p = 0 if flags & START else self.pos
        if p == 0:
            self.grid[:] = 0
        k0, k1 = self.vs.histogram_bins(v0, self.e0), self.vs.histogram_bins(v1, self.e1)
        cell = np.where((k0 >= 0) & (k1 >= 0), k0 * self.bins1 + k1, -1)
        for j, c in enumerate(cell):
            g = p + j
            if self.W:
                if g >= self.W:
                    old = self.ring[g % self.W]
                    if 0 <= old < self.cells:
                        self.grid[old] -= np.uint32(1)
                self.ring[g % self.W] = c
            if c >= 0:
                self.grid[c] += np.uint32(1)
        self.pos = int(new[0])
        return 1


@pytest.mark.parametrize('W', [37, 37 + 27, 370, None])
def test_ring_model_equals_the_histogram_of_the_window(vs, W):
    M = 37
    rng = np.random.default_rng(5 if W is None else W)
    e0, e1 = np.linspace(-1.0, 1.0, 8), np.array([-1.0, -0.5, 0.1, 0.2, 1.0])        # uneven on the second axis
    model = RingModel(vs, e0, e1, W or 0)
    voice = np.zeros((0, 2))
    ended_once, checked, slid = False, 0, 0
    for call in range(90):
        n = int(rng.choice([0, 1, M - 1, M, int(rng.integers(0, M + 1))]))
        block = rng.normal(0.0, 0.7, (n, 2))                         # some frames fall outside [-1, 1]: the -1 entries
        if n > 2:
            block[0, 0], block[1, 1] = np.nan, np.inf
        flags = 0
        if call == 0 or call == 30:
            flags |= START                                           # 30: a discard-START mid-voice
        if call in (29, 60, 75):
            flags |= END
        if call == 45:
            flags = START | END
        begins = bool(flags & START) or model.pos == 0               # (61: restarted at position 0 without START)
        got = model.call(block[:, 0], block[:, 1], flags)
        if n == 0 and not flags:
            assert got == 0
            continue
        assert got == 1
        voice = np.concatenate([voice[:0] if begins else voice, block])
        lo, hi = vs.scope_voice_window(len(voice), W)
        want = vs.histogram_counts(voice[lo:hi, 0], voice[lo:hi, 1], e0, e1)
        assert np.array_equal(model.grid.reshape(want.shape).astype(np.int64), want), (call, lo, hi)
        checked += 1
        slid += lo > 0
        if flags & END:
            assert model.pos == 0
            ended_once = True
    assert ended_once and checked > 60 and (W is None or W > 200 or slid > 10)
    assert (model.ring == -1).any() or not W                          # dropped frames went through the ring


# ---- the Python refusals that need no device --------------------------------------------------------------------------
def test_constructor_refusals(vs):
    polar, liss = vs.polar_histogram_voice_pool, vs.lissajous_histogram_voice_pool
    ok = polar(4, max_frames_per_call=480, radius_scale=1.0, window_frames=480)
    assert ok.window_frames == 480 and ok.bins == (240, 150) and ok.dtype == np.float32 and ok.polar
    assert polar(4, max_frames_per_call=480, radius_scale=2).window_frames == 0
    with pytest.raises(ValueError, match='below max_frames_per_call'):
        polar(4, max_frames_per_call=480, radius_scale=1.0, window_frames=479)
    with pytest.raises(ValueError, match='below max_frames_per_call'):
        liss(4, max_frames_per_call=480, window_frames=100)
    for bad in (0, -5, 1.5, True):
        with pytest.raises(ValueError, match='window_frames'):
            polar(4, max_frames_per_call=480, radius_scale=1.0, window_frames=bad)
    with pytest.raises(ValueError, match='window_frames'):
        polar(4, max_frames_per_call=480, radius_scale=1.0, window_frames=2 ** 31)
    with pytest.raises(TypeError):
        polar(4, max_frames_per_call=480)                             # radius_scale has no default
    with pytest.raises(ValueError, match='fixed radius_scale'):
        polar(4, max_frames_per_call=480, radius_scale=None)
    for bad in (0, 0.0, -1.0, float('nan'), float('inf'), 1e-60):
        with pytest.raises(ValueError, match='radius_scale'):
            polar(4, max_frames_per_call=480, radius_scale=bad)
    assert polar(4, max_frames_per_call=480, radius_scale=1e-60, dtype='float64').radius_scale == 1e-60
    for bad in ('float16', 'int32', None, 'complex64'):
        with pytest.raises(ValueError, match='dtype'):
            polar(4, max_frames_per_call=480, radius_scale=1.0, dtype=bad)
        with pytest.raises(ValueError, match='dtype'):
            liss(4, max_frames_per_call=480, dtype=bad)
    with pytest.raises(ValueError):
        polar(0, max_frames_per_call=480, radius_scale=1.0)
    with pytest.raises(ValueError):
        polar(65536, max_frames_per_call=480, radius_scale=1.0)
    with pytest.raises(ValueError):
        polar(4, max_frames_per_call=0, radius_scale=1.0)
    with pytest.raises(ValueError, match='counts are int32'):
        polar(4, max_frames_per_call=2 ** 31, radius_scale=1.0)
    with pytest.raises(ValueError, match='one launch'):
        polar(65535, max_frames_per_call=1024 * 129, radius_scale=1.0)        # 129 x 65535 workgroups > 2^23
    with pytest.raises(ValueError, match='one launch'):
        liss(4096, max_frames_per_call=480, bins=4096)                        # 4096 clear workgroups a slot
    with pytest.raises(ValueError):
        polar(4, max_frames_per_call=480, radius_scale=1.0, num_angle_bins=4097)
    with pytest.raises(ValueError, match='ascending'):
        liss(4, max_frames_per_call=480, range=((1.0, -1.0), (-1.0, 1.0)))
    with pytest.raises(ValueError, match='mode'):
        polar(4, max_frames_per_call=480, radius_scale=1.0, mode='XY')
    m = liss(2, max_frames_per_call=64, bins=(16, 8), window_frames=128, dtype='float64')
    assert m.bins == (16, 8) and m.dtype == np.float64 and not m.polar and m.radius_scale is None


def test_dict_form_refusals_come_before_any_device_call(vs, monkeypatch):
    from vndecorrelate_amd import _native
    pool = vs.polar_histogram_voice_pool(3, max_frames_per_call=10, radius_scale=1.0, window_frames=10)

    def no_device(*a, **k):
        raise AssertionError('a refusal reached the device')
    monkeypatch.setattr(_native, 'default_context', no_device)
    monkeypatch.setattr(_native, 'torch_module', no_device)
    block = np.zeros((4, 2), np.float32)
    assert pool.process({}) == {}
    with pytest.raises(ValueError, match='never started'):
        pool.process({0: block})
    with pytest.raises(ValueError, match='outside the pool'):
        pool.process({3: block}, start=[3])
    with pytest.raises(ValueError, match='named twice'):
        pool.process({0: block}, start=[0, 0])
    with pytest.raises(TypeError, match='float32'):
        pool.process({0: block.astype(np.float64)}, start=[0])
    with pytest.raises(ValueError, match='above max_frames_per_call'):
        pool.process({0: np.zeros((11, 2), np.float32)}, start=[0])
    with pytest.raises(ValueError, match='expected'):
        pool.process({0: np.zeros((4, 3), np.float32)}, start=[0])
    with pytest.raises(ValueError, match='never started'):
        pool.process({}, end=[1])
    # mixing the forms: a pool that ran through process_dev() refuses process() until reset()
    pool._form = 'dev'
    with pytest.raises(RuntimeError, match='runs through process_dev'):
        pool.process({0: block}, start=[0])
    pool._form = 'dict'
    with pytest.raises(RuntimeError, match='runs through process\\(\\)'):
        pool.process_dev(None, None, None)


def test_exported_from_the_package(vs):
    import vndecorrelate_amd
    from vndecorrelate_amd import analysis
    names = {'ScopeVoicePool', 'polar_histogram_voice_pool', 'lissajous_histogram_voice_pool', 'scope_voice_spans',
             'scope_voice_window'}
    assert names <= set(analysis.__all__) and names <= set(vs.__all__)
    for name in names:
        assert getattr(vndecorrelate_amd, name) is getattr(analysis, name) is getattr(vs, name)


# ---- header and binding ----------------------------------------------------------------------------------------------
def _declared(header):
    text = re.sub(r'/\*.*?\*/', '', header.read_text(), flags=re.S)
    return sorted(set(re.findall(r'\b(vnd_[a-z0-9_]+)\s*\(', text)))


def test_header_is_plain_c():
    src = ('#include "vnd_scope_voice_stream.h"\n'
           'int main(void){return VND_VOICE_START == 1 && VND_VOICE_END == 2 && VND_SCOPE_MAX_BINS == 4096 ? 0 : 1;}\n')
    r = subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-pedantic', '-fsyntax-only', '-I', str(REPO / 'include'),
                        '-x', 'c', '-'], input=src.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()


def test_every_declared_symbol_is_exported_and_bound(lib):
    from vndecorrelate_amd import _native
    names = _declared(HEADER)
    assert names == NAMES
    for name in names:
        assert hasattr(lib, name), f'{name} declared in vnd_scope_voice_stream.h but not exported'
    assert not set(names) & set(_declared(REPO / 'include' / 'vnd_amd.h'))            # vnd_amd.h keeps its fixed set
    assert not set(names) & set(_native.SCOPE_SIGNATURES)
    text = re.sub(r'/\*.*?\*/', '', HEADER.read_text(), flags=re.S)
    assert '#include "vnd_voice_stream.h"' in text and '#include "vnd_scope.h"' in text
    for wrapper in ('scope_voice_stream_state_bytes', 'scope_voice_stream_reset_device', 'scope_voice_stream_device'):
        assert callable(getattr(_native, wrapper))
    comment = HEADER.read_text()
    assert 'BELONGS TO THE POOL BETWEEN' in comment and 'distinct residues mod W' in comment


def test_checks_that_need_no_device(lib):
    from vndecorrelate_amd import _native
    null = ctypes.c_void_p(None)
    got = ctypes.c_int64(-7)
    assert lib.vnd_scope_voice_stream_state_bytes(4, 480, 0, ctypes.byref(got)) == 0 and got.value == 32
    assert lib.vnd_scope_voice_stream_state_bytes(3, 37, 64, ctypes.byref(got)) == 0
    assert got.value == 32 + 3 * 64 * 4                               # 24 bytes of positions, padded to 32
    assert lib.vnd_scope_voice_stream_state_bytes(3, 37, 37, ctypes.byref(got)) == 0
    assert got.value == 32 + (3 * 37 * 4 + 15) // 16 * 16
    assert _native.scope_voice_stream_state_bytes(3, 37, 37) == got.value
    for args in ((0, 480, 0), (4, 0, 0), (4, 2 ** 31, 0), (-1, 480, 480), (4, 480, -1), (4, 480, 479), (4, 480, 1)):
        assert lib.vnd_scope_voice_stream_state_bytes(*args, ctypes.byref(got)) == INVALID and got.value == 0, args
    for args in ((65536, 480, 0), (4, 480, 2 ** 31), (65535, 1024 * 129, 0)):
        assert lib.vnd_scope_voice_stream_state_bytes(*args, ctypes.byref(got)) == UNSUPPORTED and got.value == 0, args
    assert lib.vnd_scope_voice_stream_state_bytes(4, 480, 0, None) == INVALID
    assert lib.vnd_scope_voice_stream_reset_dev(null, null, 0, 4, 480, 0, null) == INVALID
    for fn in (lib.vnd_polar_hist_voice_stream_f32_dev, lib.vnd_polar_hist_voice_stream_f64_dev):
        assert fn(null, null, 0, 480, 0, null, null, 960, 2, null, null, 1, 1, 1.0, null, 240, null, 150, null, null, 4,
                  null) == INVALID
        assert b'null' in lib.vnd_last_error()
    for fn in (lib.vnd_lissajous_hist_voice_stream_f32_dev, lib.vnd_lissajous_hist_voice_stream_f64_dev):
        assert fn(null, null, 0, 480, 0, null, null, 960, 2, null, null, null, 512, null, 512, null, null, 4, null) == INVALID

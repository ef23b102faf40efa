"""CPU tier of the level-envelope voice pool (include/vnd_polar_level_voice_stream.h; vectorscope.LevelVoicePool): the header
against the library and the binding, the state and work sizes against the layout the header states, a NumPy model of the
rings against _host_levels of the window's frames, and the Python refusals that need no device."""
import ctypes
import pathlib
import re
import subprocess

import numpy as np
import pytest

REPO = pathlib.Path(__file__).resolve().parents[1]
HEADER = REPO / 'include' / 'vnd_polar_level_voice_stream.h'
START, END = 1, 2
INVALID, UNSUPPORTED = 1, 4
NO_SLICE = 0xFFFF
NAMES = sorted(['vnd_polar_level_voice_stream_state_bytes', 'vnd_polar_level_voice_stream_reset_dev',
                'vnd_polar_level_voice_stream_push_f32_dev', 'vnd_polar_level_voice_stream_push_f64_dev',
                'vnd_polar_level_voice_stream_work_bytes', 'vnd_polar_level_voice_stream_levels_f32_dev',
                'vnd_polar_level_voice_stream_levels_f64_dev'])


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


# ---- header and binding ----------------------------------------------------------------------------------------------
def _declared(header):
    text = re.sub(r'/\*.*?\*/', '', header.read_text(), flags=re.S)
    return sorted(set(re.findall(r'\b(vnd_[a-z0-9_]+)\s*\(', text)))


def test_header_is_plain_c():
    src = ('#include "vnd_polar_level_voice_stream.h"\n'
           'int main(void){return VND_VOICE_START == 1 && VND_VOICE_END == 2 && VND_LEVEL_MAX_BINS == 1024 '
           '&& VND_LEVEL_MAX_PERCENTILES == 4 ? 0 : 1;}\n')
    r = subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-pedantic', '-fsyntax-only', '-I', str(REPO / 'include'),
                        '-x', 'c', '-'], input=src.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()


def test_every_declared_symbol_is_exported_and_bound(lib):
    from vndecorrelate_amd import _native
    names = _declared(HEADER)
    assert names == NAMES and len(names) == 7
    for name in names:
        assert hasattr(lib, name), f'{name} declared in vnd_polar_level_voice_stream.h but not exported'
    assert not set(names) & set(_declared(REPO / 'include' / 'vnd_amd.h'))            # vnd_amd.h keeps its fixed set
    assert not set(names) & (set(_native.LEVEL_SIGNATURES) | set(_native.SCOPE_VOICE_STREAM_SIGNATURES))
    text = re.sub(r'/\*.*?\*/', '', HEADER.read_text(), flags=re.S)
    assert '#include "vnd_voice_stream.h"' in text and '#include "vnd_level.h"' in text
    for wrapper in ('level_voice_stream_state_bytes', 'level_voice_stream_reset_device', 'level_voice_stream_push_device',
                    'level_voice_stream_work_bytes', 'level_voice_stream_levels_device'):
        assert callable(getattr(_native, wrapper))
    comment = HEADER.read_text()
    assert 'fill is a prefix length' in comment and 'distinct residues mod W' in comment and 'BYTE FOR BYTE' in comment
    # one translation unit: the new part comes after what it builds on, the window core between the one-shots and the pools
    unit = (REPO / 'vndecorrelate_amd' / 'csrc' / 'vnd_amd.hip').read_text()
    order = [unit.index(f'#include "{n}"') for n in ('vnd_voice_stream.hpp', 'vnd_scope.hpp', 'vnd_level.hpp', 'vnd_voice_window.hpp',
                                                     'vnd_scope_voice_stream.hpp', 'vnd_level_voice_stream.hpp')]
    assert order == sorted(order) and unit.count('#include "vnd_voice_window.hpp"') == 1


def test_the_frame_body_is_stated_once():
    """The key and the slice of a frame: one device function, called by the one-shot's stage kernel and by the push."""
    csrc = REPO / 'vndecorrelate_amd' / 'csrc'
    level, voice = (csrc / 'vnd_level.hpp').read_text(), (csrc / 'vnd_level_voice_stream.hpp').read_text()
    assert level.count('int level_frame(') == 1 and level.count('level_frame(l, r,') == 1
    assert voice.count('level_frame(l, r,') == 1 and 'degrees(' not in voice and 'scope_bin(' not in voice
    assert level.count('K::degrees(') == 1                             # ... and nowhere else in the one-shot's file
    # the select over staged keys: one host helper, both callers
    assert level.count('level_run_select(') == 2 and voice.count('level_run_select(a,') == 1
    assert 'level_select_kernel' not in voice and 'voice_head' not in voice and 'scope_voice_span(' in voice


def test_the_ring_walk_is_stated_once():
    """The slot rule, the walk of a workgroup and its ring entry with the one wrap: vnd_voice_window.hpp, called by both
    pools' kernels; the level pool loads the chunk's frame with the one-shot's scope_load."""
    csrc = REPO / 'vndecorrelate_amd' / 'csrc'
    core = (csrc / 'vnd_voice_window.hpp').read_text()
    pools = [(csrc / name).read_text() for name in ('vnd_scope_voice_stream.hpp', 'vnd_level_voice_stream.hpp')]
    assert core.count('slot -= W') == 1 and core.count('-= W') == 1 and core.count('% W') == 1
    assert core.count('ScopeVoiceSpan scope_voice_span(') == 1 and core.count('struct VoiceWindowWalk') == 1
    assert core.count('kScopeVoiceSpan = 1024') == 1 and core.count('kScopeVoiceThreads = 256') == 1
    assert core.count('distinct residues mod W') == 1 and core.count('vnd_status voice_window_plan(') == 1
    assert core.count('vnd_status voice_window_scale(') == 1
    assert pools[1].count('scope_load(a.s, pl, pr, j, l, r)') == 1 and 'a.s.packed' not in pools[1] and 'if (a.packed)' not in pools[1]
    assert pools[0].count('if (a.packed) {') == 1          # (the scope pool keeps its own packed load: its file says why)
    for text in pools:
        assert '-= a.W' not in text and '-= W' not in text and '% a.W' not in text and '% W' not in text
        assert text.count('VoiceWindowWalk w;') == 1 and text.count('w.open(a.pos, a.counts, a.flags, a.M, b, blockIdx.x)') == 1
        assert text.count('w.entry(j)') == 1
        assert 'distinct residues' not in text and 'vnd_voice_window.hpp' in text
        assert text.count('voice_window_plan(') == 1 and 'radius_scale is NaN' not in text and 'scope_overlap(' not in text
        assert text.count('voice_window_scale<T>(radius_scale)') == 1 and 'scope_clash(outs,' in text
    scope = (csrc / 'vnd_scope.hpp').read_text()
    assert scope.count('static int scope_clash(') == 1 and scope.count('scope_clash(outs,') == 2


# ---- the sizes -------------------------------------------------------------------------------------------------------
def pad16(v):
    return (v + 15) // 16 * 16


def align8(v):
    return (v + 7) // 8 * 8


def state_bytes(S, W, is64):
    """positions int64 [S], fill int32 [S], keys [S][W] (4 or 8 bytes), bins uint16 [S][W]; each padded to 16 bytes."""
    return pad16(8 * S) + pad16(4 * S) + pad16(S * W * (8 if is64 else 4)) + pad16(S * W * 2)


def digit_bits(vs, W, bins, P, key_bytes):
    """the widest digit whose counters and prefixes of one signal fit the LDS budget, and no more than 8
    counters a signal for each frame a workgroup brings."""
    cells, frames, d = bins * P, min(W, vs.LEVEL_SPAN_FRAMES), 1
    while d < 8 and cells * ((4 << (d + 1)) + key_bytes) <= vs.LDS_BYTES and (cells << (d + 1)) <= 8 * frames:
        d += 1
    return d


def work_bytes(vs, S, W, bins, P, is64):
    """The select's cell state - prefix, next, gamma (8 bytes a cell each), rank, flags (uint32) - and the digit histograms."""
    cells = S * bins * P
    return 3 * 8 * cells + 2 * align8(4 * cells) + align8((cells << digit_bits(vs, W, bins, P, 8 if is64 else 4)) * 4)


def test_state_and_work_bytes_against_the_stated_layout(lib, vs):
    from vndecorrelate_amd import _native
    got = ctypes.c_int64(-7)
    for S, M, W in ((4, 1, 64), (4, 23, 67), (3, 37, 37), (1, 1, 1), (5, 480, 48000), (2, 7, vs.LEVEL_SPAN_FRAMES + 5)):
        for is64 in (0, 1):
            assert lib.vnd_polar_level_voice_stream_state_bytes(S, M, W, is64, ctypes.byref(got)) == 0
            assert got.value == state_bytes(S, W, is64) == _native.level_voice_stream_state_bytes(S, M, W, bool(is64)), (S, M, W)
            for bins, P in ((8, 2), (360, 2), (360, 4), (1, 1), (1024, 4), (7, 3)):
                assert lib.vnd_polar_level_voice_stream_work_bytes(S, W, bins, P, is64, ctypes.byref(got)) == 0
                assert got.value == work_bytes(vs, S, W, bins, P, is64), (S, W, bins, P, is64)
                assert got.value == _native.level_voice_stream_work_bytes(S, W, bins, P, bool(is64))
                # the one-shot's work memory is this, behind the per-signal maxima, plus the staged keys and slices
                one_shot = _native.polar_level_work_bytes(S, W, bins, P, bool(is64))
                assert one_shot == 8 * S + got.value + align8(S * W * (8 if is64 else 4)) + align8(S * W * 2)
    assert state_bytes(3, 64, 0) == 32 + 16 + 768 + 384


def test_checks_that_need_no_device(lib):
    null = ctypes.c_void_p(None)
    got = ctypes.c_int64(-7)
    state = lib.vnd_polar_level_voice_stream_state_bytes
    for args in ((0, 480, 480), (4, 0, 480), (4, 2 ** 31, 2 ** 31), (-1, 480, 480), (4, 480, 479), (4, 480, 0), (4, 480, -1)):
        assert state(*args, 0, ctypes.byref(got)) == INVALID and got.value == 0, args
    for args in ((65536, 480, 480), (4, 480, 2 ** 31), (65535, 1024 * 129, 1024 * 129)):
        assert state(*args, 0, ctypes.byref(got)) == UNSUPPORTED and got.value == 0, args
    assert state(4, 480, 480, 0, None) == INVALID
    work = lib.vnd_polar_level_voice_stream_work_bytes
    for args in ((0, 64, 8, 2), (4, 0, 8, 2), (4, 64, 0, 2), (4, 64, 8, 0)):
        assert work(*args, 0, ctypes.byref(got)) == INVALID and got.value == 0, args
    for args in ((65536, 64, 8, 2), (4, 2 ** 31, 8, 2), (4, 64, 1025, 2), (4, 64, 8, 5), (65535, 32768 * 129, 8, 2)):
        assert work(*args, 0, ctypes.byref(got)) == UNSUPPORTED and got.value == 0, args
    assert work(4, 64, 8, 2, 0, None) == INVALID
    assert lib.vnd_polar_level_voice_stream_reset_dev(null, null, 0, 4, 480, 480, 0, null) == INVALID
    ps = (ctypes.c_double * 2)(95.0, 50.0)
    for fn in (lib.vnd_polar_level_voice_stream_push_f32_dev, lib.vnd_polar_level_voice_stream_push_f64_dev):
        assert fn(null, null, 0, 480, 480, null, null, 960, 2, null, null, 1, 1, 1.0, null, 360, null, 4, null) == INVALID
        assert b'null' in lib.vnd_last_error()
    for fn in (lib.vnd_polar_level_voice_stream_levels_f32_dev, lib.vnd_polar_level_voice_stream_levels_f64_dev):
        assert fn(null, null, 0, 480, 480, 360, ps, 2, null, null, null, 0, 4, null) == INVALID
        assert b'null' in lib.vnd_last_error()


# ---- the rings, modelled ---------------------------------------------------------------------------------------------
class RingModel:
    """One slot of the device's rule in NumPy: the ring of keys (the radii: their order is the order of their bit patterns)
    and the ring of slices, pre-filled with a valid slice and a key above every real one and never cleared, the position and
    the fill."""

    def __init__(self, vs, edges, W, M, scale):
        self.vs, self.edges, self.W, self.M, self.scale = vs, edges, W, M, scale
        self.keys = np.full(W, 3e38, np.float32)
        self.bins = np.zeros(W, np.uint16)
        self.pos = self.fill = 0

    def call(self, block, flags):
        from vndecorrelate_amd.utils.dsp import LayoutMode, polar_coordinates
        valid, new = self.vs.scope_voice_spans([self.pos], [len(block)], [flags], self.M)
        if valid[0] != 1:
            return int(valid[0])
        p, n, bins = (0 if flags & START else self.pos), len(block), len(self.edges) - 1
        radii, thetas = polar_coordinates(block[:, 0], block[:, 1], LayoutMode.MS, True, False, compute_weights=False)
        radii = radii / radii.dtype.type(self.scale)
        degrees = np.degrees(thetas)
        for j in range(n):
            k = int(np.searchsorted(self.edges, degrees[j], side='right')) - 1       # edges[k] <= deg < edges[k + 1]
            inside = 0 <= k < bins and self.edges[k] <= degrees[j] < self.edges[k + 1]
            self.keys[(p + j) % self.W] = radii[j]
            self.bins[(p + j) % self.W] = k if inside else NO_SLICE
        self.fill = min(p + n, self.W)
        self.pos = int(new[0])
        return 1

    def levels(self, ps):
        """What the levels entry computes: the select over ring entries [0, fill), in whatever order they lie."""
        bins = len(self.edges) - 1
        keys, slices = self.keys[:self.fill], self.bins[:self.fill]
        levels, counts = np.zeros((len(ps), bins)), np.zeros(bins, np.int64)
        for k in range(bins):
            inside = keys[slices == k]
            counts[k] = len(inside)
            for i, p in enumerate(ps):
                if len(inside):
                    levels[i, k] = np.percentile(inside, p)
        return levels, counts


@pytest.mark.parametrize('W', [37, 37 + 27, 370])
def test_ring_model_equals_the_levels_of_the_window(vs, W):
    M, scale, ps = 37, 1.5, [0.0, 37.5, 50.0, 95.0, 100.0]
    rng = np.random.default_rng(W)
    edges, _ = vs.level_edges(8)
    model = RingModel(vs, edges, W, M, scale)
    assert model.levels(ps)[1].sum() == 0                                # never started: no frame
    voice = np.zeros((0, 2), np.float32)
    ended_once, checked, slid, dropped = False, 0, 0, 0
    for call in range(90):
        n = int(rng.choice([0, 1, M - 1, M, int(rng.integers(0, M + 1))]))
        block = rng.normal(0.0, 0.5, (n, 2)).astype(np.float32)
        if n > 2:
            block[0] = (0.25, -0.25)                                     # exactly +90 degrees: the last edge, no slice
            block[1] = (0.5, 0.5)                                        # mono: 0 degrees, an inner edge
        flags = 0
        if call == 0 or call == 30:
            flags |= START                                               # 30: a discard-START mid-voice
        if call in (29, 60, 75):
            flags |= END
        if call == 45:
            flags = START | END
        if call == 50:
            flags, block = START, block[:5]                              # a short voice over a full ring
        begins = bool(flags & START) or model.pos == 0                   # (61: restarted at position 0 without START)
        got = model.call(block, flags)
        if len(block) == 0 and not flags:
            assert got == 0
            continue
        assert got == 1
        voice = np.concatenate([voice[:0] if begins else voice, block])
        lo, hi = vs.scope_voice_window(len(voice), W)
        assert model.fill == hi - lo
        levels, counts = model.levels(ps)
        if hi > lo:
            want, want_counts = vs._host_levels(voice[lo:hi, 0], voice[lo:hi, 1], edges, ps, True, True, scale)
        else:
            want, want_counts = np.zeros_like(levels), np.zeros_like(counts)
        assert np.array_equal(counts, want_counts), (call, lo, hi)
        assert levels.tobytes() == want.tobytes(), (call, lo, hi)        # exact on the host: no tolerance
        dropped += hi - lo - int(counts.sum())
        checked += 1
        slid += lo > 0
        if flags & END:
            assert model.pos == 0 and model.fill == hi - lo              # END keeps the ring and its fill
            ended_once = True
    assert ended_once and checked > 60 and dropped > 10 and (W > 200 or slid > 10)
    assert (model.bins == NO_SLICE).any()


# ---- the Python refusals that need no device --------------------------------------------------------------------------
def test_constructor_refusals(vs):
    level = vs.polar_level_voice_pool
    ok = level(4, max_frames_per_call=480, window_frames=48000, radius_scale=1.0)
    assert ok.window_frames == 48000 and ok.num_bins == 360 and ok.percentiles == (95.0, 50.0) and ok.dtype == np.float32
    assert ok.ms and ok.semicircular and isinstance(ok, vs.LevelVoicePool)
    edges, centers = vs.level_edges(360)
    assert np.array_equal(ok.bin_edges, edges) and np.array_equal(ok.bin_centers, centers)
    with pytest.raises(TypeError):
        level(4, max_frames_per_call=480, radius_scale=1.0)                          # window_frames has no default
    with pytest.raises(TypeError):
        level(4, max_frames_per_call=480, window_frames=480)                         # nor has radius_scale
    with pytest.raises(ValueError, match='below max_frames_per_call'):
        level(4, max_frames_per_call=480, window_frames=479, radius_scale=1.0)
    for bad in (0, -5, 1.5, True, None):
        with pytest.raises(ValueError, match='window_frames'):
            level(4, max_frames_per_call=1, window_frames=bad, radius_scale=1.0)
    with pytest.raises(ValueError, match='window_frames'):
        level(4, max_frames_per_call=480, window_frames=2 ** 31, radius_scale=1.0)
    with pytest.raises(ValueError, match='fixed radius_scale'):
        level(4, max_frames_per_call=480, window_frames=480, radius_scale=None)
    for bad in (0, 0.0, -1.0, float('nan'), float('inf'), 1e-60):
        with pytest.raises(ValueError, match='radius_scale'):
            level(4, max_frames_per_call=480, window_frames=480, radius_scale=bad)
    assert level(4, max_frames_per_call=480, window_frames=480, radius_scale=1e-60, dtype='float64').radius_scale == 1e-60
    for bad in ('float16', 'int32', None, 'complex64'):
        with pytest.raises(ValueError, match='dtype'):
            level(4, max_frames_per_call=480, window_frames=480, radius_scale=1.0, dtype=bad)
    with pytest.raises(ValueError):
        level(0, max_frames_per_call=480, window_frames=480, radius_scale=1.0)
    with pytest.raises(ValueError):
        level(65536, max_frames_per_call=480, window_frames=480, radius_scale=1.0)
    with pytest.raises(ValueError):
        level(4, max_frames_per_call=0, window_frames=480, radius_scale=1.0)
    with pytest.raises(ValueError, match='counts are int32'):
        level(4, max_frames_per_call=2 ** 31, window_frames=2 ** 31, radius_scale=1.0)
    with pytest.raises(ValueError, match='one launch'):
        level(65535, max_frames_per_call=1024 * 129, window_frames=1024 * 129, radius_scale=1.0)
    with pytest.raises(ValueError, match='one launch'):
        level(65535, max_frames_per_call=480, window_frames=32768 * 129, radius_scale=1.0)
    with pytest.raises(ValueError, match='slices'):
        level(4, max_frames_per_call=480, window_frames=480, radius_scale=1.0, num_bins=1025)
    assert level(4, max_frames_per_call=480, window_frames=480, radius_scale=1.0, num_bins=1024).num_bins == 1024
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError, match='num_bins'):
            level(4, max_frames_per_call=480, window_frames=480, radius_scale=1.0, num_bins=bad)
    with pytest.raises(ValueError, match='percentiles'):
        level(4, max_frames_per_call=480, window_frames=480, radius_scale=1.0, percentiles=(1, 2, 3, 4, 5))
    with pytest.raises(ValueError, match='percentiles'):
        level(4, max_frames_per_call=480, window_frames=480, radius_scale=1.0, percentiles=())
    for bad in ((101.0,), (-0.5, 50.0), (float('nan'),)):
        with pytest.raises(ValueError, match='Percentiles'):
            level(4, max_frames_per_call=480, window_frames=480, radius_scale=1.0, percentiles=bad)
    with pytest.raises(ValueError, match='mode'):
        level(4, max_frames_per_call=480, window_frames=480, radius_scale=1.0, mode='XY')
    m = level(2, max_frames_per_call=64, window_frames=128, radius_scale=2, num_bins=8, percentiles=(0, 37.5, 50, 100),
              dtype='float64', mode='LR', semicircular=False)
    assert m.num_bins == 8 and m.dtype == np.float64 and m.percentiles == (0.0, 37.5, 50.0, 100.0) and not m.ms


def test_refusals_come_before_any_device_call(vs, monkeypatch):
    from vndecorrelate_amd import _native
    pool = vs.polar_level_voice_pool(3, max_frames_per_call=10, window_frames=10, radius_scale=1.0, num_bins=8)

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
    with pytest.raises(ValueError, match='device tensor'):
        pool.process_dev(block, None, None)
    pool._form = 'dev'
    with pytest.raises(RuntimeError, match='runs through process_dev'):
        pool.process({0: block}, start=[0])
    pool._form = 'dict'
    with pytest.raises(RuntimeError, match='runs through process\\(\\)'):
        pool.process_dev(None, None, None)


def test_exported_from_the_package(vs):
    import vndecorrelate_amd
    from vndecorrelate_amd import analysis
    names = {'LevelVoicePool', 'polar_level_voice_pool'}
    assert names <= set(analysis.__all__) and names <= set(vs.__all__)
    for name in names:
        assert getattr(vndecorrelate_amd, name) is getattr(analysis, name) is getattr(vs, name)

"""CPU tier of the cross-correlogram: the host path against the reference's fixtures (sha256), the reference's
exceptions, the routing rule, the analysis header, and the behaviour without a device."""
import hashlib
import json
import pathlib
import re
import subprocess

import numpy as np
import pytest

REPO = pathlib.Path(__file__).resolve().parents[1]
GOLDEN = REPO / 'tests' / 'golden'
ANALYSIS_H = REPO / 'include' / 'vnd_analysis.h'


def sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def fixture_inputs(case, g):
    """A fixture case's (x, y), rebuilt from its manifest recipe by the generator's own function."""
    import importlib.util
    spec = importlib.util.spec_from_file_location('gen_correlogram_golden', REPO / 'tools' / 'gen_correlogram_golden.py')
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen.fixture_inputs(case['input'], g)


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN / 'correlogram.npz'), json.loads((GOLDEN / 'correlogram_manifest.json').read_text())


@pytest.fixture
def host_only():
    from vndecorrelate_amd import analysis
    analysis.set_correlogram_device(False)
    yield analysis
    analysis.set_correlogram_device(None)


def test_host_path_matches_every_fixture(golden, host_only):
    from vndecorrelate_amd.utils.dsp import cross_correlogram
    g, manifest = golden
    assert len(manifest['cases']) >= 10
    for name, case in manifest['cases'].items():
        got = cross_correlogram(*fixture_inputs(case, g), **case['kwargs'])
        assert got.dtype == np.float32 and list(got.shape) == case['shape'], name
        assert sha(got) == case['sha256'] == sha(g[name + '__out']), name


def test_host_helpers_match_the_reference(golden):
    from vndecorrelate_amd.utils import dsp
    g, manifest = golden
    got = {
        'sine_sweep': dsp.sine_sweep(20, 20000, 0.1, 44100),
        'sine_sweep_48k': dsp.sine_sweep(100.0, 1000.0, 0.1, 48000),
        'exponential_decay': np.array([dsp.exponential_decay(t) for t in (0.0, 0.1, 0.37, 1.0, 2.5)]
                                      + [dsp.exponential_decay(0.3, k=5.5)]),
        'generate_decay_envelope': np.array(dsp.generate_decay_envelope(8, 0.3)),
        'generate_decay_envelope_1': np.array(dsp.generate_decay_envelope(1, 0.0)),
        'radians_to_degrees': dsp.radians_to_degrees(np.linspace(-4, 4, 41)),
    }
    got['polar_to_cartesian_x'], got['polar_to_cartesian_y'] = dsp.polar_to_cartesian(
        np.linspace(-180, 180, 37), np.random.default_rng(18).uniform(0, 1, 37))
    for k, v in got.items():
        assert str(v.dtype) == manifest['helpers'][k]['dtype'], k
        assert sha(v) == manifest['helpers'][k]['sha256'], k
    assert dsp.sine_sweep(20, 8000, 1.0, 16000).dtype == np.float32
    assert isinstance(dsp.generate_decay_envelope(4, 0.5), tuple)


def test_reference_exceptions(host_only):
    from vndecorrelate_amd.utils.dsp import cross_correlogram
    x = np.zeros(1000, np.float32)
    with pytest.raises(ValueError):
        cross_correlogram(np.zeros((1000, 2)), x)                     # check_mono(x)
    with pytest.raises(ValueError):
        cross_correlogram(x, np.zeros((1000, 2)))                     # check_mono(y)
    with pytest.raises(ValueError):
        cross_correlogram(x, np.zeros(999))                           # check_equal_length
    with pytest.raises(ZeroDivisionError):
        cross_correlogram(x, x, stride_seconds=0.0)
    with pytest.raises(ValueError):
        cross_correlogram(x, x, window_size_seconds=0.0)
    with pytest.raises(ValueError):
        cross_correlogram(x, x, max_lag_seconds=-0.01)                # a negative column count


@pytest.mark.parametrize('device', [None, True])
def test_uncovered_calls_keep_numpy_exceptions(device):
    """The routing refuses these before anything needs a device, so the NumPy exceptions come first even under True."""
    from vndecorrelate_amd import analysis
    from vndecorrelate_amd.utils.dsp import cross_correlogram
    x = np.zeros(1000, np.float32)
    analysis.set_correlogram_device(device)
    try:
        with pytest.raises(ZeroDivisionError):
            cross_correlogram(x, x, stride_seconds=0.0)
        with pytest.raises(ValueError):
            cross_correlogram(x, x, window_size_seconds=0.0)
    finally:
        analysis.set_correlogram_device(None)


def test_routing_rule():
    from vndecorrelate_amd.analysis import MAX_WINDOW, correlogram_covers as covers
    assert MAX_WINDOW == 16384
    assert covers(441000, 882, 441, 1765, 1e-10)
    assert covers(0, 882, 441, 1765, 1e-10)                          # no windows: an empty result
    assert covers(100, 1, 1, 1, 1e-10) and covers(10 ** 6, MAX_WINDOW, 1, 2 ** 31 - 1, 0.0)
    assert covers(1000, 10, 5, 21, 0) and covers(1000, 10, 5, 21, 1)
    assert not covers(1000, 0, 5, 21, 1e-10)                         # window 0: ValueError in NumPy
    assert not covers(1000, -3, 5, 21, 1e-10)
    assert not covers(1000, MAX_WINDOW + 1, 5, 21, 1e-10)            # above the cap
    assert not covers(1000, 10, 0, 21, 1e-10)                        # hop 0: ZeroDivisionError
    assert not covers(1000, 10, -1, 21, 1e-10)
    assert not covers(1000, 10, 5, -1, 1e-10)                        # negative column count: ValueError
    assert not covers(1000, 10, 5, 2 ** 31 + 1, 1e-10)
    assert not covers(1000, 10, 5, 21, np.float64(1e-10))            # a NumPy scalar changes the promotion
    assert not covers(1000, 10, 5, 21, np.float32(1e-10))
    assert not covers(1000, 10, 5, 21, 1e40)                         # not a finite float32
    assert not covers(1000, 10, 5, 21, float('nan'))
    assert not covers(1000, 10, 5, 21, 2 ** 30)
    assert not covers(1000, 10, 5, 21, True)
    assert not covers(1000, 10.0, 5, 21, 1e-10)


def test_set_correlogram_device_checks_its_argument():
    import vndecorrelate_amd
    from vndecorrelate_amd import analysis
    assert vndecorrelate_amd.set_correlogram_device is analysis.set_correlogram_device
    for bad in ('yes', 1, 0, 2.0):
        with pytest.raises(TypeError):
            analysis.set_correlogram_device(bad)
    analysis.set_correlogram_device(np.bool_(False))
    analysis.set_correlogram_device(None)


def test_dsp_imports_without_the_native_binding():
    """utils/dsp.py reaches the device code only inside cross_correlogram: no module-level import of it."""
    import ast
    tree = ast.parse((REPO / 'vndecorrelate_amd' / 'utils' / 'dsp.py').read_text())
    for node in tree.body:
        if isinstance(node, (ast.Import, ast.ImportFrom)):
            names = [a.name for a in node.names] + [getattr(node, 'module', None) or '']
            assert not any('_native' in n or 'analysis' in n for n in names), ast.dump(node)


def declared(header):
    text = re.sub(r'/\*.*?\*/', '', header.read_text(), flags=re.S)
    return sorted(set(re.findall(r'\b(vnd_[a-z0-9_]+)\s*\(', text)))


def test_analysis_header_is_plain_c_and_bound():
    src = ('#include "vnd_analysis.h"\nint main(void){vnd_status (*f)(vnd_ctx *, const float *, const float *, float *,'
           ' int64_t, int64_t, int64_t, int32_t, int32_t, int32_t, int32_t, float, void *) = vnd_correlogram_f32_dev;'
           ' return f == 0 && VND_CORRELOGRAM_MAX_WINDOW == 16384;}\n')
    r = subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-fsyntax-only', '-I', str(REPO / 'include'), '-x', 'c',
                        '-'], input=src.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    import __graft_entry__ as entry
    entry.build()
    from vndecorrelate_amd import _native
    lib = _native.load_library()
    names = declared(ANALYSIS_H)
    assert names == ['vnd_correlogram_f32_dev']
    for name in names:
        assert hasattr(lib, name), f'{name} declared in vnd_analysis.h but not exported'
    assert not set(names) & set(declared(REPO / 'include' / 'vnd_amd.h'))
    assert not set(names) & set(_native.SIGNATURES)
    assert _native.CORRELOGRAM_MAX_WINDOW == 16384


def test_without_a_device_numpy_answers_and_true_raises():
    from vndecorrelate_amd import _native, analysis
    from vndecorrelate_amd.utils.dsp import _correlogram_numpy, cross_correlogram
    if _native.device_count() > 0:
        pytest.skip('a GPU is present')
    rng = np.random.default_rng(1)
    x = rng.uniform(-1, 1, 5000).astype(np.float32)
    y = rng.uniform(-1, 1, 5000).astype(np.float32)
    got = cross_correlogram(x, y)
    assert np.array_equal(got, _correlogram_numpy(x, y, 882, 441, 882, 1e-10))
    st = np.stack([x, y], axis=1)[None].repeat(2, axis=0)
    batched = analysis.cross_correlogram_batched(st)
    # the per-stream loop over the channel views (NumPy's float32 dot follows the memory layout)
    assert batched.shape == (2,) + got.shape and np.array_equal(batched[1], cross_correlogram(st[1, :, 0], st[1, :, 1]))
    assert np.abs(batched[1].astype(np.float64) - got).max() <= 1e-6
    assert np.array_equal(analysis.cross_correlogram_batched(st[:, :, 0], st[:, :, 1]), batched)
    analysis.set_correlogram_device(True)
    try:
        with pytest.raises(RuntimeError):
            cross_correlogram(x, y)
        with pytest.raises(RuntimeError):
            analysis.cross_correlogram_batched(st)
    finally:
        analysis.set_correlogram_device(None)


def test_batched_shapes_are_checked():
    from vndecorrelate_amd import analysis
    with pytest.raises(ValueError):
        analysis.cross_correlogram_batched(np.zeros((2, 100, 3), np.float32))
    with pytest.raises(ValueError):
        analysis.cross_correlogram_batched(np.zeros((2, 100), np.float32))
    with pytest.raises(ValueError):
        analysis.cross_correlogram_batched(np.zeros((2, 100), np.float32), np.zeros((2, 99), np.float32))
    empty = analysis.cross_correlogram_batched(np.zeros((0, 2000, 2), np.float32))
    assert empty.shape == (0, 3, 1765) and empty.dtype == np.float32

"""CPU tier: what every plain wrapper of ``_native.py`` hands to the C ABI, argument by argument.

``tests/golden/native_calls.json`` holds the calls of an earlier commit's wrappers against a stand-in for the library that
records ``(function name, argument values)`` and returns 0 (``tools/gen_native_calls_golden.py``: distinct sentinel
arguments, every flag both ways, ``width`` absent and present, both fan-out names).  The wrappers of this tree must make the
same calls: two arguments of one type swapped inside a wrapper, a flag dropped or the wrong ``_f32_`` / ``_f64_`` name show
here, without a GPU.  The fixture is generated from another checkout, never from this tree."""
import importlib.util
import json
import pathlib

import pytest

REPO = pathlib.Path(__file__).resolve().parents[1]
FIXTURE = json.loads((REPO / 'tests' / 'golden' / 'native_calls.json').read_text())


def _generator():
    spec = importlib.util.spec_from_file_location('gen_native_calls_golden', REPO / 'tools' / 'gen_native_calls_golden.py')
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


GEN = _generator()


@pytest.fixture(scope='module')
def native():
    from vndecorrelate_amd import _native
    return _native


@pytest.fixture(scope='module')
def recorded(native):
    return GEN.record(native)


def test_the_fixture_says_where_it_came_from():
    header = FIXTURE['header']
    assert header['generated_by'] == 'tools/gen_native_calls_golden.py'
    assert len(header['recorded_commit']) == 40 and 'never from the code under test' in header['note']
    assert header['wrappers'] == len(FIXTURE['wrappers']) >= 70
    assert header['runs'] == sum(len(runs) for runs in FIXTURE['wrappers'].values())


def test_no_wrapper_is_skipped_silently(native, recorded):
    """Every public function and method of the binding is in the record or listed, with the reason, as left out."""
    functions, table_methods, context_methods = GEN.recorded_names(native)
    names = functions + [f'TapTable.{m}' for m in table_methods] + [f'Context.{m}' for m in context_methods]
    assert sorted(names) == sorted(FIXTURE['wrappers']) == sorted(recorded)
    assert not set(names) & set(GEN.NOT_RECORDED)
    assert sorted(set(names) | set(GEN.NOT_RECORDED)) == GEN.public_callables(native)
    for name in names:                                   # by the rule of the issue, none of these may be left out
        plain = name.split('.')[-1]
        assert (plain.endswith('_device') or plain.endswith('_bytes') or plain.startswith('describe') or 'device' in plain
                or plain in ('scope_route', 'spectrum_run_length', 'prepare', 'set_variant', 'time_copy')), name
    for name in GEN.NOT_RECORDED:
        assert not name.endswith('_device') and not name.startswith('describe_'), name


def test_the_sentinels_tell_the_arguments_apart():
    """Within one call no two numeric arguments are equal, except the 0 / 1 of flags and a repeated buffer length."""
    for name, runs in FIXTURE['wrappers'].items():
        for run in runs:
            for function, args in run['calls']:
                numbers = [a for a in args if isinstance(a, (int, float)) and not isinstance(a, bool) and a not in (0, 1, 512)]
                assert len(numbers) == len(set(numbers)), (name, function, args)


@pytest.mark.parametrize('name', sorted(FIXTURE['wrappers']))
def test_wrapper_makes_the_recorded_calls(name, recorded):
    want, got = FIXTURE['wrappers'][name], recorded[name]
    assert len(got) == len(want), f'{name}: {len(got)} runs, the fixture has {len(want)}'
    for w, g in zip(want, got):
        assert g['args'] == w['args'], f'{name}: the generator no longer draws the recorded arguments'
        assert g['calls'] == w['calls'], f'{name}({w["args"]})'
        assert g['returns'] == w['returns'], f'{name}({w["args"]})'


def test_a_swap_would_show(native):
    """The check has teeth: a wrapper that swaps two addresses makes another call than the recorded one."""
    lib = GEN.RecordingLibrary(native)
    ctx = GEN.Handle(lib, GEN.CTX_HANDLE)
    run = FIXTURE['wrappers']['haas_device'][0]
    native.haas_device(ctx, **run['args'])
    assert lib.calls == run['calls']
    lib.calls = []
    native.haas_device(ctx, **{**run['args'], 'x_ptr': run['args']['y_ptr'], 'y_ptr': run['args']['x_ptr']})
    assert lib.calls and lib.calls != run['calls']


def test_an_address_that_is_no_integer_is_refused_before_the_call(native):
    import ctypes
    lib = GEN.RecordingLibrary(native)
    with pytest.raises((TypeError, ctypes.ArgumentError)):
        native.haas_device(GEN.Handle(lib, GEN.CTX_HANDLE), 'address', 1032, 1, 2, 2, delay=3, delayed_channel=1,
                           ms_mode=True, width=None)
    assert not lib.calls

#!/usr/bin/env python3
"""Write tests/golden/native_calls.json: what every plain wrapper of ``_native.py`` hands to the C ABI.

Usage:  python tools/gen_native_calls_golden.py <checkout of the commit to record>

The checkout is another tree than this one - the parent of a change to the binding, or any commit whose GPU suite passed -
and its commit goes into the fixture's header.  Never point it at the code under test: the fixture is what
``tests/test_native_marshalling_cpu.py`` holds the working tree's ``_native.py`` to, argument by argument.  No GPU and no
built library are needed: the library is replaced by a stand-in that records every call.

What is recorded.  Every wrapper whose parameters are plain numbers, flags and addresses (``recorded_names`` finds them by
name: the ``*_device``, ``*_bytes`` and ``describe_*`` functions, ``scope_route``, ``spectrum_run_length``, the ``TapTable``
device, prepare and describe methods and ``Context``'s two) is called with a distinct integer per parameter, 1000 + 16 i
for the i-th, and a distinct float 0.25 + i where the annotation says ``float``.  The runs of one wrapper are the product of

* its ``bool`` parameters all true, all false and, where it has several, each one alone true;
* ``width`` as ``None`` and as 0.5;
* for the ``TapTable`` methods, ``channels`` equal to the table's count and not (the plain and the fan-out entry).

``percentiles`` is ``(5.0, 50.0)``.  A record holds the C functions called, each argument as the C function receives it
(converted through the function's ``argtypes`` entry: an out-parameter is ``"out"``, a buffer its length, a ctypes array a
list, a null pointer 0) and what the wrapper returned.  The stand-in writes 4000 + 16 i + j into out-parameter j of the
i-th call, and ``launch <n>`` into the buffer of the n-th describe call, so the return value shows which one came back.

The array-taking host wrappers and the two kernel-source calls are not recorded: ``NOT_RECORDED`` says why, name by name.
"""
from __future__ import annotations

import ctypes
import importlib.util
import inspect
import itertools
import json
import pathlib
import subprocess
import sys

REPO = pathlib.Path(__file__).resolve().parents[1]
OUT = REPO / 'tests' / 'golden' / 'native_calls.json'
CTX_HANDLE, BANK_HANDLE, TABLE_HANDLE, TABLE_CHANNELS = 0x7000, 0x7100, 0x7200, 6

_HOST = 'takes NumPy arrays: its checks stay as written, the GPU suite compares what it computes'
NOT_RECORDED = {
    **{name: _HOST for name in (
        'convolve_promote_host', 'haas_host', 'haas_scan_host', 'haas_pairs_host', 'velvet_pairs_host', 'convolve_each_host',
        'decorrelate_each_host', 'haas_each_host', 'each_stream_host', 'voice_stream_host', 'haas_voice_stream_host',
        'haas_each_stream_host', 'host_buffers_mapped', 'TapTable.convolve_host', 'TapTable.decorrelate_host',
        'TapTable.scan_host', 'TapTable.create', 'TapTable.from_bytes', 'TapTable.to_bytes', 'TapTable.read_stamps')},
    'spec_kernel_source': 'a kernel-source call: tap arrays in, text out (tests/test_spec_cpu.py runs it for real)',
    'window_kernel_source': 'a kernel-source call: tap arrays in, text out (tests/test_spec_cpu.py runs it for real)',
    'load_library': 'opens the library', 'shard_range': 'two out-parameters, run for real by the CPU tests',
    'device_count': 'ignores the status by design, run for real by the CPU tests',
    'context_for': 'makes a Context', 'default_context': 'makes a Context', 'is_torch': 'no C call',
    'torch_module': 'no C call', 'Context.info': 'a name buffer and three out-parameters, run by the GPU suite',
    'Context.close': 'lifetime', 'TapTable.close': 'lifetime', 'TapTable.broadcast_rccl': 'needs an RCCL communicator',
}


def recorded_names(native):
    """(functions, TapTable methods, Context methods) that the fixture covers, by the naming rule of the docstring."""
    functions = sorted(
        name for name, f in vars(native).items()
        if inspect.isfunction(f) and f.__module__ == native.__name__ and not name.startswith('_') and name not in NOT_RECORDED
        and (name.endswith('_device') or name.endswith('_bytes') or name.startswith('describe_')
             or name in ('scope_route', 'spectrum_run_length')))
    table = sorted(name for name, f in vars(native.TapTable).items()
                   if inspect.isfunction(f) and ('device' in name or name == 'prepare' or name.startswith('describe')))
    context = sorted(name for name in ('set_variant', 'time_copy') if name in vars(native.Context))
    return functions, table, context


def public_callables(native):
    """Every public function of the module and every public method of its two classes: recorded, or listed above."""
    names = [name for name, f in vars(native).items()
             if inspect.isfunction(f) and f.__module__ == native.__name__ and not name.startswith('_')]
    for cls in (native.TapTable, native.Context):
        names += [f'{cls.__name__}.{name}' for name, f in vars(cls).items()
                  if not name.startswith('_') and (inspect.isfunction(f) or isinstance(f, classmethod))]
    return sorted(names)


def signature_tables(native):
    """name -> (restype, argtypes) over every ``*SIGNATURES`` table of the module."""
    merged = {}
    for attr, table in vars(native).items():
        if attr.endswith('SIGNATURES') and isinstance(table, dict):
            merged.update(table)
    return merged


def as_received(argtype, value):
    """``value`` as the C function sees it through ``argtype``; raises what the real call would raise."""
    argtype.from_param(value)
    if type(value).__name__ == 'CArgObject':               # ctypes.byref(...)
        return 'out'
    if isinstance(value, ctypes.Array):
        return len(value) if value._type_ is ctypes.c_char else list(value)
    if isinstance(value, ctypes._Pointer):
        return 'out' if value else 0
    if value is None:
        return 0
    if isinstance(value, bytes):
        return value.decode('latin-1')
    if isinstance(value, ctypes._SimpleCData):
        return value.value or 0
    if argtype in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(argtype, ctypes._Pointer):
        return ctypes.c_void_p(value).value or 0
    return argtype(value).value


class RecordingLibrary:
    """Stands in for the ``CDLL``: every bound function records ``[name, arguments]`` and returns 0."""

    def __init__(self, native):
        self._signatures = signature_tables(native)
        self.calls = []
        self.described = 0

    def __getattr__(self, name):
        if name.startswith('_') or name not in self._signatures:
            raise AttributeError(name)
        argtypes = self._signatures[name][1]

        def call(*args):
            if len(args) != len(argtypes):
                raise TypeError(f'{name}: {len(args)} arguments for {len(argtypes)} parameters')
            outs = 0
            for argtype, value in zip(argtypes, args):
                if type(value).__name__ == 'CArgObject':
                    value._obj.value = 4000 + 16 * len(self.calls) + outs
                    outs += 1
                elif argtype is ctypes.c_char_p and isinstance(value, ctypes.Array):
                    self.described += 1
                    value.value = f'launch {self.described}'.encode()
            self.calls.append([name, [as_received(t, v) for t, v in zip(argtypes, args)]])
            return 0
        setattr(self, name, call)
        return call


class Handle:
    def __init__(self, lib, handle):
        self._lib, self.handle = lib, handle


def _variations(parameters, with_channels):
    bools = [p.name for p in parameters if p.annotation == 'bool']
    patterns = [{b: True for b in bools}, {b: False for b in bools}] if bools else [{}]
    if len(bools) > 1:
        patterns += [{b: b == one for b in bools} for one in bools]
    widths = [None, 0.5] if any(p.name == 'width' for p in parameters) else [None]
    channels = [TABLE_CHANNELS, 2] if with_channels and any(p.name == 'channels' for p in parameters) else [None]
    return itertools.product(patterns, widths, channels)


def _arguments(parameters, lib, pattern, width, channels):
    kwargs = {}
    for i, p in enumerate(parameters):
        if p.name == 'ctx':
            kwargs[p.name] = Handle(lib, CTX_HANDLE)
        elif p.name == 'bank':
            kwargs[p.name] = Handle(lib, BANK_HANDLE)
        elif p.name in pattern:
            kwargs[p.name] = pattern[p.name]
        elif p.name == 'width':
            kwargs[p.name] = width
        elif p.name == 'channels' and channels is not None:
            kwargs[p.name] = channels
        elif p.name == 'percentiles':
            kwargs[p.name] = (5.0, 50.0)
        elif p.name == 'image':
            kwargs[p.name] = b'\x7fELF image'
        elif p.name == 'kernel':
            kwargs[p.name] = 'kernel_name'
        elif p.annotation == 'float':
            kwargs[p.name] = 0.25 + i
        else:
            kwargs[p.name] = 1000 + 16 * i
    return kwargs


def _jsonable(value):
    if isinstance(value, dict):
        return {k: _jsonable(v) for k, v in value.items()}
    if isinstance(value, (tuple, list)):
        return [_jsonable(v) for v in value]
    if isinstance(value, bytes):
        return value.decode('latin-1')
    assert value is None or isinstance(value, (bool, int, float, str)), type(value)
    return value


def record(native):
    """``{wrapper: [{args, calls, returns}, ...]}`` of ``native`` (a loaded ``_native`` module) against the stand-in."""
    lib = RecordingLibrary(native)
    saved, native._lib = native._lib, lib
    try:
        functions, table_methods, context_methods = recorded_names(native)
        table = native.TapTable.__new__(native.TapTable)
        table.ctx, table._lib, table._h, table.num_channels = Handle(lib, CTX_HANDLE), lib, TABLE_HANDLE, TABLE_CHANNELS
        context = native.Context.__new__(native.Context)
        context._lib, context._h, context.device = lib, CTX_HANDLE, 0
        targets = [(name, getattr(native, name), False) for name in functions]
        targets += [(f'TapTable.{name}', getattr(table, name), True) for name in table_methods]
        targets += [(f'Context.{name}', getattr(context, name), False) for name in context_methods]
        out = {}
        try:
            for label, fn, with_channels in targets:
                parameters = list(inspect.signature(fn).parameters.values())
                runs = []
                for pattern, width, channels in _variations(parameters, with_channels):
                    kwargs = _arguments(parameters, lib, pattern, width, channels)
                    lib.calls, lib.described = [], 0
                    returned = fn(**kwargs)
                    shown = {k: v for k, v in kwargs.items() if k not in ('ctx', 'bank')}
                    runs.append(_jsonable({'args': shown, 'calls': lib.calls, 'returns': returned}))
                assert all(run['calls'] for run in runs), label
                out[label] = runs
        finally:
            table._h = context._h = None            # (no destroy call when the two stand-ins are collected)
        return out
    finally:
        native._lib = saved


def load_native(checkout: pathlib.Path):
    path = checkout / 'vndecorrelate_amd' / '_native.py'
    spec = importlib.util.spec_from_file_location('recorded_native', path)
    module = importlib.util.module_from_spec(spec)
    sys.modules['recorded_native'] = module
    spec.loader.exec_module(module)
    return module


def dumps(fixture) -> str:
    lines = ['{', ' "header": ' + json.dumps(fixture['header']) + ',', ' "wrappers": {']
    blocks = []
    for label, runs in fixture['wrappers'].items():
        blocks.append(f'  {json.dumps(label)}: [\n' + ',\n'.join('   ' + json.dumps(run) for run in runs) + '\n  ]')
    return '\n'.join(lines) + '\n' + ',\n'.join(blocks) + '\n }\n}\n'


def main(argv):
    if len(argv) != 2:
        sys.exit(__doc__)
    checkout = pathlib.Path(argv[1]).resolve()
    if checkout == REPO:
        sys.exit('record another checkout than this tree: the fixture must not come from the code under test')
    commit = subprocess.run(['git', '-C', str(checkout), 'rev-parse', 'HEAD'], capture_output=True, text=True,
                            check=True).stdout.strip()
    dirty = subprocess.run(['git', '-C', str(checkout), 'status', '--porcelain', '--', 'vndecorrelate_amd/_native.py'],
                           capture_output=True, text=True, check=True).stdout.strip()
    if dirty:
        sys.exit(f'{checkout} has an uncommitted _native.py: record a commit')
    wrappers = record(load_native(checkout))
    header = {'generated_by': 'tools/gen_native_calls_golden.py', 'recorded_commit': commit,
              'note': 'the calls of that commit\'s vndecorrelate_amd/_native.py against a recording stand-in for the '
                      'library; generated from another checkout, never from the code under test',
              'wrappers': len(wrappers), 'runs': sum(len(r) for r in wrappers.values())}
    OUT.write_text(dumps({'header': header, 'wrappers': wrappers}))
    print(f'{header["wrappers"]} wrappers, {header["runs"]} runs of commit {commit[:7]} -> {OUT} ({OUT.stat().st_size} bytes)')


if __name__ == '__main__':
    main(sys.argv)

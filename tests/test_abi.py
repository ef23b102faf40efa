"""CPU tier: the C-ABI shared library builds, loads, and exports exactly what
include/vnd_amd.h declares.  No compute calls (there is no GPU here)."""
import ctypes
import pathlib
import re
import subprocess

import pytest

REPO = pathlib.Path(__file__).resolve().parents[1]
HEADER = REPO / 'include' / 'vnd_amd.h'


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as entry
    entry.build()
    from vndecorrelate_amd import _native
    return _native.load_library()


INTERNAL = REPO / 'include' / 'vnd_amd_internal.h'


def declared_functions(header=HEADER):
    text = re.sub(r'/\*.*?\*/', '', header.read_text(), flags=re.S)
    return sorted(set(re.findall(r'\b(vnd_[a-z0-9_]+)\s*\(', text)))


C_SCALARS = {'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64, 'int': ctypes.c_int, 'float': ctypes.c_float,
             'double': ctypes.c_double}
C_POINTEES = dict(C_SCALARS, uint8_t=ctypes.c_uint8, uint32_t=ctypes.c_uint32, uint64_t=ctypes.c_uint64, char=ctypes.c_char)
C_RETURNS = {'vnd_status': ctypes.c_int, 'int': ctypes.c_int, 'const char *': ctypes.c_char_p}
BOUND_HEADERS = sorted(p.name for p in (REPO / 'include').glob('*.h'))


def prototypes(header):
    """``{function: (return type, [parameter type, ...])}`` of a header, comments stripped, types as the header spells them
    (one space between words, the parameter's name dropped)."""
    text = re.sub(r'/\*.*?\*/', '', header.read_text(), flags=re.S)
    found = {}
    for ret, name, params in re.findall(r'([A-Za-z_][\w \*]*?)\b(vnd_[a-z0-9_]+)\s*\(([^()]*)\)\s*;', text):
        assert name not in found, f'{name} is declared twice in {header.name}'
        params = [' '.join(p.split()) for p in params.split(',')]
        types = [] if params == ['void'] else [re.sub(r'\s*\b\w+$', '', p) for p in params]
        assert all(types), f'{name}: a parameter of {header.name} without a name'
        found[name] = (' '.join(ret.split()), types)
    return found


def allowed_ctypes(c_type):
    """The ctypes types a parameter spelled ``c_type`` in a header may be bound as."""
    if '*' not in c_type:
        return {C_SCALARS[c_type]}                                   # a scalar: exactly its own type
    base = c_type.replace('const', '').replace('*', '').strip()
    allowed = {ctypes.c_void_p}
    if c_type.count('*') == 2:
        allowed.add(ctypes.POINTER(ctypes.c_void_p))
    elif base in C_POINTEES:
        allowed.add(ctypes.POINTER(C_POINTEES[base]))
    if c_type in ('char *', 'const char *', 'const void *'):
        allowed.add(ctypes.c_char_p)
    return allowed


@pytest.mark.parametrize('header', BOUND_HEADERS)
def test_binding_matches_the_header_type_by_type(header):
    """Every function of the header is bound under the header's table, with the header's return type and every parameter
    of the header's type: a row that says ``c_int32`` where the header says ``int64_t`` fails here, not past 2^31 frames."""
    from vndecorrelate_amd import _native
    assert header in _native.HEADERS, f'include/{header} has no line in _native.HEADERS'
    table, declared = _native.HEADERS[header], prototypes(REPO / 'include' / header)
    assert sorted(declared) == declared_functions(REPO / 'include' / header), 'a declaration the parser did not take'
    assert sorted(table) == sorted(declared)
    for name, (ret, params) in declared.items():
        restype, argtypes = table[name]
        assert restype is C_RETURNS[ret], f'{name} returns {ret}, bound as {restype.__name__}'
        assert len(argtypes) == len(params), f'{name} takes {len(params)} parameters, {len(argtypes)} are bound'
        for i, (c_type, bound) in enumerate(zip(params, argtypes)):
            assert bound in allowed_ctypes(c_type), f'{name}: parameter {i} is `{c_type}`, bound as {bound.__name__}'


def test_every_header_is_bound_once():
    from vndecorrelate_amd import _native
    assert sorted(_native.HEADERS) == BOUND_HEADERS and len(BOUND_HEADERS) >= 21
    names = [name for table in _native.HEADERS.values() for name in table]
    assert len(names) == len(set(names)), 'a function is bound under two headers'
    tables = {name: t for name, t in vars(_native).items() if name.endswith('SIGNATURES') and isinstance(t, dict)}
    assert sorted(map(id, tables.values())) == sorted(map(id, _native.HEADERS.values())), 'a table that HEADERS does not list'


def test_the_typed_check_refuses_a_narrowed_row():
    """int32 where the header says int64_t, a float for a double, the wrong pointee: none is among the types allowed."""
    assert ctypes.c_int32 not in allowed_ctypes('int64_t') and ctypes.c_int64 not in allowed_ctypes('int32_t')
    assert ctypes.c_float not in allowed_ctypes('double') and ctypes.c_void_p not in allowed_ctypes('int64_t')
    assert ctypes.POINTER(ctypes.c_int32) not in allowed_ctypes('const int64_t *')
    assert ctypes.POINTER(ctypes.c_void_p) not in allowed_ctypes('vnd_ctx *')
    assert ctypes.c_char_p not in allowed_ctypes('void *') and ctypes.c_int64 not in allowed_ctypes('void *')


def test_header_is_plain_c():
    """The boundary must be consumable by cgo/JNI/ctypes: compile it as C."""
    src = '#include "vnd_amd.h"\nint main(void){return VND_ABI_VERSION == vnd_abi_version() ? 0 : 1;}\n'
    r = subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-fsyntax-only', '-I', str(REPO / 'include'),
                        '-x', 'c', '-'], input=src.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    assert 'torch' not in HEADER.read_text().lower().replace('(hipmalloc / torch)', '')


def test_every_declared_symbol_is_exported(lib):
    names = declared_functions()
    assert len(names) >= 15
    for name in names:
        assert hasattr(lib, name), f'{name} declared in vnd_amd.h but not exported'
    # (that the Python binding covers the whole header, nothing more: test_binding_matches_the_header_type_by_type)
    assert len(names) <= 35, 'the drop-in ABI stays small: measurement and tuning hooks belong in vnd_amd_internal.h'
    # the measurement / tuning / diagnosis hooks: their own header, exported by the same library, bound separately
    internal = declared_functions(INTERNAL)
    assert internal and not set(internal) & set(names)
    for name in internal:
        assert hasattr(lib, name), f'{name} declared in vnd_amd_internal.h but not exported'


def test_abi_version_and_error_channel(lib):
    assert lib.vnd_abi_version() == 2
    assert isinstance(lib.vnd_last_error(), bytes)
    n = ctypes.c_int32(-1)
    rc = lib.vnd_device_count(ctypes.byref(n))
    assert rc in (0, 2) and n.value >= 0


def test_no_cpu_fallback_without_device(lib):
    """On a box without a GPU the product path fails loudly (and says why)."""
    from vndecorrelate_amd import _native
    if _native.device_count() > 0:
        pytest.skip('a GPU is present')
    with pytest.raises(_native.NativeError) as e:
        _native.Context(0)
    assert 'gfx950' in str(e.value) or 'HIP device' in str(e.value)
    import numpy as np
    import vndecorrelate_amd.decorrelation as vnd
    fir = vnd.generate_velvet_noise(duration_seconds=0.03, num_impulses=30, seed=1)
    with pytest.raises(RuntimeError):
        vnd.convolve_velvet_noise(np.zeros((100, 2), np.float32), fir)
    with pytest.raises(RuntimeError):
        vnd.VelvetNoise(sample_rate_hz=44100, seed=1).decorrelate(np.zeros((100, 2), np.float32))


def test_product_never_imports_the_oracle():
    for path in (REPO / 'vndecorrelate_amd').rglob('*.py'):
        text = path.read_text()
        assert 'oracle' not in text.replace('the oracle', '').replace('oracle/', ''), path
    for path in (REPO / 'vndecorrelate_amd' / 'csrc').iterdir():
        assert 'oracle' not in path.read_text(), path

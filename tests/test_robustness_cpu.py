"""CPU tier: host-side robustness (no GPU compute): the build's staleness check sees every
source of the translation unit, and the FIR table cache is safe under concurrent callers."""
import os
import pathlib
import threading
import time

import numpy as np

REPO = pathlib.Path(__file__).resolve().parents[1]


def test_build_watches_every_native_source(tmp_path, monkeypatch):
    """An edit to ANY header under csrc/ or include/ must rebuild the git-ignored .so
    (it ships to the GPU box as built)."""
    import __graft_entry__ as entry
    ran = []
    monkeypatch.setattr(entry.subprocess, 'run', lambda cmd, **kw: ran.append([str(c) for c in cmd]))
    fake = tmp_path / 'libvnd_amd.so'
    fake.write_bytes(b'')
    monkeypatch.setattr(entry, 'LIB', fake)
    sources = sorted((REPO / 'vndecorrelate_amd' / 'csrc').glob('*.h*')) + sorted((REPO / 'vndecorrelate_amd' / 'csrc').glob('*.inc')) + sorted((REPO / 'include').glob('*.h'))
    assert len(sources) >= 6
    newest = max(s.stat().st_mtime for s in sources)
    for src in sources:
        # library newer than everything except `src`
        os.utime(fake, (newest + 10, newest + 10))
        old = src.stat()
        try:
            os.utime(src, (newest + 20, newest + 20))
            ran.clear()
            try:
                entry.build()
            except Exception:
                pass                       # the import after the (mocked) compile may fail; only the decision matters
            assert any('hipcc' in c[0] for c in ran), f'an edit to {src.name} did not trigger a rebuild'
        finally:
            os.utime(src, (old.st_atime, old.st_mtime))
    os.utime(fake, (newest + 30, newest + 30))
    ran.clear()
    try:
        entry.build()
    except Exception:
        pass
    assert not any('hipcc' in c[0] for c in ran), 'an up-to-date library was rebuilt'


class _FakeTable:
    closed = 0

    def close(self):
        type(self).closed += 1


def test_table_cache_is_thread_safe(monkeypatch):
    """Concurrent lookups build each key at most a few times, always hand every thread a live
    table, and eviction never closes a table somebody may still be using."""
    from vndecorrelate_amd import _native
    import vndecorrelate_amd.decorrelation as d

    built = []

    def fake_create(ctx, offs, idx, w, **kw):
        time.sleep(0.001)
        t = _FakeTable()
        built.append(t)
        return t

    monkeypatch.setattr(_native.TapTable, 'create', staticmethod(fake_create))
    monkeypatch.setattr(_native, 'default_context', lambda: None)
    cache = d._TableCache(capacity=4)

    class Arr:
        tap_offsets = tap_index = tap_weight = np.zeros(1)

        def kwargs(self):
            return {}

    errors = []

    def worker(seed):
        rng = np.random.default_rng(seed)
        for _ in range(300):
            key = int(rng.integers(0, 12))
            try:
                t = cache.get(key, Arr)
                assert isinstance(t, _FakeTable)
            except Exception as e:      # noqa: BLE001
                errors.append(e)

    threads = [threading.Thread(target=worker, args=(s,)) for s in range(8)]
    [t.start() for t in threads]
    [t.join() for t in threads]
    assert not errors
    assert len(cache._items) <= 4
    assert _FakeTable.closed == 0       # dropped, never closed under a possible user
    cache.clear()
    assert len(cache._items) == 0


def test_host_entry_points_take_the_context_lock():
    """Every *_host entry point of the C ABI serialises on the context (source-level check; the
    behaviour is exercised on the GPU by tests/test_gpu_robustness.py).  The lock is taken in one place, the
    HostCall helper every host call runs on, which also waits for the call's streams on every way out."""
    import re
    # (the library's one translation unit: vnd_amd.hip and the parts it includes)
    csrc = REPO / 'vndecorrelate_amd' / 'csrc'
    text = '\n'.join(f.read_text() for f in sorted(csrc.glob('*.hip')) + sorted(csrc.glob('*.hpp')))
    headers = '\n'.join(f.read_text() for f in sorted((REPO / 'include').glob('*.h')))
    headers = re.sub(r'/\*.*?\*/', '', headers, flags=re.S)
    host_fns = sorted(set(re.findall(r'\b(vnd_[a-z0-9_]+_host)\s*\(', headers)))
    assert len(host_fns) >= 11
    helper = re.search(r'\nclass HostCall \{\n(.*?)\n\};\n', text, re.S).group(1)
    assert 'HostLock lock_;' in helper and 'lock_(c->host_mutex)' in helper
    assert '~HostCall() { drain(); }' in helper and 'hipStreamSynchronize' in helper
    assert text.count('host_mutex)') == 1                   # nobody else takes it, or takes it twice
    takes_lock = 'HostCall call(ctx);'
    # each one either locks itself or forwards to a static helper that does
    bodies = {m.group(1): m.group(2) for m in re.finditer(r'static vnd_status (\w+_host)\(.*?\n\{(.*?)\n\}\n', text, re.S)}
    locked_helpers = {name for name, body in bodies.items() if takes_lock in body}
    for fn in host_fns:
        bodies[fn] = re.search(r'vnd_status ' + fn + r'\(.*?\n\{(.*?)\n\}\n', text, re.S).group(1)
        assert takes_lock in bodies[fn] or any(h + '(' in bodies[fn] for h in locked_helpers), fn
    # once the helper exists, every way out is its exit: no return of another kind, no synchronise of the call's own
    # (the callables handed to the helper return to the helper: cut out before the search)
    checked = 0
    for fn, body in bodies.items():
        if takes_lock not in body:
            continue
        after = re.sub(r'\[&\] \{ return [^;]*; \}\);', '', body[body.index(takes_lock):])            # one statement
        after = re.sub(r'\[&\][^\n]*\{\n.*?\n {4,}\}\);', '', after, flags=re.S)                        # a block
        assert '[&]' not in after, fn
        assert 'hipStreamSynchronize' not in after and 'HIP_TRY' not in after, fn
        returns = re.findall(r'\n\s+return ([^;]*);', after)
        assert returns and all(r.startswith('call.finish(') for r in returns), (fn, returns)
        checked += 1
    assert checked >= 8

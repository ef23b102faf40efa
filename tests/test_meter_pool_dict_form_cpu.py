"""The dict form of the three meters that answer ``valid`` in {-1, 0, 1} - the polar-moments, the count-grid and the
level-envelope voice pool - over a fake ``_call_host``: one body in ``streaming._MeterPool`` does their bookkeeping, and
each pool says only how a host row is handed back.  No GPU."""
import numpy as np
import pytest

START, END = 1, 2
S, M = 4, 100


def _polar():
    from vndecorrelate_amd import analysis
    return analysis.stereo_image_voice_pool(S, max_frames_per_call=M), None, (8,), np.float64


def _scope():
    from vndecorrelate_amd import vectorscope
    pool = vectorscope.polar_histogram_voice_pool(S, max_frames_per_call=M, radius_scale=1.0, num_angle_bins=12,
                                                  num_radius_bins=7, window_frames=250)
    return pool, 'grids', (12, 7), np.int32


def _level():
    from vndecorrelate_amd import vectorscope
    pool = vectorscope.polar_level_voice_pool(S, max_frames_per_call=M, window_frames=250, radius_scale=1.0, num_bins=8)
    return pool, 'levels', (2, 8), np.float32


POOLS = {'polar': _polar, 'scope': _scope, 'level': _level}


@pytest.fixture
def no_device(monkeypatch):
    from vndecorrelate_amd import _native

    def refuse(*a, **k):
        raise AssertionError('the dict form reached the device')
    monkeypatch.setattr(_native, 'default_context', refuse)
    monkeypatch.setattr(_native, 'torch_module', refuse)


class FakeHost:
    """Stands for ``_call_host``: records what every call uploads and whether rows were asked for, keeps a position of
    its own per slot (the device's) and answers the rule's ``valid`` and rows that name the slot and the call."""

    def __init__(self, pool, shape, dtype):
        self.pool, self.shape, self.dtype = pool, shape, dtype
        self.calls, self.rows_asked = [], []
        self.pos = np.zeros(pool.slots, np.int64)
        pool._call_host = self

    def __call__(self, x, counts, flags, rows=True):
        from vndecorrelate_amd.vectorscope import scope_voice_spans
        p = self.pool
        assert x.shape == (p.slots, p.max_frames_per_call, 2) and x.dtype == p.dtype
        assert counts.dtype == flags.dtype == np.int32
        self.calls.append((x.copy(), counts.copy(), flags.copy()))
        self.rows_asked.append(rows)
        valid, self.pos = scope_voice_spans(self.pos, counts, flags, p.max_frames_per_call)
        if not rows:
            return None, valid.astype(np.int32)
        out = np.full((p.slots,) + self.shape, -1, self.dtype)
        for b, v in enumerate(valid):
            if v == 1:
                out[b] = 1000 * len(self.calls) + b
        return out, valid.astype(np.int32)


@pytest.mark.parametrize('kind', sorted(POOLS))
def test_bookkeeping_over_a_schedule(no_device, kind):
    from vndecorrelate_amd import _native
    pool, rows_keyword, shape, host_dtype = POOLS[kind]()
    assert pool.in_channels == 2 and pool._bank_len() == 1 and pool._out_dtype == np.float64 and pool._form is None
    fake = FakeHost(pool, shape, host_dtype)
    rng = np.random.default_rng(0)

    def block(n):
        return rng.uniform(-1, 1, (n, 2)).astype(np.float32)

    def state():
        return pool.positions.tolist(), pool.live.tolist(), pool._form
    assert pool.process({}) == {} and not fake.calls and pool._form is None       # nothing at all: no device call
    a, b = block(M), block(7)
    out = pool.process({0: a, 2: b}, start=[0, 2])                                # a block and a start
    assert sorted(out) == [0, 2] and out[0].shape == shape and out[0].dtype == np.float64 and (out[2] == 1002).all()
    x, counts, flags = fake.calls[-1]
    assert counts.tolist() == [M, 0, 7, 0] and flags.tolist() == [START, 0, START, 0]
    assert x[0].tobytes() == a.tobytes() and x[2, :7].tobytes() == b.tobytes() and not x[2, 7:].any() and not x[1].any()
    assert state() == ([M, 0, 7, 0], [True, False, True, False], 'dict')
    for _ in range(3):                                                            # slot 0 advances alone; slot 2 is idle
        out = pool.process({0: block(M)})
    assert sorted(out) == [0] and (out[0] == 1000 * 4 + 0).all()
    assert state() == ([4 * M, 0, 7, 0], [True, False, True, False], 'dict')
    assert pool.process({0: block(0)}) == {} and len(fake.calls) == 4             # an empty block alone: no device call
    out = pool.process({0: block(0), 2: block(3)})                                # ... beside a neighbour's block: idle
    assert sorted(out) == [2] and len(fake.calls) == 5 and fake.calls[-1][1].tolist() == [0, 0, 3, 0]
    assert state() == ([4 * M, 0, 10, 0], [True, False, True, False], 'dict')
    # slot 2 ends with no block, slot 1 is a whole voice in one call, slot 0 ends with its last block, slot 3 starts with
    # no block: all four are answered
    out = pool.process({1: block(88), 0: block(5)}, start=[1, 3], end=[2, 1, 0])
    assert sorted(out) == [0, 1, 2, 3] and (out[1] == 1000 * len(fake.calls) + 1).all()
    assert fake.calls[-1][1].tolist() == [5, 88, 0, 0] and fake.calls[-1][2].tolist() == [END, START | END, END, START]
    assert state() == ([0, 0, 0, 0], [False, False, False, True], 'dict')
    pool.process({2: block(10)}, start=[2])
    with pytest.raises(ValueError, match='slot 2 holds a live voice'):
        pool.process({2: block(10)}, start=[2])
    pool.process({2: block(10)}, start=[2], discard=True)                         # a live voice is dropped only on request
    assert fake.calls[-1][2].tolist() == [0, 0, START, 0] and state()[0] == [0, 0, 10, 0]
    assert pool.positions.tolist() == fake.pos.tolist()                           # the mirror is the device's
    assert all(fake.rows_asked)
    if rows_keyword:                                                              # no rows: None for every answered slot
        out = pool.process({2: block(4), 3: block(0)}, end=[3], **{rows_keyword: False})
        assert out == {2: None, 3: None} and fake.rows_asked[-1] is False
        assert state() == ([0, 0, 14, 0], [False, False, True, False], 'dict')
    # a native that answers another valid than the spans is an error, and the mirror stays
    before, calls = state(), len(fake.calls)
    pool._call_host = lambda x, c, f, rows=True: (np.zeros((S,) + shape, host_dtype), np.array([0, 0, 1, 1], np.int32))
    with pytest.raises(_native.NativeError, match='the voice pool answered .* the spans are'):
        pool.process({2: block(1)})
    assert state() == before and len(fake.calls) == calls
    with pytest.raises(RuntimeError, match='runs through process\\(\\)'):
        pool.process_dev(None, None, None)

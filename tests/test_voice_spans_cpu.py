"""The six public span functions of the voice pools against a scalar restatement of their headers' formulas, slot by
slot, on the full grid of positions, counts and flags - bad and idle corners included.  The restatements are plain ``if``s
and share nothing with the functions under test.  No GPU."""
import itertools

import numpy as np

START, END = 1, 2
M, H, W, HOP, MAX_DELAY = 8, 3, 4, 2, 3
TOP = 1 << 60
POSITIONS = (-1, 0, 1, H - 1, H, H + 1, TOP, TOP + 1)
COUNTS = (-1, 0, 1, M, M + 1)
FLAGS = (0, START, END, START | END)
DELAYS = (-1, 0, MAX_DELAY, MAX_DELAY + 1)
GRID = list(itertools.product(POSITIONS, COUNTS, FLAGS))


def _head(pos, n, f):
    """``(p, bad)``: include/vnd_voice_stream.h - START restarts at 0; a count outside [0, M] or a p outside [0, 2^60]."""
    p = 0 if f & START else pos
    return p, (n < 0 or n > M or p < 0 or p > TOP)


def _velvet(pos, n, f):
    p, bad = _head(pos, n, f)
    if bad:
        return -1, pos
    first = max(0, p - H)
    last = p + n if f & END else max(0, p + n - H)
    return last - first, (0 if f & END else p + n)


def _haas(pos, n, f, d):
    p, bad = _head(pos, n, f)
    if bad:
        return -1, pos
    if n == 0 and not f & (START | END):                  # idle: the delay is not looked at
        return 0, pos
    if d < 0 or d > MAX_DELAY:
        return -1, pos
    if f & END:
        return n + d, 0
    return n, p + n


def _correlogram(pos, n, f):
    p, bad = _head(pos, n, f)
    if bad:
        return -1, pos

    def complete(q):
        return (q - W) // HOP + 1 if q >= W else 0
    return complete(p + n) - complete(p), (0 if f & END else p + n)


def _polar(pos, n, f):
    p, bad = _head(pos, n, f)
    if bad:
        return -1, pos
    if n == 0 and not f & (START | END):                  # idle: no answer, the position stays
        return 0, pos
    return 1, (0 if f & END else p + n)


def _scope(pos, n, f):
    """include/vnd_scope_voice_stream.h: valid and the position; a row is cleared when a slot answers 1 from p = 0."""
    p = pos
    if f & START:
        p = 0
    if n < 0 or n > M:
        return -1, pos
    if p < 0 or p > TOP:
        return -1, pos
    if n == 0 and f & START == 0 and f & END == 0:
        return 0, pos
    if f & END:
        return 1, 0
    return 1, p + n


def _spectrum(pos, n, f):
    """include/vnd_spectrum_voice_stream.h, nperseg W and hop HOP: (out_count, segments, new position)."""
    p, bad = _head(pos, n, f)
    if bad:
        return -1, -1, pos

    def complete(q):
        if q < W:
            return 0
        return (q - W) // HOP + 1
    if n == 0 and not f & (START | END):                  # idle: the means stay as they are
        return 0, -1, pos
    return complete(p + n) - complete(p), complete(p + n), (0 if f & END else p + n)


def _columns(grid):
    return [np.array(c, np.int64) for c in zip(*grid)]


def _check(got, want, grid):
    assert all(a.dtype == np.int64 for a in got)
    for cell, *values, expected in zip(grid, *(a.tolist() for a in got), want):
        assert tuple(values) == expected, cell


def test_grid_size():
    assert len(GRID) == 160 and len(GRID) * len(DELAYS) == 640


def test_voice_spans_grid():
    from vndecorrelate_amd.streaming import voice_spans
    pos, n, f = _columns(GRID)
    _check(voice_spans(pos, n, f, H, M), [_velvet(*cell) for cell in GRID], GRID)


def test_haas_voice_spans_grid():
    from vndecorrelate_amd.streaming import haas_voice_spans
    grid = [cell + (d,) for cell in GRID for d in DELAYS]
    pos, n, f, d = _columns(grid)
    _check(haas_voice_spans(pos, n, f, d, MAX_DELAY, M), [_haas(*cell) for cell in grid], grid)


def test_correlogram_voice_spans_grid():
    from vndecorrelate_amd.analysis import correlogram_voice_spans
    pos, n, f = _columns(GRID)
    _check(correlogram_voice_spans(pos, n, f, W, HOP, M), [_correlogram(*cell) for cell in GRID], GRID)


def test_polar_voice_spans_grid():
    from vndecorrelate_amd.analysis import polar_voice_spans
    pos, n, f = _columns(GRID)
    _check(polar_voice_spans(pos, n, f, M), [_polar(*cell) for cell in GRID], GRID)


def test_scope_voice_spans_grid():
    from vndecorrelate_amd.vectorscope import scope_voice_spans
    pos, n, f = _columns(GRID)
    _check(scope_voice_spans(pos, n, f, M), [_scope(*cell) for cell in GRID], GRID)


def test_spectrum_voice_spans_grid():
    from vndecorrelate_amd.spectral import spectrum_voice_spans
    pos, n, f = _columns(GRID)
    got = spectrum_voice_spans(pos, n, f, W, HOP, M)
    assert len(got) == 3
    _check(got, [_spectrum(*cell) for cell in GRID], GRID)

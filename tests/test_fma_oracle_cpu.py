"""CPU tier: the reference for VND_MODE_FMA (include/vnd_amd.h: ``acc = fma(x, w, acc)`` in table order, one
rounding per tap) against exact rational arithmetic.  ``vnd_oracle.fma_f32`` must be the correctly rounded float32
fma (ties to even) on random and adversarial triples; ``vnd_oracle.convolve_taps_fma`` must be the mode's tap sum
restated with ``fractions.Fraction``; the C oracle's ``convolve_fma`` must be ``convolve_taps_fma`` bit for bit; and
on +-1 tables the fma arithmetic must equal the exact one, the identity the library's ``arithmetic_of`` relies on."""
import ctypes
import ctypes.util
from fractions import Fraction

import numpy as np
import pytest
from hypothesis import given, settings, strategies as st

from oracle import c_oracle
from oracle import vnd_oracle as O
from test_properties_cpu import class_table, sparse_fir
from vndecorrelate_amd.taps import class_path_arrays, function_path_arrays

SET = settings(max_examples=40, deadline=None, derandomize=True, database=None)
F32 = np.float32
_MAX = Fraction(2) ** 128          # the first power of two float32 cannot hold


def round_f32(q: Fraction, zero_sign: float = 1.0) -> np.float32:
    """Exact rational -> float32, round to nearest, ties to even; ``zero_sign`` is the sign IEEE 754 gives an
    exact zero sum."""
    if q == 0:
        return F32(np.copysign(0.0, zero_sign))
    sign = -1 if q < 0 else 1
    a = abs(q)
    e = a.numerator.bit_length() - a.denominator.bit_length()         # 2^e <= a < 2^(e+2)
    if Fraction(2) ** e > a:
        e -= 1
    if Fraction(2) ** (e + 1) <= a:
        e += 1
    quantum = Fraction(2) ** max(e - 23, -149)
    m, rem = divmod(a, quantum)
    half = quantum / 2
    if rem > half or (rem == half and m % 2 == 1):
        m += 1
    r = m * quantum
    if r >= _MAX:
        return F32(sign * np.inf)
    return F32(sign * float(r))


def fma_exact(x, w, acc) -> np.float32:
    x, w, acc = F32(x), F32(w), F32(acc)
    q = Fraction(float(x)) * Fraction(float(w)) + Fraction(float(acc))
    p_neg = np.signbit(x) != np.signbit(w)
    # an exact zero sum is -0 only when both addends are -0 (round to nearest)
    zero_sign = -1.0 if (p_neg and np.signbit(acc) and (x == 0 or w == 0) and acc == 0) else 1.0
    return round_f32(q, zero_sign)


def _random_f32(rng, n, lo=-60, hi=60):
    mant = rng.uniform(1.0, 2.0, n)
    return (rng.choice([-1.0, 1.0], n) * np.ldexp(mant, rng.integers(lo, hi, n))).astype(F32)


def _triples():
    """(x, w, acc) float32 arrays: random ones and the adversarial families."""
    rng = np.random.default_rng(20260)
    xs, ws, accs = [], [], []

    def add(x, w, acc):
        xs.append(np.asarray(x, F32).ravel())
        ws.append(np.asarray(w, F32).ravel())
        accs.append(np.asarray(acc, F32).ravel())

    # random
    add(_random_f32(rng, 3000), _random_f32(rng, 3000), _random_f32(rng, 3000, -120, 0))
    # a product near half an ulp of acc, its low bits far below float64 precision (the double-rounding trap)
    m = 3000
    acc = _random_f32(rng, m, -10, 10)
    ulp = np.spacing(np.abs(acc)).astype(np.float64)
    x = (rng.uniform(1.0, 2.0, m)).astype(F32)
    w = (0.5 * ulp / x.astype(np.float64) * rng.choice([-1.0, 1.0], m)).astype(F32)
    wiggle = rng.integers(-2, 3, m)
    for s in range(m):
        for _ in range(abs(int(wiggle[s]))):
            w[s] = np.nextafter(w[s], F32(np.inf) if wiggle[s] > 0 else F32(-np.inf))
    add(x, w, acc)
    # the constructed ties: (1 + 2^-23)(1 - 2^-23) = 1 - 2^-46 times half an ulp, on odd and even acc
    acc = _random_f32(rng, 400, -10, 10)
    half = (0.5 * np.spacing(np.abs(acc)).astype(np.float64)).astype(F32)
    sgn = rng.choice([-1.0, 1.0], 400).astype(F32)
    add(np.full(400, 1 + 2.0 ** -23, F32), (F32(1 - 2.0 ** -23) * half * sgn).astype(F32), acc)
    add(np.full(400, 1 + 2.0 ** -23, F32), (F32(1 + 2.0 ** -23) * half * sgn).astype(F32), acc)
    # subnormal results: products and sums below 2^-126
    add(_random_f32(rng, 1500, -75, -60), _random_f32(rng, 1500, -75, -60),
        (_random_f32(rng, 1500, -20, 0).astype(np.float64) * 2.0 ** -126).astype(F32))
    add(_random_f32(rng, 500, -80, -70), _random_f32(rng, 500, -80, -70), np.zeros(500, F32))
    # exact cancellation: acc = -x*w where the product fits a float32, and x*w - acc with acc the rounded product
    x = (rng.integers(1, 2 ** 12, 500) * 2.0 ** -11).astype(F32)
    w = (rng.integers(1, 2 ** 12, 500) * 2.0 ** -7 * rng.choice([-1, 1], 500)).astype(F32)
    add(x, w, -(x.astype(np.float64) * w).astype(F32))
    x, w = _random_f32(rng, 500, -4, 4), _random_f32(rng, 500, -4, 4)
    add(x, w, -(x * w))
    # large exponent gaps both ways
    add(_random_f32(rng, 500, -70, -50), _random_f32(rng, 500, -70, -50), _random_f32(rng, 500, 20, 40))
    add(_random_f32(rng, 500, 20, 40), _random_f32(rng, 500, 20, 40), _random_f32(rng, 500, -70, -40))
    # overflow to +-inf, and sums just under the overflow threshold
    add(_random_f32(rng, 300, 64, 100), _random_f32(rng, 300, 64, 100), _random_f32(rng, 300, 100, 127))
    big = np.finfo(F32).max
    add(np.full(6, big, F32), np.float32([1, 1, -1, 1, 0.5, -0.5]),
        np.float32([2.0 ** 103, 2.0 ** 103 - 2.0 ** 79, -2.0 ** 103, -big, big, -big]))
    # signed zeros
    add(np.float32([0, -0.0, 0, -0.0, 1, -1]), np.float32([1, 1, -1, -1, 0, 0]), np.float32([-0.0, -0.0, 0, -0.0, -0.0, -0.0]))
    return np.concatenate(xs), np.concatenate(ws), np.concatenate(accs)


def test_fma_f32_is_correctly_rounded():
    x, w, acc = _triples()
    with np.errstate(over='ignore', invalid='ignore'):
        got = O.fma_f32(x, w, acc)
        naive = (x.astype(np.float64) * w.astype(np.float64) + acc.astype(np.float64)).astype(F32)
    want = np.array([fma_exact(a, b, c) for a, b, c in zip(x, w, acc)], F32)
    assert got.dtype == np.float32 and got.shape == x.shape
    bad = np.flatnonzero((got != want) | (np.signbit(got) != np.signbit(want)))
    assert bad.size == 0, [(x[i], w[i], acc[i], got[i], want[i]) for i in bad[:5]]
    # the set has power: naive float64-then-float32 rounding misses some of it, and it reaches every corner
    assert np.count_nonzero(naive != want) >= 20
    assert np.any(np.isinf(want)) and np.any((want != 0) & (np.abs(want) < np.finfo(F32).tiny)) and np.any(want == 0)
    # the vectorised call broadcasts like the scalar one
    assert O.fma_f32(x[:3], w[0], acc[:3]).shape == (3,)


def test_fma_f32_matches_libm_fmaf():
    """The C oracle's fma form calls libm's fmaf: it must round as the exact arithmetic (and fma_f32) do."""
    libm = ctypes.CDLL(ctypes.util.find_library('m'))
    libm.fmaf.restype = ctypes.c_float
    libm.fmaf.argtypes = [ctypes.c_float] * 3
    x, w, acc = _triples()
    got = np.array([libm.fmaf(float(a), float(b), float(c)) for a, b, c in zip(x, w, acc)], F32)
    with np.errstate(over='ignore', invalid='ignore'):
        want = O.fma_f32(x, w, acc)
    assert np.array_equal(got, want) and np.array_equal(np.signbit(got), np.signbit(want))


def _scalar_fma_conv(x, offsets, idx, w, seg_off=None, seg_end=None, seg_gain=None, flags=None, apply_gain=False):
    """The mode's definition, one output at a time, every rounding through Fraction."""
    n, channels = x.shape
    y = np.zeros((n, channels), F32)
    for c in range(channels):
        for n0 in range(n):
            if flags is not None and flags[c] & 1:
                y[n0, c] = x[n0, c]
                continue
            ends = [offsets[c + 1]] if seg_off is None else list(seg_end[seg_off[c]:seg_off[c + 1]])
            k, out = offsets[c], F32(0)
            for s, kend in enumerate(ends):
                sb = F32(0)
                for t in range(k, kend):
                    if n0 + idx[t] < n:                  # a tap past the end of the signal drops its term
                        sb = fma_exact(x[n0 + idx[t], c], w[t], sb)
                k = kend
                if seg_off is None:
                    out = sb
                else:
                    if apply_gain:
                        sb = round_f32(Fraction(float(sb)) * Fraction(float(seg_gain[seg_off[c] + s])))
                    out = round_f32(Fraction(float(out)) + Fraction(float(sb)))
            y[n0, c] = out
    return y


def _irregular_weights(rng, k):
    return (rng.uniform(-1.5, 1.5, k) * rng.choice([1.0, 1e-3, 7.0], k)).astype(F32)


@pytest.mark.parametrize('n', [0, 1, 2, 17, 60])
def test_convolve_taps_fma_function_path_matches_the_definition(n):
    rng = np.random.default_rng(100 + n)
    # channel 1 has taps past the end for every n here (max index 40 > n for n < 41), channel 2 none
    offsets = np.int32([0, 5, 11, 11, 14])
    idx = np.int32([0, 1, 3, 7, 12, 2, 5, 9, 20, 33, 40, 0, 1, 2])
    w = _irregular_weights(rng, len(idx))
    x = rng.uniform(-1, 1, (n, 4)).astype(F32)
    want = _scalar_fma_conv(x, offsets, idx, w)
    got = O.convolve_taps_fma(x, offsets, idx, w)
    assert got.dtype == np.float32 and got.shape == x.shape and np.array_equal(got, want)
    assert np.array_equal(c_oracle.convolve_fma(x, offsets, idx, w), want)
    if n >= 17:           # it is not the exact arithmetic under another name
        assert not np.array_equal(got, c_oracle.convolve(x, offsets, idx, w))


@pytest.mark.parametrize('n', [0, 1, 30, 70])
def test_convolve_taps_fma_class_path_matches_the_definition(n):
    rng = np.random.default_rng(200 + n)
    # channel 0: two segments; channel 1: pass-through; channel 2: three segments, one of them empty, taps past the end
    offsets = np.int32([0, 6, 6, 13])
    idx = np.int32([0, 3, 8, 1, 4, 50, 2, 6, 11, 29, 45, 65, 5])
    w = _irregular_weights(rng, len(idx))
    seg_off = np.int32([0, 2, 2, 5])
    seg_end = np.int32([3, 6, 9, 9, 13])
    gain = np.float32([0.85, 0.55, 0.35, 0.2, 0.1])
    flags = np.uint8([0, 1, 0])
    x = rng.uniform(-1, 1, (n, 3)).astype(F32)
    for apply_gain in (False, True):
        want = _scalar_fma_conv(x, offsets, idx, w, seg_off, seg_end, gain, flags, apply_gain)
        kw = dict(seg_offsets=seg_off, seg_end=seg_end, seg_gain=gain, chan_flags=flags, apply_gain=apply_gain)
        got = O.convolve_taps_fma(x, offsets, idx, w, **kw)
        assert np.array_equal(got, want), apply_gain
        assert np.array_equal(c_oracle.convolve_fma(x, offsets, idx, w, seg_off=seg_off, seg_end=seg_end, seg_gain=gain,
                                                    chan_flags=flags, apply_gain=apply_gain), want), apply_gain
        assert np.array_equal(got[:, 1], x[:, 1])


def test_convolve_taps_fma_batched_equals_the_loop():
    rng = np.random.default_rng(7)
    offsets, idx = np.int32([0, 3, 7]), np.int32([0, 4, 9, 1, 2, 6, 30])
    w = _irregular_weights(rng, 7)
    x = rng.uniform(-1, 1, (3, 41, 2)).astype(F32)
    got = O.convolve_taps_fma(x, offsets, idx, w)
    assert got.shape == x.shape
    for b in range(3):
        assert np.array_equal(got[b], O.convolve_taps_fma(x[b], offsets, idx, w)), b
    assert np.array_equal(c_oracle.convolve_fma(x, offsets, idx, w, threads=2), got)


def test_non_finite_weights_and_dropped_terms():
    """A tap past the end DROPS its term: were it added as x = 0, an inf weight would make 0 * inf = NaN there."""
    x = np.random.default_rng(3).uniform(-1, 1, (40, 2)).astype(F32)
    x[12, 0] = 0.0
    offsets, idx = np.int32([0, 3, 6]), np.int32([0, 7, 30, 2, 20, 35])
    w = np.float32([0.5, np.inf, -0.25, np.nan, 0.75, -np.inf])
    with np.errstate(invalid='ignore'):
        got = O.convolve_taps_fma(x, offsets, idx, w)
    assert np.array_equal(c_oracle.convolve_fma(x, offsets, idx, w), got, equal_nan=True)
    assert np.isnan(got[5, 0]) and np.count_nonzero(np.isnan(got[:, 0])) == 1     # 0 * inf, where tap 7 reads x[12]
    assert np.all(np.isinf(np.delete(got[:33, 0], 5)))
    assert np.all(np.isfinite(got[33:, 0]))          # only tap 0 reaches these outputs
    assert np.all(np.isnan(got[:38, 1]))             # the NaN weight reaches every output it touches
    assert np.array_equal(got[38:, 1], np.zeros(2, F32))


@SET
@given(fir=sparse_fir(), n=st.integers(0, 400), seed=st.integers(0, 2**31 - 1))
def test_c_and_numpy_fma_oracles_agree_function_path(fir, n, seed):
    rng = np.random.default_rng(seed)
    fir = np.where(fir != 0, fir * rng.uniform(0.3, 1.7, fir.shape).astype(F32), 0).astype(F32)
    x = rng.uniform(-1, 1, (n, fir.shape[1])).astype(F32)
    arr = function_path_arrays(fir)
    got = O.convolve_taps_fma(x, arr.tap_offsets, arr.tap_index, arr.tap_weight)
    assert np.array_equal(c_oracle.convolve_fma(x, arr.tap_offsets, arr.tap_index, arr.tap_weight), got)


@SET
@given(tab=class_table(), n=st.integers(0, 300), seed=st.integers(0, 2**31 - 1))
def test_fma_equals_exact_on_unit_weight_class_tables(tab, n, seed):
    """+-1 weights: x * (+-1) is exact, so fma(x, +-1, acc) is acc +- x rounded once - the exact mode's bits; the segment gain
    and the segment add are separate operations in both."""
    chans, env = tab
    x = np.random.default_rng(seed).uniform(-1, 1, (n, len(chans))).astype(F32)
    arr = class_path_arrays(chans, env, env != (1.0,))
    kw = dict(seg_offsets=arr.seg_offsets, seg_end=arr.seg_end, seg_gain=arr.seg_gain, chan_flags=arr.chan_flags,
              apply_gain=arr.apply_gain)
    got = O.convolve_taps_fma(x, arr.tap_offsets, arr.tap_index, arr.tap_weight, **kw)
    exact = c_oracle.convolve(x, arr.tap_offsets, arr.tap_index, arr.tap_weight, seg_off=arr.seg_offsets,
                              seg_end=arr.seg_end, seg_gain=arr.seg_gain, chan_flags=arr.chan_flags, apply_gain=arr.apply_gain)
    assert np.array_equal(got, exact)
    assert np.array_equal(got, O.class_convolve(x, chans, env, len(chans)))


@SET
@given(fir=sparse_fir(), n=st.integers(1, 400), seed=st.integers(0, 2**31 - 1))
def test_fma_equals_exact_on_unit_weight_function_tables(fir, n, seed):
    fir = np.sign(fir).astype(F32)
    x = np.random.default_rng(seed).uniform(-1, 1, (n, fir.shape[1])).astype(F32)
    arr = function_path_arrays(fir)
    got = O.convolve_taps_fma(x, arr.tap_offsets, arr.tap_index, arr.tap_weight)
    assert np.array_equal(got, O.convolve_taps_scalar(x, arr.tap_offsets, arr.tap_index, arr.tap_weight))
    assert np.array_equal(got, c_oracle.convolve(x, arr.tap_offsets, arr.tap_index, arr.tap_weight))


def test_fma_differs_from_exact_on_the_golden_table(golden):
    """The two arithmetics are distinguishable on the reference's own table (the GPU tests rely on it), and by far less than
    the 1e-6-of-peak tolerance that used to stand for the fma mode."""
    offs, idx, w = O.fir_to_taps(golden.fir('g48k_k30'))
    x = np.random.default_rng(11).uniform(-1, 1, (20011, 2)).astype(F32)
    fma = c_oracle.convolve_fma(x, offs, idx, w)
    assert np.array_equal(fma, O.convolve_taps_fma(x, offs, idx, w))
    exact = c_oracle.convolve(x, offs, idx, w)
    differ = np.count_nonzero(fma != exact)
    gap = float(np.max(np.abs(fma.astype(np.float64) - exact))) / float(np.max(np.abs(exact)))
    assert differ > x.size // 4 and 0 < gap < 1e-6, (differ, gap)

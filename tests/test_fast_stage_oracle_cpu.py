"""CPU tier: the references tests/test_gpu_fast_stage.py holds the fast decorrelate stage to.  ``vnd_oracle.pointwise`` is the
reference's own pointwise steps; ``exact_sum_squares`` is the exact sum of squares rounded once (against ``fractions.Fraction``);
``rms_scale_of_sums`` is the float64-sum normaliser's formula (restated step by step with exact rationals where the step is
rational); and ``rms_scale_bounds`` holds the scale of every simulated device summation whose float32 partials take at most ``k``
squares - in any order, with or without fused multiply-adds - among them inputs built to round every partial the same way."""
from fractions import Fraction

import numpy as np
import pytest

from oracle import vnd_oracle as O

F32 = np.float32


def _fraction_sum_squares(a):
    return [sum((Fraction(float(v)) ** 2 for v in a[:, c]), Fraction(0)) for c in range(a.shape[1])]


def _signals():
    rng = np.random.default_rng(5)
    yield 'uniform', rng.uniform(-1, 1, (3001, 2)).astype(F32)
    mant = rng.uniform(1, 2, (2000, 3))
    yield 'wide_range', (np.ldexp(mant, rng.integers(-70, 60, (2000, 3))) * rng.choice([-1, 1], (2000, 3))).astype(F32)
    yield 'denormal', (rng.uniform(-1, 1, (500, 2)) * 1e-40).astype(F32)
    big = rng.uniform(-1, 1, (1500, 2)).astype(F32)
    big[::97] = F32(3e18)
    yield 'one_dominant_sample_per_run', big
    yield 'one_frame', np.array([[0.5, -3.0]], F32)


@pytest.mark.parametrize('name,x', list(_signals()), ids=lambda v: v if isinstance(v, str) else '')
def test_exact_sum_squares_is_the_exact_sum_rounded_once(name, x):
    got = O.exact_sum_squares(x)
    assert got.dtype == np.float64 and got.shape == (x.shape[1],)
    for c, s in enumerate(_fraction_sum_squares(x)):
        assert got[c] == float(s), (name, c)                  # float(Fraction) rounds correctly


def _scale_by_fractions(sx, sy, n, eps):
    """rms_scale_of_sums restated: the float64 divisions as exact quotients rounded once, the roots as IEEE square roots."""
    import math
    mean_x = F32(float(Fraction(float(sx)) / n))
    mean_y = F32(float(Fraction(float(sy)) / n))
    rms_x = F32(math.sqrt(float(mean_x)))
    rms_y = F32(math.sqrt(float(F32(mean_y + F32(eps)))))
    return F32(float(Fraction(float(rms_x)) / Fraction(float(rms_y))))


@pytest.mark.parametrize('name,x', list(_signals()), ids=lambda v: v if isinstance(v, str) else '')
def test_rms_scale_of_sums_is_the_kernel_formula(name, x):
    rng = np.random.default_rng(len(x))
    y = (x.astype(np.float64) * rng.uniform(0.3, 3.0, x.shape)).astype(F32)
    sx, sy = O.exact_sum_squares(x), O.exact_sum_squares(y)
    got = O.rms_scale_of_sums(sx, sy, len(x))
    assert got.dtype == F32
    for c in range(x.shape[1]):
        assert got[c] == _scale_by_fractions(sx[c], sy[c], len(x), O.RMS_EPS), (name, c)
    # a silent output: the root of eps
    assert O.rms_scale_of_sums(sx[:1], np.zeros(1), len(x))[0] == _scale_by_fractions(sx[0], 0.0, len(x), O.RMS_EPS)


def _device_like(a, k, fused, reverse):
    """A device's sum of squares: float32 partials of k rounded squares each (sequential, optionally backwards, with or without
    an fma per square), the partials added in float64."""
    n, chans = a.shape
    out = np.zeros(chans, np.float64)
    for f0 in range(0, n, k):
        run = a[f0:f0 + k][::-1] if reverse else a[f0:f0 + k]
        acc = np.zeros(chans, F32)
        for row in run:
            acc = O.fma_f32(row, row, acc) if fused else (acc + np.square(row)).astype(F32)
        out += acc.astype(np.float64)
    return out


def _adversarial(k):
    # constant magnitude: every partial sum of k equal squares rounds the same way (1 + 2^-12 squared has bits far below the
    # float32 ulp of its multiples); one dominant sample per run of k; a slow ramp; alternating binades
    n = 40 * k
    yield 'constant_magnitude', np.full((n, 2), F32(1 + 2.0 ** -12)) * np.array([1, -1], F32)
    dom = np.full((n, 2), F32(1.0 + 2.0 ** -11))
    dom[::k] = F32(4096.0 + 1.0)
    yield 'dominant_per_run', dom
    yield 'ramp', np.linspace(1, 1.9, n, dtype=F32)[:, None].repeat(2, axis=1)
    alt = np.ones((n, 2), F32) * F32(1 + 2.0 ** -10)
    alt[1::2] *= F32(3.0)
    yield 'alternating', alt


@pytest.mark.parametrize('k', [16, 32, 64])
def test_rms_scale_bounds_hold_every_partial_summation(k):
    rng = np.random.default_rng(k)
    signals = list(_adversarial(k)) + [('uniform', rng.uniform(-1, 1, (50 * k + 7, 2)).astype(F32))]
    for name, x in signals:
        p = (x.astype(np.float64) * np.float32(0.37) + 0.01).astype(F32)
        n = len(x)
        lo, exact, hi = O.rms_scale_bounds(x, p, k)
        assert np.all(lo <= exact) and np.all(exact <= hi), name
        # the bound is honest but not vacuous: about (k + a few) float32 ulps wide
        assert np.all((hi.astype(np.float64) - lo) / exact <= (2 * k + 8) * 2.0 ** -24), (name, lo, hi)
        for fused in (False, True):
            for reverse in (False, True):
                s = O.rms_scale_of_sums(_device_like(x, k, fused, reverse), _device_like(p, k, fused, reverse), n)
                assert np.all(lo <= s) and np.all(s <= hi), (name, k, fused, reverse, s, lo, hi)


def test_rms_sum_error_is_gamma_k():
    rel, ab = O.rms_sum_error(32, 1000)
    assert 32 * 2.0 ** -24 < rel < 32.01 * 2.0 ** -24 and ab == 1000 * 2.0 ** -149


def test_pointwise_is_the_reference_stage_without_its_normaliser():
    x = np.random.default_rng(3).uniform(-1, 1, (5000, 2)).astype(F32)
    taps = O.generate_class_taps(sample_rate_hz=48000, seed=2)
    conv = O.class_convolve(x, taps, O.DEFAULT_ENVELOPE, 2)
    for mode in ('MS', 'LR'):
        for width in (None, 0.35):
            want = O.decorrelate(x, sample_rate_hz=48000, seed=2, width=width, mode=mode, normalize=False)
            got = O.pointwise(x, conv, mode == 'MS', width)
            assert np.array_equal(got, want), (mode, width)
    assert np.array_equal(O.pointwise(x, conv, False, None), conv)

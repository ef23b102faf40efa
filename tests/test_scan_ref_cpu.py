"""CPU tier of the candidate scan's reference (tests/scan_ref.py): what tests/test_gpu_scan_moments.py takes for granted
about its own inputs, checked where no device is needed."""
import warnings

import numpy as np
import pytest

import scan_ref as S
from oracle import vnd_oracle as O

ENV3 = (1.0, 0.5, 0.25)


def _members(envelope):
    return [S.class_member(0.0, envelope=envelope), S.class_member(1.0, envelope=envelope),
            S.class_member(0.7, filtered=(0, 1), envelope=envelope, seed=5)]


@pytest.mark.parametrize('envelope', [(1.0,), ENV3])
@pytest.mark.parametrize('channels', [1, 2])
def test_integer_samples_make_the_frames_exact(envelope, channels):
    """Tier (a)'s precondition: integer samples in [-3, 3] through +-1 taps and power-of-two gains give frames that are exact
    in float32 in any association - both oracles' float32 frames equal the float64 restatement - as multiples of 1/4."""
    rng = np.random.default_rng(len(envelope) + channels)
    kinds = dict(half_pi=False, pi_folds=False, silent=False)
    for member in _members(envelope):
        for m in (member, S.fir_member(member)):
            for n in (1, 3, 200, 1025):
                y = S.exact_frames(rng.integers(-3, 4, (n, channels)).astype(np.float32), m)
                assert y.dtype == np.float32 and y.shape == (n, 2)
                assert np.array_equal(4 * y, np.round(4 * y)) and np.max(np.abs(y)) <= 90
                for kind, seen in S.theta_kinds(y).items():
                    kinds[kind] |= seen
    assert all(kinds.values()), kinds


def test_general_samples_do_not():
    """... and the check can fail: uniform floats round."""
    x = np.random.default_rng(0).uniform(-1, 1, (500, 2)).astype(np.float32)
    with pytest.raises(AssertionError):
        S.exact_frames(x, S.class_member(0.5, filtered=(0, 1), envelope=ENV3))


def test_function_path_form_is_the_class_fir():
    member = S.class_member(0.3, envelope=ENV3)
    fir = S.fir_member(member)[1]
    assert fir.shape[1] == 2 and fir[0, 1] == 1.0 and np.count_nonzero(fir[:, 1]) == 1       # the pass-through channel
    assert set(np.abs(fir[:, 0][fir[:, 0] != 0])) <= set(ENV3)
    assert S.max_index(S.fir_member(member)) == S.max_index(member)
    arrays = S.bank_arrays([S.fir_member(member), S.fir_member(S.class_member(0.9, envelope=ENV3, filtered=(0, 1), seed=4))])
    assert arrays.num_channels == 4 and arrays.seg_offsets is None
    arrays = S.bank_arrays([member, S.allpass_member()])
    assert arrays.num_channels == 4 and arrays.chan_flags.tolist() == [0, 1, 0, 0]


def test_moments_and_their_bounds():
    rng = np.random.default_rng(5)
    y = rng.uniform(-1, 1, (1000, 2)).astype(np.float32)
    y[10] = 0.0
    y[11, 0] = -y[11, 1]
    m, sums, scale = S.moments64(y), S.term_sums(y), S.scale(y)
    y64 = y.astype(np.float64)
    assert m[5:].tolist() == pytest.approx([np.sum(y64[:, 0] * y64[:, 1]), np.sum(y64[:, 0]**2), np.sum(y64[:, 1]**2)], rel=1e-6)
    assert m[4] == np.float32(np.pi / 2)                                  # L + R = 0: +-pi/2 exactly
    assert np.all(np.abs(m[S.SUMMED]) <= sums[S.SUMMED] * (1 + 1e-12)) and sums[4] == 0.0
    assert np.all(scale[1:4] >= sums[1:4]) and sums[0] == m[0]
    assert np.array_equal(S.moments64(np.zeros((0, 2), np.float32)), np.zeros(8))
    assert S.reorder_bound(1, sums).tolist() == [0.0] * 8 and S.reorder_bound(0, sums).tolist() == [0.0] * 8
    # a reversed sum stays inside the reordering bound
    assert np.all(np.abs(S.moments64(y[::-1]) - m) <= S.reorder_bound(len(y), sums))


@pytest.mark.parametrize('sample', [np.nan, np.inf, -np.inf, 3e38])
def test_the_host_objective_of_a_non_finite_sample_is_nan(sample):
    x = np.random.default_rng(1100).uniform(-1, 1, (1300, 2)).astype(np.float32)
    x[700, 0] = np.float32(sample)
    assert np.array_equal(S.frames(x, S.allpass_member()), x, equal_nan=True)
    with np.errstate(all='ignore'), warnings.catch_warnings():
        warnings.simplefilter('ignore')
        want = S.moments64(x)
        assert np.isnan(O.symmetry_aware_objective(x, angle_limit=np.pi / 4, lambda_mean=5.0, lambda_skew=2.0,
                                                   lambda_correlation=15.0, lambda_penalty=1e3))
    assert not np.all(np.isfinite(want[S.SUMMED]))
    assert np.isfinite(want[7])                                             # R is ordinary: its sum of squares stays finite

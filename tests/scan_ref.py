"""Reference side of the candidate scan's tests (vnd_scan_bank_f32_host): the eight polar moments of a
stereo array as NumPy computes them, the bounds the project holds them to, small banks in both table forms and the
oracle's frames of one candidate.  A plain helper module (no fixtures, no device access of its own): the GPU tiers
import it, tests/test_scan_ref_cpu.py checks it where no device is needed."""
import numpy as np

from oracle import c_oracle
from oracle import vnd_oracle as O

FS, IMPULSES = 48000, 30
MODE_EXACT, MODE_FMA, MODE_FAST = 0, 1, 2          # VND_MODE_* of include/vnd_amd.h


# ---- the reference --------------------------------------------------------------------------------------------------
def _polar(y):
    left, right = y[:, 0], y[:, 1]
    th = np.arctan2(left - right, left + right)
    th = np.where(th < -np.pi / 2, th + np.pi, np.where(th > np.pi / 2, th - np.pi, th))
    r = np.sqrt(left**2 + right**2)
    assert th.dtype == np.float32 and r.dtype == np.float32
    return left, right, th, r


def moments64(y):
    """float32 element maths as NumPy, float64 sums: what the device computes."""
    left, right, th, r = _polar(y)
    d = np.float64
    return np.array([r.sum(dtype=d), (r * th).sum(dtype=d), (r * th**2).sum(dtype=d), (r * (th**2 * th)).sum(dtype=d),
                     np.max(np.abs(th)) if len(th) else 0.0, (left * right).sum(dtype=d), (left * left).sum(dtype=d),
                     (right * right).sum(dtype=d)])


def term_sums(y):
    """Sum of |term| of every summed slot (slot 4, a maximum, gets 0)."""
    left, right, th, r = _polar(y)
    d = np.float64
    return np.array([np.abs(t).sum(dtype=d) for t in (r, r * th, r * th**2, r * (th**2 * th))] + [0.0]
                    + [np.abs(t).sum(dtype=d) for t in (left * right, left * left, right * right)])


def scale(y):
    """The scale of each sum's TERMS that tests/test_gpu_optimization.py's moments test compares on (the odd moments
    cancel): atan2f and NumPy's float32 arctan2 differ by an ulp on some samples."""
    s = moments64(np.abs(y) * np.array([1.0, 0.5], np.float32))
    s[1:4] = moments64(y)[0] * np.array([np.pi / 2, (np.pi / 2) ** 2, (np.pi / 2) ** 3])
    return s


SUM_TOL, THETA_TOL = 3e-8, 2.4e-7          # that test's bounds: per summed slot on max(scale, 1); one float32 ulp on max |theta|
SUMMED = [0, 1, 2, 3, 5, 6, 7]


def reorder_bound(n, sums):
    """Two float64 sums of the same n terms in different orders differ by at most this."""
    return max(n - 1, 0) * 2.0 ** -52 * sums


def theta_kinds(y):
    """Which of the theta edges an array of frames holds: L + R == 0 off silence (atan2 = +-pi/2 exactly), L == R < 0
    (atan2(+-0, negative) = +-pi, which folds to 0) and silence."""
    left, right = y[:, 0], y[:, 1]
    return {'half_pi': bool(np.any((left + right == 0) & (left != 0))), 'pi_folds': bool(np.any((left == right) & (left < 0))),
            'silent': bool(np.any((left == 0) & (right == 0)))}


# ---- banks ----------------------------------------------------------------------------------------------------------
def stereo(x):
    return np.repeat(x, 2, axis=1) if x.shape[1] == 1 else x


def class_member(kappa, *, duration=0.03, filtered=(0,), envelope=(1.0,), seed=1, fs=FS, impulses=IMPULSES):
    """One class-path candidate: the oracle's tap lists of a stereo VelvetNoise and its envelope."""
    env = tuple(envelope)
    taps = O.generate_class_taps(sample_rate_hz=fs, duration_seconds=duration, num_impulses=impulses, segment_envelope=env,
                                 log_distribution_strength=kappa, filtered_channels=filtered, seed=seed)
    return ('class', taps, env)


def allpass_member():
    """Both channels 'filtered' by a single tap of weight 1 at index 0: the frames are the input."""
    return ('class', [[([], [0])], [([], [0])]], (1.0,))


def fir_member(member, fir_len=None):
    """The function-path form of a class-path candidate: its dense (L, 2) float32 FIR (duplicates collapse, last write
    wins, as VelvetNoise.FIR), a pass-through channel as the unit impulse."""
    _, taps, env = member
    top = max([i for segs in taps if segs is not None for neg, pos in segs for i in neg + pos] + [0])
    fir = np.zeros((fir_len or top + 1, 2), np.float32)
    for c, segs in enumerate(taps):
        if segs is None:
            fir[0, c] = 1.0
            continue
        fir[:, c] = O.class_fir([segs], env, len(fir))[:, 0]
    return ('fir', fir)


def max_index(member):
    if member[0] == 'fir':
        return int(np.flatnonzero(np.any(member[1] != 0, axis=1)).max())
    return max(i for segs in member[1] if segs is not None for neg, pos in segs for i in neg + pos)


def bank_arrays(members):
    """The TapArrays of a bank: class-path members or function-path members, not both."""
    from vndecorrelate_amd.taps import class_path_bank_arrays, function_path_arrays
    kinds = {m[0] for m in members}
    assert len(kinds) == 1, 'a bank is class path or function path'
    if kinds == {'fir'}:
        length = max(len(m[1]) for m in members)
        fir = np.zeros((length, 2 * len(members)), np.float32)
        for f, m in enumerate(members):
            fir[:len(m[1]), 2 * f:2 * f + 2] = m[1]
        return function_path_arrays(fir)
    return class_path_bank_arrays([(taps, env, env != (1.0,)) for _, taps, env in members])


def make_bank(ctx, members):
    from vndecorrelate_amd import _native
    arrays = bank_arrays(members)
    if arrays.seg_offsets is None:
        return _native.TapTable.create(ctx, arrays.tap_offsets, arrays.tap_index, arrays.tap_weight)
    return _native.TapTable.create(ctx, arrays.tap_offsets, arrays.tap_index, arrays.tap_weight, **arrays.kwargs())


# ---- the oracle's frames ----------------------------------------------------------------------------------------------
def frames(x, member, mode=MODE_EXACT):
    """The oracle's output of one candidate for the signal x ((n, 1) is replicated to stereo): the reference's own
    convolution in the exact mode (the fast mode has no frames of its own: callers bound it against these), the C
    oracle's fma form in VND_MODE_FMA."""
    from vndecorrelate_amd.taps import class_path_arrays, function_path_arrays
    xs = np.ascontiguousarray(stereo(x), np.float32)
    if len(xs) == 0:
        return np.zeros((0, 2), np.float32)
    if member[0] == 'fir':
        a = function_path_arrays(member[1])
        fn = c_oracle.convolve_fma if mode == MODE_FMA else c_oracle.convolve
        return fn(xs, a.tap_offsets, a.tap_index, a.tap_weight)
    _, taps, env = member
    if mode != MODE_FMA:
        return O.class_convolve(xs, taps, env, 2)
    a = class_path_arrays(taps, env, env != (1.0,))
    return c_oracle.convolve_fma(xs, a.tap_offsets, a.tap_index, a.tap_weight, seg_off=a.seg_offsets, seg_end=a.seg_end,
                                 seg_gain=a.seg_gain, chan_flags=a.chan_flags, apply_gain=a.apply_gain)


def frames64(x, member):
    """The same sum restated in float64, no intermediate rounding to float32."""
    xs = stereo(x).astype(np.float64)
    n = len(xs)
    y = np.zeros((n, 2))

    def add(c, i, w):
        if i < n:
            y[:n - i, c] += w * xs[i:, c]

    if member[0] == 'fir':
        for c in range(2):
            for i in np.flatnonzero(member[1][:, c]):
                add(c, int(i), float(member[1][i, c]))
        return y
    _, taps, env = member
    for c, segs in enumerate(taps):
        if segs is None:
            y[:, c] = xs[:, c]
            continue
        for s, (neg, pos) in enumerate(segs):
            for i in neg:
                add(c, i, -float(env[s]))
            for i in pos:
                add(c, i, float(env[s]))
    return y


def exact_frames(x, member):
    """Tier (a)'s precondition, checked: on this input every product and partial sum of the candidate is exact in
    float32 whatever the association, i.e. the oracle's float32 frames (both arithmetics) ARE the float64 sum."""
    y = frames(x, member, MODE_EXACT)
    y64 = frames64(x, member)
    assert np.array_equal(y.astype(np.float64), y64), 'the input does not make the tap sum exact in float32'
    assert np.array_equal(frames(x, member, MODE_FMA), y), 'the fma arithmetic rounds where the exact one does not'
    # ... in ANY association: integer samples and power-of-two weights make every partial sum a multiple of the smallest
    # weight q, and sum |w| * max |x| < 2^24 q keeps each of them a float32
    if member[0] == 'fir':
        w = [np.abs(member[1][:, c][member[1][:, c] != 0]).astype(np.float64) for c in range(2)]
    else:
        w = [np.array([env_s for s, (neg, pos) in enumerate(segs) for env_s in [float(member[2][s])] * len(neg + pos)])
             for segs in member[1] if segs is not None]
    xs = stereo(x)
    assert np.array_equal(xs, np.round(xs)), 'integer samples'
    for wc in w:
        q = wc.min()
        assert np.all(np.log2(wc) == np.round(np.log2(wc))), 'power-of-two weights'
        assert wc.sum() * float(np.max(np.abs(xs), initial=0.0)) < 2.0 ** 24 * q
    return y

"""SciPy's bounded scalar minimiser for many independent problems in lockstep.

``minimize_scalar(method='bounded')`` (``scipy.optimize._optimize._minimize_scalar_bounded``, Brent's method with
golden-section and parabolic steps) makes exactly one function evaluation per iteration.  So L independent problems
can advance together: each round asks the caller for f at one x per active lane, and lanes that converge (or reach
``maxiter`` evaluations) drop out.  The caller can then score a whole round in one batch - one device launch for the
batched Haas-delay optimiser.

Every step below is a NumPy float64 operation over the active lanes, the same operations in the same order as
SciPy's scalar code: the golden and parabolic steps, ``tol1`` / ``tol2``, ``sign``, the ``maxiter`` cap and the NaN
status.  Lane by lane, ``x``, ``fun``, ``nfev`` and ``status`` equal SciPy's for the same function, bit for bit.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from math import sqrt
from typing import Callable, List

import numpy as np
from numpy.typing import NDArray

_SQRT_EPS = sqrt(2.2e-16)
_GOLDEN_MEAN = 0.5 * (3.0 - sqrt(5.0))


@dataclass
class BoundedLockstepResult:
    """Per lane: the minimiser ``x``, ``fun = f(x)``, ``nfev`` (SciPy's ``nfev`` and ``nit``) and ``status``
    (0 converged, 1 ``maxiter`` evaluations reached, 2 NaN met).  ``evaluations[r]`` is how many lanes round r
    evaluated (round 0 is every lane's first point)."""
    x: NDArray[np.float64]
    fun: NDArray[np.float64]
    nfev: NDArray[np.int64]
    status: NDArray[np.int64]
    evaluations: List[int] = field(default_factory=list)

    @property
    def rounds(self) -> int:
        return len(self.evaluations)


def minimize_bounded_lockstep(fun: Callable[[NDArray[np.int64], NDArray[np.float64]], NDArray],
                              lower, upper, *, xatol: float = 1e-5, maxiter: int = 500) -> BoundedLockstepResult:
    """Minimise L scalar functions, lane l over ``[lower[l], upper[l]]``, as
    ``minimize_scalar(f_l, bounds=(lower[l], upper[l]), method='bounded', options={'xatol': xatol, 'maxiter': maxiter})``
    would one by one.

    ``fun(lanes, x)`` is called once per round with the indices of the active lanes and one float64 abscissa each,
    and returns ``f_lane(x)`` for each as float64."""
    lo = np.array(lower, np.float64).reshape(-1)
    hi = np.array(upper, np.float64).reshape(-1)
    if lo.shape != hi.shape:
        raise ValueError(f'{lo.size} lower bounds for {hi.size} upper bounds')
    if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi))):
        raise ValueError('Optimization bounds must be finite scalars.')
    if np.any(lo > hi):
        raise ValueError('The lower bound exceeds the upper bound.')
    lanes = lo.size
    out = BoundedLockstepResult(x=np.zeros(lanes), fun=np.zeros(lanes), nfev=np.zeros(lanes, np.int64),
                                status=np.zeros(lanes, np.int64))
    if lanes == 0:
        return out

    def call(idx, x):
        f = np.asarray(fun(idx, x), np.float64).reshape(-1)
        if f.shape != x.shape:
            raise ValueError(f'fun returned {f.size} values for {x.size} lanes')
        out.evaluations.append(int(idx.size))
        return f

    with np.errstate(all='ignore'):          # branches are computed on every lane and kept only where SciPy takes them
        a, b = lo.copy(), hi.copy()
        fulc = a + _GOLDEN_MEAN * (b - a)
        nfc, xf = fulc.copy(), fulc.copy()
        rat = np.zeros(lanes)
        e = np.zeros(lanes)
        fx = call(np.arange(lanes), xf.copy())
        num = np.ones(lanes, np.int64)
        fu = np.full(lanes, np.inf)
        ffulc, fnfc = fx.copy(), fx.copy()
        xm = 0.5 * (a + b)
        tol1 = _SQRT_EPS * np.abs(xf) + xatol / 3.0
        tol2 = 2.0 * tol1
        flag = np.zeros(lanes, np.int64)
        active = np.abs(xf - xm) > (tol2 - 0.5 * (b - a))

        while active.any():
            i = np.flatnonzero(active)
            A, B, XF, XM, FX = a[i], b[i], xf[i], xm[i], fx[i]
            NFC, FNFC, FULC, FFULC = nfc[i], fnfc[i], fulc[i], ffulc[i]
            T1, T2, E, RAT = tol1[i], tol2[i], e[i], rat[i]
            # parabolic fit where |e| > tol1
            par = np.abs(E) > T1
            r = (XF - NFC) * (FX - FFULC)
            q = (XF - FULC) * (FX - FNFC)
            p = (XF - FULC) * q - (XF - NFC) * r
            q = 2.0 * (q - r)
            p = np.where(q > 0.0, -p, p)
            q = np.abs(q)
            r = E
            e_par = RAT
            accept = par & (np.abs(p) < np.abs(0.5 * q * r)) & (p > q * (A - XF)) & (p < q * (B - XF))
            rat_par = (p + 0.0) / q
            x_par = XF + rat_par
            near = ((x_par - A) < T2) | ((B - x_par) < T2)
            si = np.sign(XM - XF) + ((XM - XF) == 0)
            rat_par = np.where(near, T1 * si, rat_par)
            # golden-section step everywhere else
            golden = ~accept
            e_gold = np.where(XF >= XM, A - XF, B - XF)
            E = np.where(golden, e_gold, np.where(par, e_par, E))
            RAT = np.where(golden, _GOLDEN_MEAN * e_gold, rat_par)

            si = np.sign(RAT) + (RAT == 0)
            X = XF + si * np.maximum(np.abs(RAT), T1)
            FU = call(i, X)
            NUM = num[i] + 1

            le = FU <= FX
            right = X >= XF
            left = X < XF
            a_new = np.where(le, np.where(right, XF, A), np.where(left, X, A))
            b_new = np.where(le, np.where(right, B, XF), np.where(left, B, X))
            c1 = ~le & ((FU <= FNFC) | (NFC == XF))
            c2 = ~le & ~c1 & ((FU <= FFULC) | (FULC == XF) | (FULC == NFC))
            fulc_new = np.where(le | c1, NFC, np.where(c2, X, FULC))
            ffulc_new = np.where(le | c1, FNFC, np.where(c2, FU, FFULC))
            nfc_new = np.where(le, XF, np.where(c1, X, NFC))
            fnfc_new = np.where(le, FX, np.where(c1, FU, FNFC))
            xf[i] = np.where(le, X, XF)
            fx[i] = np.where(le, FU, FX)
            a[i], b[i] = a_new, b_new
            fulc[i], ffulc[i], nfc[i], fnfc[i] = fulc_new, ffulc_new, nfc_new, fnfc_new
            e[i], rat[i], fu[i], num[i] = E, RAT, FU, NUM

            xm[i] = 0.5 * (a[i] + b[i])
            tol1[i] = _SQRT_EPS * np.abs(xf[i]) + xatol / 3.0
            tol2[i] = 2.0 * tol1[i]
            capped = NUM >= maxiter
            flag[i[capped]] = 1
            active[i] = ~capped & (np.abs(xf[i] - xm[i]) > (tol2[i] - 0.5 * (b[i] - a[i])))

        flag[np.isnan(xf) | np.isnan(fx) | np.isnan(fu)] = 2
    out.x, out.fun, out.nfev, out.status = xf, fx, num, flag
    return out


def round_half_even(values) -> NDArray[np.int64]:
    """Python's ``round(v)`` of each float64 v, as int64: nearest integer, ties to even (``np.rint`` is exact)."""
    return np.rint(np.asarray(values, np.float64)).astype(np.int64)

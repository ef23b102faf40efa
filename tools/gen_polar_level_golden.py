#!/usr/bin/env python3
"""Write tests/golden/polar_level.npz and polar_level_manifest.json from the reference's own code.

Usage:  python tools/gen_polar_level_golden.py <reference checkout>

Runs the reference's ``utils/plot.py`` ``_build_pseudo_hull(np.degrees(thetas), radii, num_bins, p, 0.0, False)`` - the raw
per-slice percentiles ``plot_polar_level`` draws from, for p = 95 (the outline) and p = 50 (the median overlay) - on the polar
sample ``utils/dsp.py`` ``polar_coordinates(L, R, compute_weights=False)`` gives for one float32 and one float64 signal, and
stores the frames and the ``bin_percentile_radii``; the manifest keeps the parameters and the sha256 of every array.  Only
where the reference is present (matplotlib and SciPy, which ``utils/plot.py`` imports, included); under Python 3.10 the
reference is loaded from its unmodified source with the in-memory shim of ``tools/gen_correlogram_golden.py``.

The inputs are drawn so that the last bits of another ``atan2`` cannot move a frame across a slice edge, which makes the
comparison of a device result with this file exact:

* a random frame is redrawn while its NumPy angle in degrees lies within ``MARGIN_ULPS`` ulps of a slice edge.  The ulp is
  that of 180 degrees in the sample type for every edge: the fold ``theta -+ pi`` turns a last-bit error of an angle near
  +-pi into many ulps of the small folded angle, so the margin is absolute, the widest any angle can need;
* frames in [30, 40) degrees are redrawn as well: twenty slices stay empty;
* the planted frames have an angle that is exact in any libm: mono frames of both signs (theta 0: the edge between slices
  179 and 180, and in 180) and anti-phase frames of both signs (-90.0: slice 0; +90.0: the last edge, in no slice).
  Hard-panned frames (+-45 degrees, on an edge) are not planted: ``atan2(l, l)`` is not exact by specification.
"""
from __future__ import annotations

import enum
import hashlib
import json
import pathlib
import sys
import types
import typing

import numpy as np

REPO = pathlib.Path(__file__).resolve().parents[1]
OUT = REPO / 'tests' / 'golden'
NUM_BINS = 360
PERCENTILES = (95.0, 50.0)
FRAMES = 4000
MARGIN_ULPS = 64
EMPTY_DEGREES = (30.0, 40.0)


def load_reference(root: pathlib.Path):
    if not hasattr(enum, 'StrEnum'):
        class StrEnum(str, enum.Enum):
            def __str__(self):
                return str(self.value)
        enum.StrEnum = StrEnum
    if not hasattr(typing, 'Self'):
        typing.Self = typing.TypeVar('Self')
    src = root / 'src' / 'vndecorrelate'

    def load(name, path):
        m = types.ModuleType(name)
        m.__file__ = str(path)
        if path.name == '__init__.py':
            m.__path__ = [str(path.parent)]
        sys.modules[name] = m
        exec(compile(path.read_text(), str(path), 'exec'), m.__dict__)
        return m

    load('vndecorrelate', src / '__init__.py')
    load('vndecorrelate.utils', src / 'utils' / '__init__.py')
    dsp = load('vndecorrelate.utils.dsp', src / 'utils' / 'dsp.py')
    import matplotlib
    matplotlib.use('Agg')
    plot = load('vndecorrelate.utils.plot', src / 'utils' / 'plot.py')
    return dsp, plot


def sha(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def near_an_edge(degrees: np.ndarray, edges: np.ndarray) -> np.ndarray:
    margin = MARGIN_ULPS * float(np.spacing(degrees.dtype.type(180.0)))
    wide = degrees.astype(np.float64)
    nearest = np.abs(wide[:, None] - edges[None, :]).min(axis=1)
    return nearest <= margin


def draw_frames(dsp, dtype, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    edges = np.linspace(-90.0, 90.0, NUM_BINS + 1)
    frames = (rng.standard_normal((FRAMES, 2)) * 0.25).astype(dtype)
    planted = {7: (0.5, 0.5), 8: (-0.125, -0.125), 9: (0.25, -0.25), 10: (-0.25, 0.25), 11: (0.0625, -0.0625),
               FRAMES - 1: (0.75, 0.75)}
    for _ in range(100):
        _, thetas = dsp.polar_coordinates(frames[:, 0], frames[:, 1], compute_weights=False)
        degrees = np.degrees(thetas)
        bad = near_an_edge(degrees, edges) | ((degrees >= EMPTY_DEGREES[0]) & (degrees < EMPTY_DEGREES[1]))
        bad[list(planted)] = False
        if not bad.any():
            break
        frames[bad] = (rng.standard_normal((int(bad.sum()), 2)) * 0.25).astype(dtype)
    else:
        raise SystemExit('the redraw did not settle')
    for at, frame in planted.items():
        frames[at] = frame
    return frames


def main(argv):
    if len(argv) != 2:
        sys.exit(__doc__)
    dsp, plot = load_reference(pathlib.Path(argv[1]).resolve())
    arrays = {}
    manifest = {'numpy': np.__version__, 'num_bins': NUM_BINS, 'percentiles': list(PERCENTILES), 'frames': FRAMES,
                'margin_ulps_of_180_degrees': MARGIN_ULPS, 'empty_degrees': list(EMPTY_DEGREES),
                'call': '_build_pseudo_hull(np.degrees(thetas), radii, num_bins, p, 0.0, False)[3] of '
                        'polar_coordinates(L, R, compute_weights=False)', 'cases': {}}
    for name, dtype, seed in (('f32', np.float32, 21), ('f64', np.float64, 22)):
        frames = draw_frames(dsp, dtype, seed)
        radii, thetas = dsp.polar_coordinates(frames[:, 0], frames[:, 1], compute_weights=False)
        assert radii.dtype == dtype and thetas.dtype == dtype
        degrees = np.degrees(thetas)
        assert degrees[7] == 0 and degrees[8] == 0 and degrees[9] == 90 and degrees[10] == -90 and degrees[11] == 90
        levels = np.stack([plot._build_pseudo_hull(degrees, radii, NUM_BINS, p, 0.0, False)[3] for p in PERCENTILES])
        arrays[f'{name}__frames'] = frames
        arrays[f'{name}__levels'] = levels
        manifest['cases'][name] = {'dtype': np.dtype(dtype).name, 'seed': seed, 'frames_sha256': sha(frames),
                                   'levels_shape': list(levels.shape), 'levels_sha256': sha(levels),
                                   'empty_bins': int((levels[0] == 0).sum()), 'frames_at_plus_90': int((degrees == 90).sum())}
    OUT.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(OUT / 'polar_level.npz', **arrays)
    (OUT / 'polar_level_manifest.json').write_text(json.dumps(manifest, indent=1) + '\n')
    print(f'{len(manifest["cases"])} cases -> {OUT / "polar_level.npz"} ({(OUT / "polar_level.npz").stat().st_size} bytes)')


if __name__ == '__main__':
    main(sys.argv)

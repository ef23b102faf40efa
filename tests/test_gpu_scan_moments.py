"""GPU tier of the single-signal candidate scan (vnd_scan_bank_f32_host): all eight moments of
every row, slot by slot, against a reference of the scan's own operation (tests/scan_ref.py) in every route the entry point
can take.  Every scan of this file first asserts, through TapTable.describe_scan (vnd_describe_scan), the route it means to
run.  T = 2 * nt * r frames is the tile.

Routes, and the cases that reach them (a: frames exactly, b: moments on general input, c: a row depends on its candidate
and the signal only, d: nothing stale is summed, f: non-finite samples and the empty signal):

  fused ordered, exact and FMA, r = 1 (automatic), 2, 4, 8 ........ a b c d f   B30 / F30, stereo
  fused ordered, mono (bc) ...................................... a b c       B30 / F30, mono
  fused fast, r = 2, 4 .......................................... a b c       B30, stereo (r = 1, 3, 6 have no fused instantiation)
  fused fast, r = 8 ............................................. a           B45 (a 45 ms bank: at r = 8 the exchange buffer needs a halo of 2049)
  fused fast at the automatic tile (r = 2) ...................... wide        400 pairs x 4099 frames
  fused fast, mono (bc), r = 2, 4, 8 ............................ a b         B30, mono
  unfused: the nofuse bit (24) .................................. a b c d f
  unfused: cg = 1 (bits 8-11), stereo and mono (plain staging) .. a b      (fast at r = 2, 4, 8 too, where a fused kernel exists and only cg keeps it out)
  unfused: fast nt = 128, 512, 1024 (bits 16-17) ................ a b
  unfused: the direct bit (12) .................................. a b
  unfused: fast r = 1, 3, 6 (no fused instantiation) ............ a b
  unfused: fast r = 8 on B30, r = 2, 4 on Bshort (exchange rule) . a
  unfused: Blong1, stereo (cg falls to 1, the LDS kernels) ...... a (test_long_filters; mono: one plane fits, fused)
  unfused: Blong2 (no tile fits: the direct kernel) ............. a (test_long_filters)
  unfused below and above 64 pairs (by_frame / by_candidate) .... test_wide_banks, c

What the fast mode is held to: tier (a) (exact frames, so exact slots 5-7), the agreement of its routes with each other
(the fused and the plain fast kernels are one template), and the existing score bar - not a moment-level bound against
the oracle's frames (the odd moments are discontinuous at the fold).  The direct kernel keeps the table's association in
every mode, so in the fast mode its rows are held to the FMA oracle instead of to the fast LDS kernels' rows."""
import collections
import re
import warnings

import numpy as np
import pytest

import scan_ref as S
from oracle import vnd_oracle as O

pytestmark = pytest.mark.gpu

EXACT, FMA, FAST = S.MODE_EXACT, S.MODE_FMA, S.MODE_FAST
MODE_NAME = {EXACT: 'exact', FMA: 'fma', FAST: 'fast'}
ENVELOPES = {'class1': (1.0,), 'class3': (1.0, 0.5, 0.25), 'fir3': (1.0, 0.5, 0.25),
             'fir_general': (1.0, 0.7, 0.3)}        # weights that are no powers of two: fma(x, w, acc) rounds once where x * w + acc rounds twice


def V(r=0, cg=0, direct=0, nt=0, nofuse=0):
    """The variant word of vnd_set_variant: bits 0-4 frame pairs per lane, 8-11 channels per workgroup, 12 the direct kernel,
    16-17 the generic fast kernel's threads (1: 128, 2: 512, 3: 1024), 24 the moments as a pass of their own."""
    return r | cg << 8 | direct << 12 | nt << 16 | nofuse << 24


class Route(collections.namedtuple('Route', 'mode variant head conv fields')):
    """One way through the entry point: the mode and variant that ask for it and what vnd_describe_scan must say."""

    def __str__(self):
        return f'{MODE_NAME[self.mode]} variant={self.variant:#x} -> {self.head} {self.conv} {self.fields}'


def route(mode, variant, head, conv, **fields):
    return Route(mode, variant, head, conv, fields)


def parse(text):
    return dict(re.findall(r'(\w+)=(\S+)', text))


def scan(ctx, bank, x, rt):
    """The route's assertion, then - only then - the scan."""
    ctx.set_variant(rt.variant)
    try:
        text = bank.describe_scan(len(x), x.shape[1], rt.mode)
        assert text.startswith(f'{rt.head} {rt.conv} '), f'{rt}: a scan of {x.shape} takes "{text}"'
        got = parse(text)
        for key, value in rt.fields.items():
            assert got[key] == str(value), f'{rt}: a scan of {x.shape} takes "{text}"'
        scan.tile = None if got['direct'] == '1' else 2 * int(got['nt']) * int(got['r'])      # of the scan that follows
        return bank.scan_host(x, rt.mode)
    finally:
        ctx.set_variant(-1)


@pytest.fixture(scope='module')
def ctx():
    from vndecorrelate_amd import _native
    context = _native.default_context()
    assert 'gfx950' in context.info()['name']
    yield context
    context.set_variant(-1)


# ---- banks ------------------------------------------------------------------------------------------------------------
def b30_members(envelope, *, duration=0.03):
    """Five candidates: three with a pass-through channel, two with both channels filtered."""
    return [S.class_member(0.0, envelope=envelope, duration=duration), S.class_member(0.4, envelope=envelope, duration=duration),
            S.class_member(1.0, envelope=envelope, duration=duration),
            S.class_member(0.7, filtered=(0, 1), envelope=envelope, seed=5, duration=duration),
            S.class_member(0.2, filtered=(0, 1), envelope=envelope, seed=9, duration=duration)]


def members_of(kind, **kw):
    members = b30_members(ENVELOPES[kind], **kw)
    return [S.fir_member(m) for m in members] if kind.startswith('fir') else members


def int_signal(rng, n, channels):
    return rng.integers(-3, 4, (n, channels)).astype(np.float32)


# ---- the routes of a small bank (5 pairs: the automatic tile is r = 1, T = 512) -----------------------------------------
def auto_routes(channels):
    fan = '_fanout' if channels == 1 else ''
    bc = 1 if channels == 1 else 0
    routes = [route(EXACT, V(), 'fused', 'conv_ordered' + fan, cg=2, r=1, nt=256, bc=bc, direct=0),
              route(FMA, V(), 'fused', 'conv_ordered' + fan, cg=2, r=1, nt=256, bc=bc, direct=0),
              route(FAST, V(), 'unfused by_frame', 'conv_fast' + fan, cg=2, r=1, nt=256, bc=bc, direct=0)]      # no fused fast r = 1
    for mode in (EXACT, FMA, FAST):
        conv = 'conv_fast' if mode == FAST else 'conv_ordered'
        routes += [route(mode, V(nofuse=1), 'unfused by_frame', conv + fan, cg=2, r=1, bc=bc, direct=0),
                   route(mode, V(cg=1), 'unfused by_frame', conv, cg=1, r=1, bc=0, direct=0),                 # mono: plain staging
                   route(mode, V(direct=1), 'unfused by_frame', 'conv_direct', direct=1)]
    if channels == 2:                                            # (a mono input's fan-out kernels have 256 threads, whatever the bits)
        routes += [route(FAST, V(nt=k), 'unfused by_frame', 'conv_fast', cg=2, nt=nt, bc=0, direct=0)
                   for k, nt in ((1, 128), (2, 512), (3, 1024))]
    return routes


def forced_routes(channels, r, *, fast_fused):
    """The routes at r frame pairs per lane (T = 512 r).  The ordered kernels have r = 1, 2, 4, 8; the fast kernels also 3 and 6,
    but their fused instantiations are r = 2, 4, 8 only, and a stereo one needs a halo of T / 2 + 1 for its exchange buffer."""
    fan = '_fanout' if channels == 1 else ''
    bc = 1 if channels == 1 else 0
    routes = []
    if r in (1, 2, 4, 8):
        routes += [route(mode, V(r=r), 'fused', 'conv_ordered' + fan, cg=2, r=r, nt=256, bc=bc) for mode in (EXACT, FMA)]
        routes += [route(EXACT, V(r=r, nofuse=1), 'unfused by_frame', 'conv_ordered' + fan, cg=2, r=r, bc=bc)]
    else:
        routes += [route(EXACT, V(), 'fused', 'conv_ordered' + fan, cg=2, r=1, bc=bc)]      # the comparison row: the automatic tile
    routes += [route(FAST, V(r=r), 'fused' if fast_fused else 'unfused by_frame', 'conv_fast' + fan, cg=2, r=r, nt=256, bc=bc),
               route(FAST, V(r=r, nofuse=1), 'unfused by_frame', 'conv_fast' + fan, cg=2, r=r, nt=256, bc=bc),
               # one channel per workgroup at a tile whose fused fast kernel exists (r = 2, 4, 8) and is not taken: cg = 2 only
               route(FAST, V(r=r, cg=1), 'unfused by_frame', 'conv_fast', cg=1, r=r, nt=256, bc=0)]
    return routes


# ---- a. frames, exactly ---------------------------------------------------------------------------------------------
def check_exact_case(ctx, bank, members, x, routes, kinds):
    """Tier (a) on one signal: every route's rows against the oracle's frames and against each other."""
    n = len(x)
    rows = [scan(ctx, bank, x, rt) for rt in routes]
    for c, member in enumerate(members):
        y = S.exact_frames(x, member)                        # the precondition, checked on the CPU
        for kind, seen in S.theta_kinds(y).items():
            kinds[kind] |= seen
        want, bound = S.moments64(y), S.reorder_bound(n, S.term_sums(y))
        for rt, got in zip(routes, rows):
            where = f'{rt}, n={n}, candidate {c}'
            assert got[c][5:].tobytes() == want[5:].tobytes(), (where, got[c][5:], want[5:])
            assert got[c][4].tobytes() == rows[0][c][4].tobytes(), (where, got[c][4], rows[0][c][4])
            assert abs(got[c][4] - want[4]) <= S.THETA_TOL, (where, got[c][4], want[4])
            assert np.all(np.abs(got[c][:4] - rows[0][c][:4]) <= bound[:4]), (where, got[c][:4] - rows[0][c][:4], bound[:4])


def all_kinds(kinds):
    assert all(kinds.values()), f'the integer frames miss a theta edge: {kinds}'


@pytest.mark.parametrize('channels', [2, 1])
@pytest.mark.parametrize('kind', ['class1', 'class3', 'fir3'])
def test_frames_exactly_at_the_automatic_tile(ctx, kind, channels):
    """B30 / F30 at T = 512: all lengths (a tile with one live frame, odd lengths, the seams, 200 < the largest tap index)."""
    rng = np.random.default_rng(300 + channels + len(kind))
    members = members_of(kind)
    bank = S.make_bank(ctx, members)
    kinds = collections.defaultdict(bool)
    try:
        assert 1300 < bank.max_index < 1440
        T = 512
        for n in (1, 2, 3, 200, T - 1, T, T + 1, 2 * T + 1):
            check_exact_case(ctx, bank, members, int_signal(rng, n, channels), auto_routes(channels), kinds)
    finally:
        bank.close()
    all_kinds(kinds)


@pytest.mark.parametrize('channels', [2, 1])
@pytest.mark.parametrize('r', [1, 2, 3, 4, 6, 8])
@pytest.mark.parametrize('kind', ['class3', 'fir3'])
def test_frames_exactly_at_forced_tiles(ctx, kind, r, channels):
    """T - 1, T + 1 and 2 T + 1 frames at T = 512 r.  The fast kernel fuses at r = 2, 4 (B30's halo, 1456 frames, is short of the
    2049 that r = 8 needs); a mono input's fused fast kernel has an exchange buffer of its own and fuses at r = 8 too."""
    rng = np.random.default_rng(400 + 10 * r + channels + len(kind))
    members = members_of(kind)
    bank = S.make_bank(ctx, members)
    kinds = collections.defaultdict(bool)
    try:
        T = 512 * r
        fast_fused = r in (2, 4) or (channels == 1 and r == 8)
        for n in (T - 1, T + 1, 2 * T + 1):
            check_exact_case(ctx, bank, members, int_signal(rng, n, channels), forced_routes(channels, r, fast_fused=fast_fused), kinds)
    finally:
        bank.close()
    all_kinds(kinds)


def test_frames_exactly_fused_fast_at_eight_pairs_per_lane(ctx):
    """B45, a 45 ms bank (largest index about 2150): its halo holds the stereo fused fast kernel's exchange buffer at r = 8."""
    rng = np.random.default_rng(45)
    members = members_of('class3', duration=0.045)
    bank = S.make_bank(ctx, members)
    kinds = collections.defaultdict(bool)
    try:
        assert 2050 <= bank.max_index < 2160
        T = 4096
        for n in (T - 1, T + 1, 2 * T + 1):
            check_exact_case(ctx, bank, members, int_signal(rng, n, 2), forced_routes(2, 8, fast_fused=True), kinds)
    finally:
        bank.close()
    all_kinds(kinds)


@pytest.mark.parametrize('r', [0, 2, 4])
def test_frames_exactly_short_bank(ctx, r):
    """Bshort (2 ms: a halo of 256 frames at most): the fused fast kernel's exchange buffer, T / 2 + 1 floats in the halo part of a
    plane, fits at no r, so the fast mode runs unfused at every tile; the ordered kernels fuse."""
    rng = np.random.default_rng(500 + r)
    members = members_of('class3', duration=0.002)
    bank = S.make_bank(ctx, members)
    kinds = collections.defaultdict(bool)
    try:
        assert bank.max_index < 240
        T = 512 * max(r, 1)
        routes = [route(EXACT, V(r=r), 'fused', 'conv_ordered', cg=2, r=max(r, 1)),
                  route(FMA, V(r=r), 'fused', 'conv_ordered', cg=2, r=max(r, 1)),
                  route(FAST, V(r=r), 'unfused by_frame', 'conv_fast', cg=2, r=max(r, 1), nt=256, direct=0),
                  route(EXACT, V(r=r, nofuse=1), 'unfused by_frame', 'conv_ordered', cg=2, r=max(r, 1))]
        for n in (1, 200, T - 1, T + 1, 2 * T + 1):
            check_exact_case(ctx, bank, members, int_signal(rng, n, 2), routes, kinds)
    finally:
        bank.close()
    all_kinds(kinds)


@pytest.mark.parametrize('channels', [2, 1])
@pytest.mark.parametrize('which', ['Blong1', 'Blong2'])
def test_frames_exactly_long_filters(ctx, which, channels):
    """Blong1 (largest index about 25 000: two planes do not fit LDS, so a stereo input's cg falls to 1 and the LDS kernels run
    unfused; a mono input's one plane fits and fuses) and
    Blong2 (about 45 000: no tile fits, the direct kernel), 3 candidates, one length above the largest index and one below."""
    rng = np.random.default_rng(600 + channels + len(which))
    duration = 25000 / S.FS if which == 'Blong1' else 45000 / S.FS
    members = [S.class_member(0.0, duration=duration, envelope=(1.0, 0.5, 0.25)),
               S.class_member(0.1, duration=duration, envelope=(1.0, 0.5, 0.25), filtered=(0, 1), seed=5),
               S.class_member(0.0, duration=duration, envelope=(1.0, 0.5, 0.25), seed=7)]
    bank = S.make_bank(ctx, members)
    kinds = collections.defaultdict(bool)
    try:
        top = bank.max_index
        assert (21000 < top < 25000) if which == 'Blong1' else (41000 < top < 45000)
        if which == 'Blong1' and channels == 2:
            routes = [route(mode, V(), 'unfused by_frame', 'conv_fast' if mode == FAST else 'conv_ordered', cg=1, bc=0, direct=0)
                      for mode in (EXACT, FMA, FAST)]
            routes += [route(FAST, V(r=2), 'unfused by_frame', 'conv_fast', cg=1, r=2, bc=0, direct=0)]      # (a fused fast r = 2 exists: cg keeps it out)
        elif which == 'Blong1':                    # a mono input stages ONE plane, which fits: the fan-out kernels, fused
            routes = [route(EXACT, V(), 'fused', 'conv_ordered_fanout', cg=2, bc=1, direct=0),
                      route(FMA, V(), 'fused', 'conv_ordered_fanout', cg=2, bc=1, direct=0),
                      route(FAST, V(), 'unfused by_frame', 'conv_fast_fanout', cg=2, r=1, bc=1, direct=0),
                      route(FAST, V(r=2), 'fused', 'conv_fast_fanout', cg=2, r=2, bc=1, direct=0),
                      route(EXACT, V(cg=1), 'unfused by_frame', 'conv_ordered', cg=1, bc=0, direct=0)]
        else:
            routes = [route(mode, V(), 'unfused by_frame', 'conv_direct', direct=1) for mode in (EXACT, FMA, FAST)]
        for n in (top + 1000, top - 1000):
            check_exact_case(ctx, bank, members, int_signal(rng, n, channels), routes, kinds)
    finally:
        bank.close()
    all_kinds(kinds)


@pytest.mark.parametrize('pairs,n', [(63, 1025), (64, 1025), (65, 1025), (400, 4099)])
def test_wide_banks(ctx, pairs, n):
    """Three distinct tap lists repeated: the fused sink with many groups per tile, and the unfused reducer on either side of
    64 pairs (lanes along time below, a lane per candidate from 64 on).  400 pairs x 4099 frames fill enough workgroups for
    the planner to pick r = 2 by itself, where the fast kernel fuses."""
    rng = np.random.default_rng(700 + pairs)
    three = [S.class_member(0.3, envelope=(1.0, 0.5, 0.25)), S.class_member(0.9, envelope=(1.0, 0.5, 0.25), seed=2),
             S.class_member(0.6, envelope=(1.0, 0.5, 0.25), filtered=(0, 1), seed=3)]
    bank = S.make_bank(ctx, [three[f % 3] for f in range(pairs)])
    by = 'unfused by_candidate' if pairs >= 64 else 'unfused by_frame'
    routes = [route(EXACT, V(), 'fused', 'conv_ordered', cg=2, pairs=pairs), route(FMA, V(), 'fused', 'conv_ordered', cg=2),
              route(FAST, V(), 'fused', 'conv_fast', cg=2, r=2) if pairs == 400 else route(FAST, V(), by, 'conv_fast', cg=2, r=1),
              route(EXACT, V(nofuse=1), by, 'conv_ordered', cg=2), route(FAST, V(nofuse=1), by, 'conv_fast', cg=2),
              route(EXACT, V(cg=1), by, 'conv_ordered', cg=1)]
    try:
        for channels in (2, 1):
            x = int_signal(rng, n, channels)
            fan = [rt._replace(conv=rt.conv + '_fanout') if channels == 1 and rt.fields.get('cg') == 2 else rt for rt in routes]
            rows = [scan(ctx, bank, x, rt) for rt in fan]
            ys = [S.exact_frames(x, m) for m in three]
            wants, bounds = [S.moments64(y) for y in ys], [S.reorder_bound(n, S.term_sums(y)) for y in ys]
            for rt, got in zip(fan, rows):
                for f in range(pairs):
                    want, bound, first = wants[f % 3], bounds[f % 3], rows[0][f % 3]
                    assert got[f][5:].tobytes() == want[5:].tobytes(), (str(rt), channels, f, got[f][5:], want[5:])
                    assert got[f][4].tobytes() == first[4].tobytes(), (str(rt), channels, f)
                    assert np.all(np.abs(got[f][:4] - first[:4]) <= bound[:4]), (str(rt), channels, f, got[f][:4] - first[:4], bound[:4])
    finally:
        bank.close()


# ---- b. moments, general input --------------------------------------------------------------------------------------
def general_signal(rng, n, channels):
    x = rng.uniform(-1, 1, (n, channels)).astype(np.float32)
    x[n // 2] = 0.0                                   # a silent frame
    if channels == 2:
        x[3, 0] = -x[3, 1]                            # L = -R
    return x


@pytest.mark.parametrize('channels', [2, 1])
@pytest.mark.parametrize('kind', ['class3', 'fir_general'])
def test_moments_on_general_input(ctx, kind, channels):
    """Uniform floats.  Exact and FMA mode: every route's row against moments64 of the oracle's frames at the bounds of
    test_moments_kernel_against_numpy.  Every mode: the routes of one case agree within the float64 reordering bound and
    slot 4 bit for bit - the fast LDS kernels with each other tile size by tile size (fused, plain, 128 to 1024 threads, one
    or two channels per workgroup are one template and give the same frames at the same tile T = 2 nt r; across tile sizes
    the frames differ in rounding, see below); the direct kernel keeps the table's order in the fast mode too and is held
    to the FMA oracle there.  Prints the worst error-to-bound ratios (DESIGN 4 quotes them)."""
    rng = np.random.default_rng(800 + channels + len(kind))
    members = members_of(kind)
    bank = S.make_bank(ctx, members)
    worst = collections.defaultdict(float)
    try:
        for n in (777, 512, 3 * 512 + 5, 1024, 3 * 1024 + 5):          # T and 3 T + 5 at the automatic tile and at r = 2
            x = general_signal(rng, n, channels)
            fan = '_fanout' if channels == 1 else ''
            routes = auto_routes(channels) + forced_routes(channels, 2, fast_fused=True) + [
                route(FAST, V(r=4), 'fused', 'conv_fast' + fan, cg=2, r=4),                          # T = 2048, as 1024 threads at r = 1
                route(FAST, V(r=4, nofuse=1), 'unfused by_frame', 'conv_fast' + fan, cg=2, r=4),
                route(FAST, V(r=3), 'unfused by_frame', 'conv_fast' + fan, cg=2, r=3),
                route(FAST, V(r=3, cg=1), 'unfused by_frame', 'conv_fast', cg=1, r=3)]
            if channels == 2:
                routes += [route(FAST, V(nt=1, cg=1), 'unfused by_frame', 'conv_fast', cg=1, nt=128)]  # T = 256, as 128 threads at cg = 2
            rows = [(rt, scan(ctx, bank, x, rt), scan.tile) for rt in routes]          # (the tile is read after its scan)
            for c, member in enumerate(members):
                ys = {EXACT: S.frames(x, member, EXACT), FMA: S.frames(x, member, FMA)}
                for mode in (EXACT, FMA, FAST):
                    mine = [(rt, got[c], tile) for rt, got, tile in rows if rt.mode == mode]
                    direct = [entry for entry in mine if entry[0].conv == 'conv_direct']
                    if mode == FAST:
                        mine = [entry for entry in mine if entry[0].conv != 'conv_direct']
                    y = ys[FMA if mode == FAST else mode]
                    want, tol = S.moments64(y), S.SUM_TOL * np.maximum(S.scale(y), 1.0)
                    for rt, row, _ in (direct if mode == FAST else mine):
                        where = f'{rt}, n={n}, candidate {c}'
                        assert np.all(np.abs(row - want)[S.SUMMED] <= tol[S.SUMMED]), (where, row, want)
                        assert abs(row[4] - want[4]) <= S.THETA_TOL, (where, row[4], want[4])
                        ratio = float(np.max(np.abs(row - want)[S.SUMMED] / tol[S.SUMMED]))
                        key = 'fast (direct kernel) vs numpy' if mode == FAST else MODE_NAME[mode] + ' vs numpy'
                        worst[key] = max(worst[key], ratio)
                    bound = S.reorder_bound(n, S.term_sums(y) * (1.01 if mode == FAST else 1.0))
                    # the fast mode's frames are a function of the tile: frame T - 1 of a tile sums its odd taps across a wave,
                    # every other frame tap by tap - so its routes agree tile size by tile size, each with a partner
                    groups = collections.defaultdict(list)
                    for rt, row, tile in mine:
                        groups[tile if mode == FAST else 0].append((rt, row))
                    for same in groups.values():
                        assert len(same) >= 2, f'{same[0][0]} has no route of its tile to agree with'
                        for rt, row in same[1:]:
                            where = f'{rt} against {same[0][0]}, n={n}, candidate {c}'
                            assert row[4].tobytes() == same[0][1][4].tobytes(), (where, row[4], same[0][1][4])
                            diff = np.abs(row - same[0][1])
                            assert np.all(diff[S.SUMMED] <= bound[S.SUMMED]), (where, diff, bound)
                            ratio = float(np.max(diff[S.SUMMED] / np.maximum(bound[S.SUMMED], 1e-300)))
                            worst[MODE_NAME[mode] + ' routes'] = max(worst[MODE_NAME[mode] + ' routes'], ratio)
    finally:
        bank.close()
    print('TIER_B', kind, f'channels={channels}', ' '.join(f'{k}: {v:.3f}' for k, v in sorted(worst.items())))


# ---- c. a row depends on its candidate and the signal only ----------------------------------------------------------
@pytest.mark.parametrize('channels', [2, 1])
def test_a_row_depends_on_its_candidate_and_the_signal_only(ctx, channels):
    rng = np.random.default_rng(900 + channels)
    env = (1.0, 0.5, 0.25)
    m = S.class_member(0.55, envelope=env, seed=11)
    others = b30_members(env)
    five = [m, others[0], others[3], m, others[4]]
    fan = '_fanout' if channels == 1 else ''
    x = rng.uniform(-1, 1, (2 * 1024 + 77, channels)).astype(np.float32)
    y = S.frames(x, m)
    bound = S.reorder_bound(len(x), S.term_sums(y) * 1.01)
    bank5, bank1 = S.make_bank(ctx, five), S.make_bank(ctx, [m])
    bank65 = S.make_bank(ctx, [five[f % 5] for f in range(65)])
    try:
        fused = [route(EXACT, V(), 'fused', 'conv_ordered' + fan, cg=2), route(FMA, V(r=4), 'fused', 'conv_ordered' + fan, r=4),
                 route(FAST, V(r=2), 'fused', 'conv_fast' + fan, r=2)]
        for rt in fused:
            a, b = scan(ctx, bank5, x, rt), scan(ctx, bank1, x, rt)
            assert a[0].tobytes() == a[3].tobytes() == b[0].tobytes(), (str(rt), a[0], a[3], b[0])
            assert scan(ctx, bank5, x, rt).tobytes() == a.tobytes(), f'{rt}: two calls, two answers'
            wide = scan(ctx, bank65, x, rt._replace(fields={}))
            assert wide[0].tobytes() == wide[3].tobytes() == wide[60].tobytes() == b[0].tobytes(), str(rt)
        for mode in (EXACT, FAST):
            conv = ('conv_fast' if mode == FAST else 'conv_ordered') + fan
            rt = route(mode, V(nofuse=1), 'unfused by_frame', conv, cg=2)
            a, b = scan(ctx, bank5, x, rt), scan(ctx, bank1, x, rt)
            assert a[0].tobytes() == a[3].tobytes() == b[0].tobytes(), (str(rt), a[0], a[3], b[0])     # both below 64 pairs
            assert scan(ctx, bank5, x, rt).tobytes() == a.tobytes(), f'{rt}: two calls, two answers'
            wide = scan(ctx, bank65, x, rt._replace(head='unfused by_candidate'))
            assert wide[0].tobytes() == wide[3].tobytes() == wide[60].tobytes(), str(rt)               # one kernel: one order
            assert wide[0][4].tobytes() == b[0][4].tobytes()
            assert np.all(np.abs(wide[0] - b[0])[S.SUMMED] <= bound[S.SUMMED]), (str(rt), wide[0] - b[0], bound)
    finally:
        for bank in (bank5, bank1, bank65):
            bank.close()


@pytest.mark.parametrize('channels', [2, 1])
def test_sub_banks_give_the_bits_of_one_launch(ctx, channels):
    """scan_moments with _SCAN_BYTES lowered so that a bank of 9 goes out as 4 + 4 + 1."""
    import vndecorrelate_amd.decorrelation as vnd
    import vndecorrelate_amd.optimization as opt
    from vndecorrelate_amd import _native
    from vndecorrelate_amd.taps import class_path_bank_arrays
    n = 1500
    x = np.random.default_rng(950 + channels).uniform(-1, 1, (n, channels)).astype(np.float32)
    cands = [vnd.VelvetNoise(sample_rate_hz=S.FS, duration_seconds=0.03, num_impulses=30, log_distribution_strength=k,
                             normalizer=None, filtered_channels=(0,), mode='LR', seed=1 + i % 3)
             for i, k in enumerate(np.linspace(0, 1, 9))]
    for count in (9, 4, 1):                                         # the launches' route: fused, whatever the split
        arrays = class_path_bank_arrays([d._tap_member() for d in cands[:count]])
        table = _native.TapTable.create(ctx, arrays.tap_offsets, arrays.tap_index, arrays.tap_weight, **arrays.kwargs())
        try:
            assert table.describe_scan(n, channels, EXACT).startswith('fused conv_ordered')
        finally:
            table.close()
    sig = x[:, 0] if channels == 1 else x
    whole = opt.scan_moments(sig, cands, mode=EXACT)
    old = opt._SCAN_BYTES
    opt._SCAN_BYTES = n * 8 * 4
    try:
        assert max(1, opt._SCAN_BYTES // (n * 8)) == 4
        parts = opt.scan_moments(sig, cands, mode=EXACT)
    finally:
        opt._SCAN_BYTES = old
    assert whole.shape == (9, 8) and parts.tobytes() == whole.tobytes()


# ---- d. nothing stale is summed -------------------------------------------------------------------------------------
@pytest.mark.parametrize('fused', [True, False])
def test_nothing_stale_is_summed(ctx, fused):
    """A scan of an all-NaN signal with more tiles and more pairs leaves NaN in the context's staged input, staged output and
    partials; the case that follows on the same context (another shape) must give the bits of a call on a fresh context."""
    from vndecorrelate_amd import _native
    rng = np.random.default_rng(1000 + fused)
    env = (1.0, 0.5, 0.25)
    members = b30_members(env)
    big = members + members[:4]                                      # 9 pairs against 5
    head = 'fused' if fused else 'unfused by_frame'
    variant = V() if fused else V(nofuse=1)
    fresh_ctx = _native.Context(ctx.device)
    fresh, bank, poison = S.make_bank(fresh_ctx, members), S.make_bank(ctx, members), S.make_bank(ctx, big)
    try:
        for n, n_before in ((777, 3 * 512 + 100), (2 * 512 + 1, 5 * 512 + 3), (1, 1029)):
            x = rng.uniform(-1, 1, (n, 2)).astype(np.float32)
            for rt in (route(EXACT, variant, head, 'conv_ordered', cg=2, r=1),
                       route(FAST, V(r=2) if fused else V(r=2, nofuse=1), head, 'conv_fast', cg=2, r=2)):
                want = scan(fresh_ctx, fresh, x, rt)
                assert np.all(np.isfinite(want))
                nan = np.full((n_before, 2), np.nan, np.float32)
                before = scan(ctx, poison, nan, rt)
                assert np.all(np.isnan(before[:, [0, 1, 2, 3, 5]])), before
                got = scan(ctx, bank, x, rt)
                assert got.tobytes() == want.tobytes(), (str(rt), n, got, want)
    finally:
        for t in (fresh, bank, poison):
            t.close()
        fresh_ctx.close()


# ---- f. non-finite samples and the empty signal ---------------------------------------------------------------------
OBJECTIVE = dict(angle_limit=float(np.pi / 4), lambda_mean=5.0, lambda_skew=2.0, lambda_correlation=15.0, lambda_penalty=1e3)


@pytest.mark.parametrize('sample', [np.nan, np.inf, -np.inf, 3e38])
def test_non_finite_samples(ctx, sample):
    """One bad sample in an ordinary signal through an all-pass candidate (the frames are the input): the summed slots are NaN
    where NumPy's are, equal where NumPy's are infinite, within the usual bounds where finite.  Slot 4 is unspecified for
    a signal with a NaN frame (vnd_amd.h): the device's running maximum drops a NaN theta, np.max propagates it."""
    import vndecorrelate_amd.optimization as opt
    rng = np.random.default_rng(1100)
    member = S.allpass_member()
    bank = S.make_bank(ctx, [member])
    try:
        x = rng.uniform(-1, 1, (1300, 2)).astype(np.float32)
        x[700, 0] = np.float32(sample)
        assert np.array_equal(S.frames(x, member), x, equal_nan=True)
        with np.errstate(all='ignore'), warnings.catch_warnings():
            warnings.simplefilter('ignore')
            want = S.moments64(x)
            host = O.symmetry_aware_objective(x, **OBJECTIVE)
        assert np.isnan(host)
        clean = x.copy()
        clean[700] = 0.0
        tol = S.SUM_TOL * np.maximum(S.scale(clean), 1.0)
        assert not np.all(np.isfinite(want[S.SUMMED]))
        for rt in (route(EXACT, V(), 'fused', 'conv_ordered', cg=2), route(FMA, V(r=2), 'fused', 'conv_ordered', r=2),
                   route(EXACT, V(nofuse=1), 'unfused by_frame', 'conv_ordered', cg=2),
                   route(EXACT, V(direct=1), 'unfused by_frame', 'conv_direct', direct=1),
                   route(FAST, V(r=2), 'unfused by_frame', 'conv_fast', r=2)):       # (a halo of 16 frames: no fused fast kernel)
            got = scan(ctx, bank, x, rt)[0]
            for k in S.SUMMED:
                if np.isnan(want[k]):
                    assert np.isnan(got[k]), (str(rt), k, got, want)
                elif np.isinf(want[k]):
                    assert got[k] == want[k], (str(rt), k, got, want)
                else:
                    assert abs(got[k] - want[k]) <= tol[k], (str(rt), k, got, want)
            if not np.isnan(want[4]):
                assert abs(got[4] - want[4]) <= S.THETA_TOL, (str(rt), got[4], want[4])
            with np.errstate(all='ignore'):
                assert np.isnan(opt.scores_from_moments(got[None], **OBJECTIVE)[0]), (str(rt), got)
    finally:
        bank.close()


@pytest.mark.parametrize('channels', [2, 1])
def test_the_empty_signal_gives_zeros(ctx, channels):
    """n = 0: nothing is convolved, the stand-alone reducer's one chunk sums no frame - eight zeros per pair (vnd_amd.h)."""
    bank = S.make_bank(ctx, b30_members((1.0,)))
    try:
        x = np.zeros((0, channels), np.float32)
        for mode in (EXACT, FAST):
            got = scan(ctx, bank, x, route(mode, V(), 'unfused by_frame', 'conv_none', tiles=0))
            assert got.shape == (5, 8) and got.tobytes() == np.zeros((5, 8)).tobytes()
    finally:
        bank.close()

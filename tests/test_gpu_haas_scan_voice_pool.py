"""GPU tier of the Haas-delay scan voice pool (vnd_haas_scan_voice_stream_*, include/vnd_haas_scan_voice_stream.h;
optimization.HaasScanVoicePool).  The yardstick everywhere is the one-shot vnd_haas_pairs_f64_host on a contiguous copy of
each slot's window, made on the host from the frames the test itself pushed - the entry tests/test_gpu_scan_moments.py and
tests/test_gpu_haas_scan.py pin to the oracle - and every comparison is equality of bytes.

Shapes: 5 slots, W = 2500 (no multiple of the 2048-frame tile, so a wrap falls inside a tile), M = 700, and the delays
{0, 1, 7, 2047, 2048, 2049, 3000} with max_delay = 3000: the largest exceeds the fill of a young voice, fill + d crosses tile
edges, and a slot's seven delays in one block of 16 pairs span 3000 + 2048 > 4096 staged entries: the unstaged route."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

START, END, SWITCH = 1, 2, 4
S, W, M, MAXD = 5, 2500, 700, 3000
DELAYS = np.array([0, 1, 7, 2047, 2048, 2049, 3000], np.int32)
CONFIGS = [(cx, ms, dc, width) for cx in (1, 2) for ms in (False, True) for dc in (0, 1) for width in (None, 0.35)]
STALE = 0x5A                                  # what the state holds before the reset: the rings are never cleared


@pytest.fixture(scope='module')
def ctx():
    from vndecorrelate_amd import _native
    c = _native.default_context()
    assert 'gfx950' in c.info()['name']
    return c


def make_pool(cx, ms=False, dc=0, width=None, *, slots=S, window=W, block=M, max_delay=MAXD):
    """A pool whose state - the rings included - holds STALE bytes before its reset, the same in every run."""
    from vndecorrelate_amd.optimization import HaasScanVoicePool
    pool = HaasScanVoicePool(slots, in_channels=cx, max_frames_per_call=block, window_frames=window, max_delay=max_delay,
                             delayed_channel=dc, ms_mode=ms, width=width)
    pool.reset()
    pool._state[0].fill_(STALE)
    pool.reset()
    return pool


class Model:
    """The host's side of a schedule: the frames of every slot's current voice (the last W are its window) and the state
    the spans predict."""

    def __init__(self, cx, slots=S, window=W, block=M):
        self.cx, self.W, self.M = cx, window, block
        self.voice = [np.zeros((0, cx), np.float32) for _ in range(slots)]
        self.pos, self.fill, self.head = (np.zeros(slots, np.int64) for _ in range(3))

    def push(self, x, counts, flags):
        from vndecorrelate_amd.optimization import haas_scan_voice_spans
        before = self.pos.copy()
        valid, self.pos, self.fill, self.head = haas_scan_voice_spans(self.pos, self.fill, self.head, counts, flags, self.W,
                                                                      self.M)
        for b in np.flatnonzero(valid == 1):
            held = self.voice[b][:0] if flags[b] & START or before[b] == 0 else self.voice[b]
            self.voice[b] = np.concatenate([held, x[b, :counts[b]]])
        return valid

    def window(self, b):
        w = np.ascontiguousarray(self.voice[b][-self.W:] if len(self.voice[b]) else self.voice[b])
        assert len(w) == self.fill[b]
        return w


def push(pool, model, x, counts, flags):
    """One call through process_dev; valid against the spans.  Returns nothing: the state is the result."""
    import torch
    dev = pool._state[0].device
    valid = pool.process_dev(torch.from_numpy(x).to(dev), torch.from_numpy(counts.astype(np.int32)).to(dev),
                             torch.from_numpy(flags.astype(np.int32)).to(dev))
    assert valid.cpu().numpy().tolist() == model.push(x, counts, flags).tolist()


def state_head(pool):
    """(positions, fill, head) as the device holds them (the header's layout: each part padded to 16 bytes)."""
    raw = pool._state[0].cpu().numpy()
    slots = pool.slots
    fill_at = (8 * slots + 15) & ~15
    head_at = fill_at + ((4 * slots + 15) & ~15)
    return (raw[:8 * slots].view(np.int64), raw[fill_at:fill_at + 4 * slots].view(np.int32),
            raw[head_at:head_at + 4 * slots].view(np.int32))


def one_shot(ctx, model, pool, b, delays=DELAYS):
    """The yardstick: the one-shot pairs entry on slot b's window as a contiguous signal."""
    from vndecorrelate_amd import _native
    return _native.haas_pairs_host(ctx, model.window(b)[None], np.zeros(len(delays), np.int32), delays,
                                   delayed_channel=pool.delayed_channel, ms_mode=pool.ms_mode, width=pool.width)


def pairs(pool, slot_idx, delays):
    import torch
    dev = pool._state[0].device
    return pool.pairs_dev(torch.from_numpy(np.asarray(slot_idx, np.int32)).to(dev),
                          torch.from_numpy(np.asarray(delays, np.int32)).to(dev)).cpu().numpy()


def schedule(cx, calls=12, seed=0):
    """About 12 calls.  Slot 0 stays below W; slot 1 is idle throughout; slot 2 wraps more than twice; slot 3 reaches
    exactly W, idles and is ended with an empty call; slot 4 fills the whole ring with a loud voice, then restarts over it
    with a quiet one of a few frames: the loud entries beyond fill would change every byte if they were read."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(calls):
        x = rng.uniform(-1, 1, (S, M, cx)).astype(np.float32)
        counts, flags = np.zeros(S, np.int64), np.zeros(S, np.int64)
        counts[0] = rng.choice([0, 0, 1, 37, 150])
        counts[2] = rng.integers(560, M + 1)
        counts[3] = (700, 700, 700, 400)[i] if i < 4 else 0
        if i < 6:
            counts[4] = M
            x[4] = rng.uniform(50, 100, (M, cx)).astype(np.float32)
        else:
            counts[4] = (300, 0, 1, 0, 699, 0)[i - 6]
        if i == 0:
            flags[[0, 2, 3, 4]] = START
        if i == 6:
            flags[4], flags[3] = START | SWITCH, END
        if i == 9:
            flags[0] = SWITCH                                          # ignored: an idle call stays idle
            counts[0] = 0
        out.append((x, counts, flags))
    return out


# ---- 1. a schedule, every (slot, delay) pair after several of the calls ---------------------------------------------------
@pytest.mark.parametrize('cx, ms, dc, width', CONFIGS)
def test_schedule_against_the_one_shot(ctx, cx, ms, dc, width):
    pool, model = make_pool(cx, ms, dc, width), Model(cx)
    import torch
    delays_dev = torch.from_numpy(DELAYS).to(pool._state[0].device)
    slot_idx, dl = np.repeat(np.arange(S), DELAYS.size), np.tile(DELAYS, S)
    seen = set()
    for i, (x, counts, flags) in enumerate(schedule(cx)):
        push(pool, model, x, counts, flags)
        if i not in (0, 3, 5, 6, 8, 11):
            continue
        pos, fill, head = state_head(pool)
        assert (pos.tolist(), fill.tolist(), head.tolist()) == (model.pos.tolist(), model.fill.tolist(), model.head.tolist())
        want = np.stack([one_shot(ctx, model, pool, b) for b in range(S)])
        got = pairs(pool, slot_idx, dl).reshape(S, DELAYS.size, 8)
        grid = pool.scan_dev(delays_dev)
        assert grid.data_ptr() == pool.scan_dev(delays_dev).data_ptr()                 # the pool's own, at a fixed address
        for b in range(S):
            for k, d in enumerate(DELAYS):
                assert got[b, k].tobytes() == want[b, k].tobytes(), (i, b, int(d), got[b, k], want[b, k])
        assert grid.cpu().numpy().tobytes() == want.tobytes()
        assert np.isfinite(want).all() and want[1].tobytes() == np.zeros((DELAYS.size, 8)).tobytes()   # never started: +0.0
        seen |= {'below' * bool(0 < model.fill[0] < W), 'exact' * bool(model.pos[3] == W),
                 'ended' * bool(i >= 6 and model.pos[3] == 0 and model.fill[3] == W), 'twice' * bool(model.pos[2] > 2 * W),
                 'restarted' * bool(i >= 6 and model.fill[4] < W)}
    assert seen >= {'below', 'exact', 'ended', 'twice', 'restarted'}, seen
    assert model.fill[3] == W and model.pos[3] == 0 and 0 < model.fill[4] < W


# ---- 2. pair order and split -----------------------------------------------------------------------------------------------
def test_pair_order_duplicates_and_splits_give_the_same_rows(ctx):
    pool, model = make_pool(2), Model(2)
    for x, counts, flags in schedule(2, seed=2)[:8]:
        push(pool, model, x, counts, flags)
    slot_idx, dl = np.repeat(np.arange(S), DELAYS.size), np.tile(DELAYS, S)
    rows = pairs(pool, slot_idx, dl)
    rng = np.random.default_rng(3)
    perm = np.concatenate([rng.permutation(slot_idx.size), rng.integers(0, slot_idx.size, 11)])     # shuffled, duplicated
    assert pairs(pool, slot_idx[perm], dl[perm]).tobytes() == rows[perm].tobytes()
    cut = 13                                                                                         # inside a block of 16
    both = np.concatenate([pairs(pool, slot_idx[perm][:cut], dl[perm][:cut]), pairs(pool, slot_idx[perm][cut:], dl[perm][cut:])])
    assert both.tobytes() == rows[perm].tobytes()
    one = pairs(pool, [2], [2049])                                                                   # a call of one pair
    assert one.tobytes() == rows[2 * DELAYS.size + 5].tobytes()


# ---- 3. what is read from device memory and would index something ------------------------------------------------------------
def test_bad_pairs_get_nan_rows_and_the_others_stay(ctx):
    pool, model = make_pool(2, True, 1, 0.35), Model(2)
    for x, counts, flags in schedule(2, seed=4)[:7]:
        push(pool, model, x, counts, flags)
    slot_idx, dl = np.repeat(np.arange(S), DELAYS.size), np.tile(DELAYS, S)
    before = pool._state[0].cpu().numpy().copy()
    clean = pairs(pool, slot_idx, dl)
    bad = [(-1, 5), (S, 5), (0, -1), (0, MAXD + 1), (2 ** 31 - 1, 0), (-2 ** 31, 0), (2, 2 ** 31 - 1), (2, -2 ** 31)]
    at = [0, 3, 3, 16, 17, 20, 35, 35]                                # where they go in: the front, inside runs, the end
    s2, d2 = slot_idx.tolist(), dl.tolist()
    for where, (s, d) in sorted(zip(at, bad), key=lambda t: -t[0]):
        s2.insert(where, s)
        d2.insert(where, d)
    mixed = pairs(pool, s2, d2)
    is_bad = np.array([(s, d) in bad for s, d in zip(s2, d2)])
    assert is_bad.sum() == len(bad) and np.isnan(mixed[is_bad]).all()
    assert mixed[~is_bad].tobytes() == clean.tobytes()
    assert pool._state[0].cpu().numpy().tobytes() == before.tobytes()                 # a scan writes nothing of the state


def test_a_bad_count_touches_nothing(ctx):
    """Slot 2 brings a bad count where the other run leaves it idle: valid = -1 there, and the whole state - positions, fills,
    heads and every ring entry, stale ones included - is the other run's byte for byte."""
    calls = schedule(2, seed=5)[:5]
    states = []
    for bad in (None, -1, M + 1, 2 ** 31 - 1):
        pool, model = make_pool(2), Model(2)
        for i, (x, counts, flags) in enumerate(calls):
            counts = counts.copy()
            if i == 3:
                counts[2] = 0 if bad is None else bad
            push(pool, model, x, counts, flags)                        # (valid against the spans: -1 for the bad count)
        states.append((pool._state[0].cpu().numpy().tobytes(), pairs(pool, np.repeat(np.arange(S), 7), np.tile(DELAYS, S)).tobytes()))
    assert all(s == states[0] for s in states[1:])


def test_a_state_that_was_never_reset_gives_nan_rows(ctx):
    """A fill outside [0, W] or a head outside [0, W) - planted here, as a state that was never reset would hold them - is
    a row of NaN for that slot's pairs; nothing is addressed with it and the neighbours' rows stay."""
    pool, model = make_pool(1), Model(1)
    for x, counts, flags in schedule(1, seed=6)[:4]:
        push(pool, model, x, counts, flags)
    slot_idx, dl = np.repeat(np.arange(S), DELAYS.size), np.tile(DELAYS, S)
    clean = pairs(pool, slot_idx, dl).reshape(S, DELAYS.size, 8)
    import torch
    fill_at = (8 * S + 15) & ~15
    head_at = fill_at + ((4 * S + 15) & ~15)
    words = pool._state[0][:head_at + 4 * S].view(torch.int32)
    for word, value in ((fill_at // 4 + 0, W + 1), (fill_at // 4 + 2, -1), (head_at // 4 + 3, W), (head_at // 4 + 4, -7)):
        words[word] = value
    got = pairs(pool, slot_idx, dl).reshape(S, DELAYS.size, 8)
    assert np.isnan(got[[0, 2, 3, 4]]).all() and got[1].tobytes() == clean[1].tobytes()


# ---- 4. optimize against the batched optimiser -------------------------------------------------------------------------------
def test_optimize_equals_the_batched_optimiser(ctx):
    import contextlib
    import io
    from vndecorrelate_amd import optimization
    fs, seconds, window, block, slots = 48000, 0.02, 4800, 1200, 3
    pool = optimization.haas_scan_voice_pool(slots, in_channels=2, max_frames_per_call=block, window_frames=window,
                                             max_delay_seconds=seconds, sample_rate_hz=fs)
    assert pool.max_delay == 960
    pool.reset()
    model = Model(2, slots, window, block)
    rng = np.random.default_rng(7)
    for i in range(5):                                                # 6000 frames a slot: full windows, wrapped once
        common = rng.normal(0, 0.2, (slots, block, 1))
        x = (common * [1.0, 0.6] + rng.normal(0, 0.1, (slots, block, 2))).astype(np.float32)
        push(pool, model, x, np.full(slots, block), np.full(slots, START if i == 0 else 0))
    windows = np.stack([model.window(b) for b in range(slots)])
    assert windows.shape == (slots, window, 2)
    optimization.set_haas_scan_device(True)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            want = optimization.optimize_haas_delay_batched(input_signals=windows, sample_rate_hz=fs, max_delay_seconds=seconds,
                                                            grid_size=40)
        stats = optimization.last_haas_search
    finally:
        optimization.set_haas_scan_device(None)
    got = pool.optimize(grid_size=40)
    assert stats.route == 'device' and got.dtype == np.float64 and got.shape == (slots,)
    assert got.tobytes() == want.tobytes(), (got, want)
    assert pool.last_search.pairs_per_round == stats.pairs_per_round and pool.last_search.rounds == stats.rounds
    assert pool.optimize([2, 0], grid_size=40).tobytes() == want[[2, 0]].tobytes()


# ---- 5. push, scan, scores, argmin and the fading pool's switch in one graph ---------------------------------------------------
def test_the_loop_closes_in_one_graph(ctx):
    """push -> scan_dev -> scores -> argmin -> HaasFadeVoicePool.process_dev with VOICE_SWITCH, captured once on one stream
    (a linear chain) and replayed over three calls with new contents in the fixed inputs, equals the uncaptured calls."""
    import torch
    from vndecorrelate_amd.optimization import HaasScanVoicePool
    from vndecorrelate_amd.streaming import HaasFadeVoicePool, fade_gains
    dev = torch.device('cuda', ctx.device)
    slots, block, window, maxd, fade = 4, 256, 600, 64, 48
    grid = np.array([0, 3, 9, 17, 30, 47, 64], np.int32)
    rng = np.random.default_rng(8)
    calls = []
    for i in range(3):
        counts = rng.integers(100, block + 1, slots).astype(np.int32)
        flags = np.full(slots, START if i == 0 else SWITCH, np.int32)
        if i == 1:
            counts[1], flags[1] = 0, 0                                 # an idle slot in both pools
        common = rng.normal(0, 0.3, (slots, block, 1))
        calls.append(((common * [1.0, -0.5] + rng.normal(0, 0.1, (slots, block, 2))).astype(np.float32), counts, flags))

    def run(replayed):
        meter = HaasScanVoicePool(slots, in_channels=2, max_frames_per_call=block, window_frames=window, max_delay=maxd)
        pool = HaasFadeVoicePool(np.array([maxd], np.int32), slots=slots, in_channels=2, max_frames_per_call=block,
                                 delayed_channel=0, ms_mode=False, fade_frames=fade, fade_gains=fade_gains(fade))
        meter.reset()
        pool.reset()
        x = torch.zeros((slots, block, 2), dtype=torch.float32, device=dev)
        counts, flags, oc = (torch.zeros(slots, dtype=torch.int32, device=dev) for _ in range(3))
        y = torch.zeros((slots, pool.row_frames, 2), dtype=torch.int64, device=dev)
        delays = torch.from_numpy(grid).to(dev)
        chosen = torch.zeros(slots, dtype=torch.int32, device=dev)
        meter.scan_dev(delays)                                         # the grid's pair arrays: allocated before the capture

        def step():
            valid = meter.process_dev(x, counts, flags)
            moments = meter.scan_dev(delays)
            chosen.copy_(delays[meter.scores(moments).argmin(-1)])
            pool.process_dev(x, counts, flags, chosen, out=(y.view(torch.float64), oc))
            return valid, moments
        meter.reset()                                                  # (the warm scan read an empty state; start clean)
        if replayed:
            graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream(dev)
            with torch.cuda.graph(graph, stream=side):
                valid, moments = step()
            torch.cuda.synchronize(dev)
            meter.reset()                                              # what the capture's warm-up may have left
            pool.reset()
        results = []
        for xh, ch, fh in calls:
            for t, v in ((x, xh), (counts, ch), (flags, fh)):
                t.copy_(torch.from_numpy(v))
            y.fill_(-1)
            if replayed:
                graph.replay()
            else:
                valid, moments = step()
            torch.cuda.synchronize(dev)
            n = oc.cpu().numpy()
            results.append((valid.cpu().numpy().tobytes(), moments.cpu().numpy().tobytes(), chosen.cpu().numpy().tobytes(),
                            n.tobytes(), pool.fade_left_dev.cpu().numpy().tobytes(),
                            b''.join(y[b, :max(int(n[b]), 0)].cpu().numpy().tobytes() for b in range(slots))))
        return results, chosen.cpu().numpy()

    plain, picked = run(False)
    again, _ = run(True)
    assert len(plain) == len(calls) == 3
    for i, (a, b) in enumerate(zip(plain, again)):
        assert a == b, f'call {i}: the replay differs from the uncaptured call'
    assert set(picked.tolist()) <= set(grid.tolist())

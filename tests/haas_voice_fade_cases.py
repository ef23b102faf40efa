"""What the two tiers of the crossfading Haas and chain voice pools share (tests/test_haas_voice_fade_pool_cpu.py,
tests/test_gpu_haas_voice_fade_pool.py): the per-slot block of include/vnd_haas_voice_fade_stream.h restated in Python
integers, the tail counted frame by frame, the expected output of a voice in NumPy float64 from the oracle's own steps, and
ragged schedules with switches whose cases are counted from the restatement alone.  Nothing here touches a GPU or the
package's own mirror."""
import numpy as np

START, END, SWITCH = 1, 2, 4
MAX_POSITION = 1 << 60
# the GPU tier's shapes: a row of M + D = 700 frames spans three 256-lane tiles, and a fade of F = 200 crosses calls
RAGGED = dict(seed=0, lengths_seed=0, shape=dict(slots=6, M=300, D=400, F=200),
              delays=(0, 1, 7, 150, 399, 400),
              cases=('longer', 'shorter', 'from_zero', 'to_zero', 'from_max', 'to_max', 'same', 'crosses_call', 'tail_cur',
                     'tail_old', 'tail_between', 'refused', 'switch_on_fresh', 'switch_alone', 'start_over_fade', 'accepted'),
              # a fade begins at a call's first frame and goes on at the next call's first: its frames are a row's first, so
              # it crosses a 256-lane tile only with F > 256 - the lengths test's F = 700
              long_cases=('crosses_tile', 'crosses_call', 'refused', 'accepted', 'longer', 'shorter', 'switch_on_fresh'))


def one_slot(pos, rec, count, flags, delay, D, F, M):
    """include/vnd_haas_voice_fade_stream.h, "one call, per slot b", in Python integers: ``(out_count, new position, new
    record (s, old, cur), fade_left, accepted)``."""
    pos, count, flags, delay = int(pos), int(count), int(flags), int(delay)
    rec = tuple(int(v) for v in rec)
    fresh = bool(flags & START) or pos == 0
    p = 0 if fresh else pos
    alone = (-1, pos, rec, -1, False)                                  # a bad slot: nothing of it changes
    if not 0 <= count <= M or not 0 <= p <= MAX_POSITION:
        return alone
    if not (count > 0 or flags & (START | END | SWITCH)):              # idle: nothing changes, the delay is not looked at
        return 0, pos, rec, (0 if fresh else min(F, max(0, rec[0] + F - p))), False
    accept = False
    if fresh:
        if not 0 <= delay <= D:
            return alone
        s, old, cur = -F, delay, delay
    else:
        s, old, cur = rec
        if not (0 <= old <= D and 0 <= cur <= D):                      # a record no call of the pool wrote
            return alone
        accept = bool(flags & SWITCH) and p >= s + F
        if accept:
            if not 0 <= delay <= D:
                return alone
            s, old, cur = p, cur, delay
    end, e = bool(flags & END), p + count
    tail = max(cur, min(old, max(0, s + F - e)))
    return count + (tail if end else 0), (0 if end else e), (s, old, cur), (0 if end else min(F, max(0, s + F - e))), accept


def tail_by_count(F, old, cur, e, s):
    """The frames at and past e to which either delay still contributes, counted one by one, with the input taken as
    present at every frame below e: frame t takes the old delay while t < s + F and the new one from s on."""
    last = e
    for t in range(e, e + max(old, cur) + F + 2):
        reads = ([t - old] if t < s + F else []) + ([t - cur] if t >= s else [])
        if any(f < e for f in reads):
            last = t + 1
    return last - e


def haas_fade(x, delay, fades, gains, F, frames, *, delayed_channel, ms_mode, width):
    """A voice's whole output, float64 ``(frames, 2)``: the oracle's haas_effect step by step - the float32 signal widened
    into a zero-padded float64 buffer, lr_to_ms, the delayed column shifted with zeros filled in, ms_to_lr and the mono
    compensation, apply_stereo_width - with the blend between the shift and the decode.  ``x`` is float32 ``(n, cx)``,
    ``delay`` the delay the voice starts with, ``fades`` its accepted switches ``(s, old, cur)`` in order."""
    from oracle import vnd_oracle as O
    n, mono = len(x), x.shape[1] == 1
    assert x.dtype == np.float32 and frames >= n
    y = np.zeros((frames, 2))
    y[:n] = np.column_stack((x[:, 0], x[:, 0])) if mono else x
    if ms_mode and not mono:
        O.lr_to_ms(y)
    column = y[:n, delayed_channel].copy()

    def shifted(d):                                                    # frame t reads t - d; zeros outside [0, n)
        out = np.zeros(frames)
        k = max(0, min(n, frames - d))
        out[d:d + k] = column[:k]
        return out
    out = shifted(delay)
    for s, old, cur in fades:
        a, b = shifted(old), shifted(cur)
        out[min(frames, s + F):] = b[min(frames, s + F):]
        k = max(0, min(F, frames - s))
        if k:
            out[s:s + k] = a[s:s + k] * gains[0][:k].astype(np.float64) + b[s:s + k] * gains[1][:k].astype(np.float64)
    y[:, delayed_channel] = out
    if ms_mode:
        O.ms_to_lr(y)
        if mono:
            y *= 0.5
    if width is not None:
        O.apply_stereo_width(y, width)
    return y


class FadeVoice:
    """One voice of a schedule: its signal, the delay it starts with, and what the restatement says happened to it."""

    def __init__(self, x, delay):
        self.x, self.delay = x, int(delay)
        self.fades, self.out, self.pushed, self.frames, self.dropped = [], [], 0, 0, False

    def result(self):
        return np.concatenate(self.out) if self.out else np.zeros((0, 2), np.float64)


def ragged_schedule(seed, *, slots, M, D, F, delays, cx=2, calls=60):
    """``(calls, voices, counted)``: ``calls`` is a list of ``(blocks, counts, flags, delays)``; ``voices`` is
    ``{slot: [FadeVoice, ...]}`` in order, slots reused after END or started over; ``counted`` holds, from the restatement
    alone, how often each case the GPU test must meet occurs."""
    rng = np.random.default_rng(seed)
    sizes = (0, 1, 7, 64, M - 1, M)
    pos, rec, left = [0] * slots, [(0, 0, 0)] * slots, [0] * slots
    live = [None] * slots
    slot_delays = np.zeros(slots, np.int32)
    voices = {b: [] for b in range(slots)}
    counted = {case: 0 for case in RAGGED['cases'] + RAGGED['long_cases']}
    out, i = [], 0
    while i < calls or any(v is not None for v in live):
        last = i >= calls                                              # closing: no new voice, whole blocks, END when done
        i += 1
        assert i < calls + 30
        blocks, counts, flags = {}, np.zeros(slots, np.int32), np.zeros(slots, np.int32)
        for b in range(slots):
            v = live[b]
            over = v is not None and left[b] > 0 and not last and rng.random() < 0.08
            if over:                                                   # START over a fading voice: it is dropped, unflushed
                counted['start_over_fade'] += 1
                v.dropped, v = True, None
            if v is None:
                if last or (not over and rng.random() < 0.4):
                    continue
                n_total = int(rng.choice([1, 200, 900, 1500]))
                x = np.random.default_rng([seed, i, b]).uniform(-1, 1, (n_total, cx))
                v = live[b] = FadeVoice(x.astype(np.float32), rng.choice(delays))
                v.wanted = int(rng.integers(0, 4))
                voices[b].append(v)
                flags[b] |= START
                slot_delays[b] = v.delay
                if rng.random() < 0.3:                                 # a SWITCH on a fresh slot: ignored, the delay is START's
                    flags[b] |= SWITCH
            rest = len(v.x) - v.pushed
            n = min(rest, int(rng.choice(sizes)))
            if last:
                n = min(rest, M)
            if n:
                blocks[b] = v.x[v.pushed:v.pushed + n]
            counts[b] = n
            v.pushed += n
            if not flags[b] & START and v.wanted and rng.random() < 0.5:
                flags[b] |= SWITCH
                slot_delays[b] = int(rng.choice(delays)) if left[b] == 0 else D + 1 + int(rng.integers(5))   # refused: not read
            if v.pushed == len(v.x) and (last or rng.random() < 0.5):
                flags[b] |= END
        for b in range(slots):
            v = live[b]
            fresh = bool(flags[b] & START) or pos[b] == 0
            before, p = rec[b], (0 if fresh else pos[b])
            n_out, pos[b], rec[b], new_left, accept = one_slot(pos[b], rec[b], counts[b], flags[b], slot_delays[b], D, F, M)
            assert n_out >= 0
            if v is None:
                continue
            s, old, cur = rec[b]
            if fresh:
                v.delay = cur                                          # (a voice that has pushed nothing yet begins again)
            if flags[b] & SWITCH:
                if fresh:
                    counted['switch_on_fresh'] += 1
                elif accept:
                    v.fades.append(rec[b])
                    v.wanted -= 1
                    for case, hit in (('accepted', True), ('longer', cur > old), ('shorter', cur < old), ('same', cur == old),
                                      ('from_zero', old == 0 and cur), ('to_zero', cur == 0 and old), ('from_max', old == D and cur < D),
                                      ('to_max', cur == D and old < D), ('switch_alone', counts[b] == 0 and not flags[b] & END)):
                        counted[case] += bool(hit)
                else:
                    counted['refused'] += 1
                    assert left[b] > 0 and rec[b] == before
            e = p + int(counts[b])
            if F and n_out > 0 and max(p, s) < min(p + n_out, s + F):  # this call returns blended frames
                counted['crosses_call'] += new_left > 0
                lo, hi = max(p, s) - p, min(p + n_out, s + F) - 1 - p
                counted['crosses_tile'] += lo // 256 != hi // 256
            if flags[b] & END and s + F - e > 0:                       # a fade cut by END: the three branches of the tail
                r = s + F - e
                counted['tail_cur' if cur >= min(old, r) else ('tail_old' if old <= r else 'tail_between')] += 1
            v.frames += n_out
            left[b] = new_left
            if flags[b] & END:
                live[b] = None
        out.append((blocks, counts.copy(), flags.copy(), slot_delays.copy()))
    assert all(v is None for v in live)
    return out, voices, counted


# ---- the chain pool: a velvet fade stage (tests/voice_fade_cases.py's restatement), then the Haas fade stage -------------
CHAIN = dict(seed=0, kappas=(0.0, 0.3, 0.55, 1.0), delays=(0, 100, 250, 400),
             cases=('both', 'fresh_corner', 'reused', 'held_back'))


class ChainVoice:
    """One voice of a chain schedule, with what the two restatements say happened to it in each stage."""

    def __init__(self, x, entry, slot):
        self.x, self.entry, self.slot = x, entry, slot
        self.table, self.fades1, self.delay, self.fades2, self.out, self.pushed, self.frames = 0, [], 0, [], [], 0, 0


def chain_step(state, v, count, flags, table, delay, *, M, D, F, H):
    """Both restatements on one slot's call of the dict form - stage 2's count is stage 1's answer, both get the flags:
    ``(n_out, fade_left, accepted by stage 1, accepted by stage 2, stage 2 fresh with work)``;
    ``state`` = ``[(position, record), (position, record)]`` is moved on, and the voice notes its tables, delays and fades."""
    from voice_fade_cases import one_slot as velvet_slot
    (p1, r1), (p2, r2) = state
    fresh1, fresh2 = bool(flags & START) or p1 == 0, bool(flags & START) or p2 == 0
    mid, p1, r1, left1, _, accept1 = velvet_slot(p1, r1, count, flags, table, H, F, M)
    n_out, p2, r2, left2, accept2 = one_slot(p2, r2, mid, flags, delay, D, F, M + H)
    assert mid >= 0 and n_out >= 0
    if fresh1:
        v.table = r1[1]
    elif accept1:
        v.fades1.append(r1)
    fresh2 = fresh2 and (mid > 0 or flags != 0)
    if fresh2:
        v.delay = r2[2]
    elif accept2:
        v.fades2.append(r2)
    state[0], state[1] = (p1, r1), (p2, r2)
    return n_out, max(left1, left2), accept1, accept2, fresh2


def chain_schedule(seed, *, slots, M, D, F, H, tables, delays, cx=2, calls=45):
    """``(calls, voices, counted)`` for the dict form of a chain pool: ``calls`` is a list of ``(blocks, start, end, switch,
    {slot: frames that come back}, fade_left after the call)``; a switch is asked wherever fade_left allows one.  (An END
    returns the velvet stage's H > F last frames: no chain voice ends inside a fade; the Haas pool's schedule has those.)"""
    rng = np.random.default_rng(seed)
    live, left = [None] * slots, [0] * slots
    states = [[(0, (0, 0, 0)), (0, (0, 0, 0))] for _ in range(slots)]
    voices, out, counted, call = [], [], {case: 0 for case in CHAIN['cases']}, 0
    while call < calls or any(v is not None for v in live):
        closing = call >= calls
        call += 1
        assert call < calls + 30
        blocks, start, end, switch, step, answers = {}, {}, [], {}, {}, {}
        for b in range(slots):
            v = live[b]
            if v is None:
                if closing or rng.random() < 0.4:
                    continue
                x = np.random.default_rng([seed, call, b]).uniform(-1, 1, (int(rng.choice([1, 200, 900, 1500])), cx))
                counted['reused'] += any(w.slot == b for w in voices)
                v = live[b] = ChainVoice(x.astype(np.float32), int(rng.integers(len(tables))), b)
                voices.append(v)
                start[b] = v.entry
            n = min(len(v.x) - v.pushed, M if closing else int(rng.choice([0, 1, 7, 64, M - 1, M])))
            blocks[b] = v.x[v.pushed:v.pushed + n]
            v.pushed += n
            flags = START if b in start else 0
            if b not in start and rng.random() < 0.5:
                if left[b] == 0:
                    v.entry = switch[b] = int(rng.integers(len(tables)))
                    flags |= SWITCH
                else:
                    counted['held_back'] += 1                          # the dict form refuses it: not asked
            if v.pushed == len(v.x) and (closing or rng.random() < 0.5):
                end.append(b)
                flags |= END
            step[b] = (n, flags)
        for b, (n, flags) in step.items():
            v = live[b]
            n_out, left[b], accept1, accept2, fresh2 = chain_step(states[b], v, n, flags, int(tables[v.entry]),
                                                                  int(delays[v.entry]), M=M, D=D, F=F, H=H)
            answers[b] = n_out
            v.frames += n_out
            counted['both'] += bool(flags & SWITCH) and accept1 and accept2
            counted['fresh_corner'] += bool(flags & SWITCH) and accept1 and fresh2
            if flags & END:
                live[b] = None
        out.append((blocks, start, end, switch, answers, list(left)))
    return out, voices, counted

"""What the two tiers of the crossfading voice pool share (tests/test_voice_fade_pool_cpu.py,
tests/test_gpu_voice_fade_pool.py): the header's per-slot block restated in Python integers, the expected output of a voice
from per-table convolutions, and ragged schedules with switches whose properties are counted from the restatement alone.
Nothing here touches a GPU or the package's own mirror."""
import numpy as np

START, END, SWITCH = 1, 2, 4
MAX_POSITION = 1 << 60
# the GPU tier's ragged schedule: the shapes of tests/test_gpu_voice_pool.py (H: bank_latency()) and a seed at which every
# case of test 2 occurs - tests/test_voice_fade_pool_cpu.py counts them without a GPU
RAGGED = dict(seed=2, lengths_seed=20, shape=dict(slots=6, M=600, F=200, T=5, cx=2),
              cases=('row_past_512', 'crosses_call', 'cut_by_end', 'refused', 'switch_on_fresh', 'accepted'),
              long_cases=('crosses_512', 'tile_inside', 'three_calls', 'crosses_call', 'cut_by_end', 'refused', 'accepted'))


def bank_latency():
    """H of the small bank of tests/test_gpu_voice_pool.py, from its tap arrays alone."""
    from oracle import vnd_oracle as O
    from test_gpu_each_stream import _members
    from vndecorrelate_amd.taps import class_path_bank_arrays
    return int(class_path_bank_arrays(_members(O.DEFAULT_ENVELOPE, (0,))).tap_index.max())


def one_slot(pos, rec, count, flags, table, H, F, M):
    """include/vnd_voice_fade_stream.h, "one call, per slot b", in Python integers: ``(out_count, new position, new record
    (s, old, cur), fade_left, E, accepted)``."""
    pos, count, flags, table = int(pos), int(count), int(flags), int(table)
    fresh = bool(flags & START) or pos == 0
    p = 0 if fresh else pos
    if not 0 <= count <= M or not 0 <= p <= MAX_POSITION:
        return -1, pos, tuple(int(v) for v in rec), -1, None, False
    end = bool(flags & END)
    E = max(0, p - H)
    E1 = p + count if end else max(0, p + count - H)
    s, old, cur = (-F, table, table) if fresh else (int(v) for v in rec)
    accept = bool(flags & SWITCH) and not fresh and E >= s + F
    if accept:
        s, old, cur = E, cur, table
    return E1 - E, (0 if end else p + count), (s, old, cur), (0 if end else min(F, max(0, s + F - E1))), E, accept


def blend(conv, first_table, fades, gains, F):
    """The convolved output of one voice: ``conv[t]`` is float32 ``(N, 2)``, its whole signal through table ``t`` alone
    (a table that is not in ``conv`` is outside the bank: NaN); ``fades`` the accepted switches ``(s, old, cur)`` in order.
    NumPy float32: two rounded products and one rounded sum per blended sample."""
    N = len(next(iter(conv.values())))
    nan = np.full((N, 2), np.nan, np.float32)
    out = conv.get(first_table, nan).copy()
    for s, old, cur in fades:
        a, b = conv.get(old, nan), conv.get(cur, nan)
        out[min(N, s + F):] = b[min(N, s + F):]
        k = max(0, min(F, N - s))
        if k:
            out[s:s + k] = a[s:s + k] * gains[0][:k, None] + b[s:s + k] * gains[1][:k, None]
    return out


class FadeVoice:
    """One voice of a schedule: its signal, the table it starts with, and what the restatement says happened to it."""

    def __init__(self, x, table):
        self.x, self.table = x, int(table)
        self.fades, self.out, self.pushed = [], [], 0

    def result(self):
        return np.concatenate(self.out) if self.out else np.zeros((0, 2), np.float32)


def ragged_schedule(seed, *, slots, M, H, F, T, cx, sizes=(0, 1, 7, 64, 599, 600), calls=40):
    """``(calls, voices, counted)``: ``calls`` is a list of ``(blocks, counts, flags, tables)``; ``voices`` is
    ``{slot: [FadeVoice, ...]}`` in order, slots reused after END, each voice with 0 to 3 accepted switches; ``counted``
    holds, from the restatement alone, how often each case the GPU test must meet occurs."""
    rng = np.random.default_rng(seed)
    pos = [0] * slots
    rec = [(0, 0, 0)] * slots
    left = [0] * slots
    live = [None] * slots
    tables = np.zeros(slots, np.int32)
    voices = {b: [] for b in range(slots)}
    fade_of, fade_calls = [None] * slots, [0] * slots                 # per slot: the fade it is returning, over how many calls
    counted = dict(crosses_512=0, tile_inside=0, three_calls=0, row_past_512=0, crosses_call=0, cut_by_end=0, refused=0, switch_on_fresh=0, accepted=0)
    out = []
    i = 0
    while i < calls or any(v is not None for v in live):
        last = i >= calls                                              # closing: no new voice, whole blocks, END when done
        i += 1
        assert i < calls + 20
        blocks, counts, flags = {}, np.zeros(slots, np.int32), np.zeros(slots, np.int32)
        for b in range(slots):
            v = live[b]
            if v is None:
                if last or rng.random() < 0.4:
                    continue
                n_total = int(rng.choice([1, 200, 900, 1500, 2600]))
                x = np.random.default_rng([seed, i, b]).uniform(-1, 1, (n_total, cx))   # (the schedule does not depend on cx)
                v = live[b] = FadeVoice(x.astype(np.float32), rng.integers(T))
                v.wanted = int(rng.integers(0, 4))
                voices[b].append(v)
                flags[b] |= START
                tables[b] = v.table
                if rng.random() < 0.3:                                 # a SWITCH on a fresh slot: ignored, the table is START's
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
                tables[b] = (int(tables[b]) + 1 + int(rng.integers(T - 1))) % T if left[b] == 0 else int(rng.integers(T))
            if v.pushed == len(v.x) and (last or rng.random() < 0.6):
                flags[b] |= END
        for b in range(slots):
            fresh = bool(flags[b] & START) or pos[b] == 0
            before = rec[b]
            n_out, pos[b], rec[b], new_left, E, accept = one_slot(pos[b], rec[b], counts[b], flags[b], tables[b], H, F, M)
            v = live[b]
            if fresh or accept:
                fade_of[b] = None
            if v is not None and fresh and n_out >= 0:
                v.table = rec[b][1]                                    # (a voice that has pushed nothing yet begins again)
            if flags[b] & SWITCH and v is not None:
                if fresh:
                    counted['switch_on_fresh'] += 1
                elif accept:
                    counted['accepted'] += 1
                    v.fades.append(rec[b])
                    v.wanted -= 1
                else:                                                  # ignored: tables[b] stays the refused one, unread
                    counted['refused'] += 1
                    assert left[b] > 0 and rec[b] == before
            if v is not None and F and n_out > 0:
                s = rec[b][0]
                lo, hi = max(E, s), min(E + n_out, s + F)              # the blended frames this call returns
                if lo < hi:
                    # A fade begins at E and goes on at the next call's E: its frames of a row are the row's first, so it
                    # reaches frame 512 of a row only with F > 512.  At a smaller F the row's second tile is one table's.
                    if (lo - E) < 512 <= (hi - 1 - E):
                        counted['crosses_512'] += 1
                    if n_out > 512:
                        counted['row_past_512'] += 1
                    if lo == E and hi - E >= 512:
                        counted['tile_inside'] += 1
                    fade_calls[b] = fade_calls[b] + 1 if s == fade_of[b] else 1
                    fade_of[b] = s
                    if fade_calls[b] == 3:
                        counted['three_calls'] += 1
                    if new_left > 0:
                        counted['crosses_call'] += 1
                    if flags[b] & END and E + n_out < s + F:
                        counted['cut_by_end'] += 1
            left[b] = new_left
            if flags[b] & END:
                live[b] = None
        out.append((blocks, counts.copy(), flags.copy(), tables.copy()))
    assert all(v is None for v in live)
    return out, voices, counted

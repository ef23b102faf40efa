"""The tap-table gate, restated: what ``vnd_taps_create`` and ``vnd_taps_deserialize`` must refuse and what they must
admit, written from the contract in ``include/vnd_amd.h`` ("tap tables") and the image layout (int32 header[8] = {magic,
version, C, taps, segments, has_seg, has_flags, apply_gain}, then tap_off[C+1], idx, w, (seg_off[C+1], seg_end, seg_gain),
(flags[C] padded to 4 bytes)) - not from the C code.  TEST INFRASTRUCTURE ONLY.

* :func:`judge_create` / :func:`judge_image` - the verdict for raw arrays / for an image's bytes: ``ADMITTED`` or a
  :class:`Verdict` with the status and the reason the entry must give;
* :func:`refusal_corpus` - every refusal, as cases both the CPU tier and the stand-alone sanitizer program replay;
* :func:`edge_tables` - the tables the gate admits at its edges (any order, duplicates, zero weights, empty channels and
  segments, indices up to 2^30, non-finite gains), for the GPU tier;
* :func:`mutated_images` - valid images of six small tables with one word changed or the tail cut, labelled by the mirror.

Pure NumPy: no device, no native library.
"""
from __future__ import annotations

import re
import struct
from dataclasses import dataclass, replace
from typing import List, Optional

import numpy as np

OK, INVALID, UNSUPPORTED = 0, 1, 4
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
MAGIC, IMAGE_VERSION = 0x564E4454, 1          # "VNDT", VND_TAPS_IMAGE_VERSION
MAX_CHANNELS = 65535
MAX_INDEX = 1 << 30


@dataclass(frozen=True)
class Verdict:
    status: int
    reason: str          # the message the entry gives, numbers replaced by '#' (see normalise)

    @property
    def admitted(self) -> bool:
        return self.status == OK


ADMITTED = Verdict(OK, '')

# every distinct refusal of the two entries, as normalise() renders its message
R_NULL_OUT = 'null out pointer'
R_NULL_CTX = 'null context'
R_CHANNELS = 'num_channels # out of range'
R_NULL_TAP_OFF = 'null tap_offsets'
R_TAP_OFF_0 = 'tap_offsets[#] must be #'
R_TAP_OFF_MONO = 'tap_offsets not monotone'
R_NULL_TAPS = 'null tap arrays'
R_NEG_INDEX = 'negative tap index at #'
R_FAR_INDEX = 'tap index # at # is beyond #^# frames'
R_SEG_INCOMPLETE = 'segment table incomplete'
R_SEG_OFF_0 = 'seg_offsets[#] must be #'
R_SEG_OFF_MONO = 'seg_offsets not monotone'
R_SEG_ORDER = 'segment # of channel # out of order'
R_SEG_COVER = 'segments of channel # do not cover its taps'
R_IMG_SHORT = 'tap image too short'
R_IMG_ALIGN = 'tap image is not #-byte aligned'
R_IMG_FORMAT = 'not a tap image of this format version'
R_IMG_HEADER = 'corrupt tap image header'
R_IMG_TRUNCATED = 'tap image truncated'
R_IMG_CORRUPT = 'corrupt tap image'
CREATE_REASONS = (R_NULL_OUT, R_NULL_CTX, R_CHANNELS, R_NULL_TAP_OFF, R_TAP_OFF_0, R_TAP_OFF_MONO, R_NULL_TAPS, R_NEG_INDEX,
                  R_FAR_INDEX, R_SEG_INCOMPLETE, R_SEG_OFF_0, R_SEG_OFF_MONO, R_SEG_ORDER, R_SEG_COVER)
IMAGE_REASONS = (R_NULL_OUT, R_IMG_SHORT, R_IMG_ALIGN, R_IMG_FORMAT, R_IMG_HEADER, R_IMG_TRUNCATED, R_IMG_CORRUPT)


def normalise(message) -> str:
    """A ``vnd_last_error()`` text with every number replaced by '#'."""
    if isinstance(message, bytes):
        message = message.decode()
    return re.sub(r'-?\d+', '#', message)


@dataclass
class Table:
    """The arguments of ``vnd_taps_create`` after the context; ``None`` is a NULL pointer.  ``C`` is passed as it stands
    (it need not match ``len(tap_offsets) - 1`` in a case that is refused before the arrays are read)."""
    name: str
    C: int
    tap_offsets: Optional[np.ndarray]
    tap_index: Optional[np.ndarray] = None
    tap_weight: Optional[np.ndarray] = None
    seg_offsets: Optional[np.ndarray] = None
    seg_end: Optional[np.ndarray] = None
    seg_gain: Optional[np.ndarray] = None
    chan_flags: Optional[np.ndarray] = None
    apply_gain: int = 0

    def __post_init__(self):
        for f, t in (('tap_offsets', np.int32), ('tap_index', np.int32), ('tap_weight', np.float32), ('seg_offsets', np.int32),
                     ('seg_end', np.int32), ('seg_gain', np.float32), ('chan_flags', np.uint8)):
            v = getattr(self, f)
            if v is not None:
                setattr(self, f, np.ascontiguousarray(v, t).ravel())

    def kwargs(self) -> dict:
        return dict(seg_offsets=self.seg_offsets, seg_end=self.seg_end, seg_gain=self.seg_gain, chan_flags=self.chan_flags,
                    apply_gain=bool(self.apply_gain))

    def oracle_kwargs(self) -> dict:
        return dict(seg_off=self.seg_offsets, seg_end=self.seg_end, seg_gain=self.seg_gain, chan_flags=self.chan_flags,
                    apply_gain=bool(self.apply_gain))

    @property
    def num_channels(self) -> int:
        return self.C

    def filled(self) -> 'Table':
        """The same table with empty arrays where a table without taps passes NULL."""
        return replace(self, tap_index=np.zeros(0, np.int32) if self.tap_index is None else self.tap_index,
                       tap_weight=np.zeros(0, np.float32) if self.tap_weight is None else self.tap_weight)

    @property
    def total(self) -> int:
        return int(self.tap_offsets[self.C])

    @property
    def max_index(self) -> int:
        return int(self.tap_index[:self.total].max()) if self.total else 0

    def to_bytes(self) -> bytes:
        """The image of an admitted table, laid out from the format's description."""
        C, total = self.C, self.total
        has_seg, has_flags = self.seg_offsets is not None, self.chan_flags is not None
        segs = int(self.seg_offsets[C]) if has_seg else 0
        out = struct.pack('<8i', MAGIC, IMAGE_VERSION, C, total, segs, int(has_seg), int(has_flags), int(bool(self.apply_gain)))
        out += self.tap_offsets[:C + 1].tobytes()
        if total:
            out += self.tap_index[:total].tobytes() + self.tap_weight[:total].tobytes()
        if has_seg:
            out += self.seg_offsets[:C + 1].tobytes() + self.seg_end[:segs].tobytes() + self.seg_gain[:segs].tobytes()
        if has_flags:
            out += self.chan_flags[:C].tobytes() + b'\0' * (-C % 4)
        return out


# ---- the mirror ------------------------------------------------------------------------------------------------------
def judge_create(t: Table, *, null_out: bool = False, null_ctx: bool = False) -> Verdict:
    """What ``vnd_taps_create`` must answer.  The order is the contract's reading order: the call's own pointers, the channel
    count, the tap CSR row, the taps one by one, then the segment table - row first, then channel by channel."""
    if null_out:
        return Verdict(INVALID, R_NULL_OUT)
    if null_ctx:
        return Verdict(INVALID, R_NULL_CTX)
    C = t.C
    if C <= 0 or C > MAX_CHANNELS:
        return Verdict(INVALID, R_CHANNELS)
    if t.tap_offsets is None:
        return Verdict(INVALID, R_NULL_TAP_OFF)
    off = [int(v) for v in t.tap_offsets[:C + 1]]
    assert len(off) == C + 1, 'a case must bring the C + 1 offsets the entry reads'
    if off[0] != 0:
        return Verdict(INVALID, R_TAP_OFF_0)
    if any(off[c + 1] < off[c] for c in range(C)):
        return Verdict(INVALID, R_TAP_OFF_MONO)
    total = off[C]
    if total > 0 and (t.tap_index is None or t.tap_weight is None):
        return Verdict(INVALID, R_NULL_TAPS)
    if total > 0:
        assert len(t.tap_index) >= total and len(t.tap_weight) >= total, 'a case must bring the taps its offsets announce'
    for k in range(total):
        i = int(t.tap_index[k])
        if i < 0:
            return Verdict(INVALID, R_NEG_INDEX)
        if i > MAX_INDEX:
            return Verdict(UNSUPPORTED, R_FAR_INDEX)
    if t.seg_offsets is None:
        return ADMITTED                                  # function path: seg_end / seg_gain are not looked at
    if t.seg_end is None or t.seg_gain is None:
        return Verdict(INVALID, R_SEG_INCOMPLETE)
    so = [int(v) for v in t.seg_offsets[:C + 1]]
    assert len(so) == C + 1
    if so[0] != 0:
        return Verdict(INVALID, R_SEG_OFF_0)
    if any(so[c + 1] < so[c] for c in range(C)):
        return Verdict(INVALID, R_SEG_OFF_MONO)
    assert len(t.seg_end) >= so[C] and len(t.seg_gain) >= so[C], 'a case must bring the segments its offsets announce'
    for c in range(C):
        prev = off[c]                                    # segment ends are absolute tap positions, ascending inside the channel
        for s in range(so[c], so[c + 1]):
            end = int(t.seg_end[s])
            if end < prev or end > off[c + 1]:
                return Verdict(INVALID, R_SEG_ORDER)
            prev = end
        if off[c + 1] != off[c] and prev != off[c + 1]:  # taps after the last segment would be dropped silently
            return Verdict(INVALID, R_SEG_COVER)
    return ADMITTED


def parse_image(image: bytes, nbytes: Optional[int] = None):
    """(verdict, table): the verdict of the image's own layer and, when that layer passes, the table it holds."""
    nbytes = len(image) if nbytes is None else nbytes
    if nbytes < 32:
        return Verdict(INVALID, R_IMG_SHORT), None
    magic, version, C, total, segs, has_seg, has_flags, gain = struct.unpack_from('<8i', image)
    if magic != MAGIC or version != IMAGE_VERSION:
        return Verdict(INVALID, R_IMG_FORMAT), None
    if C <= 0 or C > MAX_CHANNELS or total < 0 or segs < 0:
        return Verdict(INVALID, R_IMG_HEADER), None
    words = 8 + (C + 1) + 2 * total + ((C + 1) + 2 * segs if has_seg else 0) + ((C + 3) // 4 if has_flags else 0)
    if nbytes < 4 * words:
        return Verdict(INVALID, R_IMG_TRUNCATED), None
    pos = 32

    def take(dtype, count):
        nonlocal pos
        a = np.frombuffer(image, dtype, count, pos).copy()
        pos += 4 * count if dtype != np.uint8 else count
        return a

    t = Table('image', C, take(np.int32, C + 1), take(np.int32, total), take(np.float32, total), apply_gain=int(gain != 0))
    if has_seg:
        t.seg_offsets, t.seg_end, t.seg_gain = take(np.int32, C + 1), take(np.int32, segs), take(np.float32, segs)
    if has_flags:
        t.chan_flags = take(np.uint8, C)
    if int(t.tap_offsets[C]) != total or (has_seg and int(t.seg_offsets[C]) != segs):
        return Verdict(INVALID, R_IMG_CORRUPT), None
    return ADMITTED, t


def judge_image(image: Optional[bytes], nbytes: Optional[int] = None, *, null_out: bool = False, null_ctx: bool = False,
                misaligned: bool = False) -> Verdict:
    """What ``vnd_taps_deserialize`` must answer for ``nbytes`` (default: all) of ``image``; ``misaligned``: the buffer
    starts at an address that is no multiple of 4."""
    if null_out:
        return Verdict(INVALID, R_NULL_OUT)
    if image is None or (len(image) if nbytes is None else nbytes) < 32:
        return Verdict(INVALID, R_IMG_SHORT)
    if misaligned:
        return Verdict(INVALID, R_IMG_ALIGN)
    v, table = parse_image(image, nbytes)
    if not v.admitted:
        return v
    return judge_create(table, null_ctx=null_ctx)


# ---- cases -----------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    """One call of an entry and what it must answer.  ``entry``: 'create' (``table``) or 'image' (``image`` / ``nbytes``)."""
    name: str
    entry: str
    verdict: Verdict
    table: Optional[Table] = None
    image: Optional[bytes] = None
    nbytes: Optional[int] = None
    null_out: bool = False
    null_ctx: bool = False
    misaligned: bool = False
    group: str = 'listed'            # or 'mutant': one of mutated_images()


def create_case(t: Table, **how) -> Case:
    return Case(t.name + ''.join(f' [{k}]' for k in how), 'create', judge_create(t, **how), table=t, **how)


def image_case(name: str, image: Optional[bytes], nbytes: Optional[int] = None, **how) -> Case:
    return Case(name + ''.join(f' [{k}]' for k in how), 'image', judge_image(image, nbytes, **how), image=image, nbytes=nbytes, **how)


def _fn(name, offsets, idx, w, **kw) -> Table:
    return Table(name, len(offsets) - 1, offsets, idx, w, **kw)


def base_stereo() -> Table:
    """Two channels, three taps each, two segments each: the valid table the malformed ones are one step away from."""
    return Table('base', 2, [0, 3, 6], [2, 9, 4, 0, 7, 30], [-1, 1, 1, -1, -1, 1], seg_offsets=[0, 2, 4], seg_end=[2, 3, 4, 6],
                 seg_gain=[0.9, 0.5, 0.9, 0.5], chan_flags=[0, 0], apply_gain=1)


def malformed_tables() -> List[Table]:
    """The refusals of ``vnd_taps_create`` that arrays alone express (each also travels as an image where an image can
    hold it: :func:`refusal_corpus`)."""
    b = base_stereo()
    plain = dict(seg_offsets=None, seg_end=None, seg_gain=None, chan_flags=None, apply_gain=0)
    out = [replace(b, name='C = 0', C=0), replace(b, name='C = -1', C=-1), replace(b, name='C = 65536', C=65536),
           replace(b, name='null tap_offsets', tap_offsets=None),
           replace(b, name='tap_offsets[0] = 1', tap_offsets=[1, 3, 6]),
           replace(b, name='tap_offsets[0] = -1', tap_offsets=[-1, 3, 6])]
    four = dict(C=4, tap_index=[1, 2, 3, 4, 5, 6, 7, 8], tap_weight=[1] * 8, **plain)
    out += [replace(b, name='tap_offsets falls at the first channel', tap_offsets=[0, -1, 4, 6, 8], **four),
            replace(b, name='tap_offsets falls at a middle channel', tap_offsets=[0, 4, 3, 6, 8], **four),
            replace(b, name='tap_offsets falls at the last channel', tap_offsets=[0, 2, 4, 8, 7], **four),
            replace(b, name='null tap_index', tap_index=None), replace(b, name='null tap_weight', tap_weight=None),
            replace(b, name='null tap arrays', tap_index=None, tap_weight=None)]
    for where, k in (('first', 0), ('last', 5)):
        for what, value in (('-1', -1), ('INT32_MIN', INT_MIN), ('2^30 + 1', MAX_INDEX + 1), ('INT32_MAX', INT_MAX)):
            idx = b.tap_index.copy()
            idx[k] = value
            out.append(replace(b, name=f'index {what} at the {where} tap', tap_index=idx))
            out.append(replace(b, name=f'index {what} at the {where} tap, function path', tap_index=idx, **plain))
    out += [replace(b, name='seg_offsets without seg_end', seg_end=None),
            replace(b, name='seg_offsets without seg_gain', seg_gain=None),
            replace(b, name='seg_offsets without either', seg_end=None, seg_gain=None),
            replace(b, name='seg_offsets[0] = 1', seg_offsets=[1, 2, 4]),
            replace(b, name='seg_offsets falls at the first channel', seg_offsets=[0, -1, 4]),
            replace(b, name='seg_offsets falls at the last channel', seg_offsets=[0, 3, 2]),
            # (a row that rises wildly before it falls: its entries must not be followed into seg_end)
            replace(b, name='seg_offsets rises past the table, then falls', seg_offsets=[0, INT_MAX, 4]),
            # (... where every segment end there is suits the first channel: nothing else stops a walk begun too early)
            replace(b, name='seg_offsets rises past the table over ends that all fit', tap_offsets=[0, 6, 6], seg_offsets=[0, INT_MAX, 4],
                    seg_end=[2, 3, 4, 6]),
            replace(b, name='segment end below the previous one', seg_end=[2, 1, 4, 6]),
            replace(b, name='segment end below the channel\'s first tap', seg_end=[2, 3, 2, 6]),
            replace(b, name='segment end above the channel\'s last tap', seg_end=[2, 4, 4, 6]),
            replace(b, name='last segment end above the table', seg_end=[2, 3, 4, 7]),
            replace(b, name='negative segment end', seg_end=[-1, 3, 4, 6]),
            replace(b, name='segments stop short of the taps', seg_end=[2, 3, 4, 5]),
            replace(b, name='segments stop short in the first channel', seg_end=[1, 2, 4, 6]),
            replace(b, name='a channel with taps and no segment', seg_offsets=[0, 2, 2], seg_end=[2, 3], seg_gain=[0.9, 0.5]),
            replace(b, name='the first channel with taps and no segment', seg_offsets=[0, 0, 2], seg_end=[4, 6], seg_gain=[0.9, 0.5])]
    return out


def header_image(C, total=0, segs=0, has_seg=0, has_flags=0, gain=0, body_words=8, magic=MAGIC, version=IMAGE_VERSION) -> bytes:
    return struct.pack('<8i', magic, version, C, total, segs, has_seg, has_flags, gain) + b'\0' * (4 * body_words)


def refusal_corpus() -> List[Case]:
    """Every refusal of the two entries: the listed cases and the mutants the mirror refuses.  Nothing here is admitted -
    the CPU tier passes a context pointer that must never be followed."""
    b = base_stereo()
    cases = [create_case(b, null_out=True), create_case(b, null_ctx=True), create_case(b, null_out=True, null_ctx=True)]
    cases += [create_case(t) for t in malformed_tables()]
    good = b.to_bytes()
    assert judge_image(good).admitted
    cases += [image_case('valid image', good, null_out=True), image_case('valid image', good, null_ctx=True),
              image_case('null buffer', None), image_case('null buffer, zero bytes', None, 0),
              image_case('valid image', good, misaligned=True),
              image_case('0 bytes', good, 0), image_case('31 bytes', good, 31), image_case('-1 bytes', good, -1),
              image_case('header alone', good, 32),
              image_case('wrong magic', header_image(1, magic=MAGIC + 1)), image_case('magic 0', header_image(1, magic=0)),
              image_case('wrong version', header_image(1, version=IMAGE_VERSION + 1)),
              image_case('version 0', header_image(1, version=0))]
    for C in (0, -1, 65536, INT_MAX - 1, INT_MAX, INT_MIN):
        for has_seg in (0, 1):
            for has_flags in (0, 1):
                cases.append(image_case(f'header C = {C}, has_seg = {has_seg}, has_flags = {has_flags}', header_image(C, 0, 0, has_seg, has_flags)))
    for name, total, segs in (('total = -1', -1, 0), ('segs = -1', 0, -1), ('total = INT_MIN', INT_MIN, 0), ('segs = INT_MIN', 0, INT_MIN),
                              ('total = INT_MAX', INT_MAX, 0), ('segs = INT_MAX', 0, INT_MAX), ('total = segs = INT_MAX', INT_MAX, INT_MAX)):
        for C in (1, 65535):
            cases.append(image_case(f'header {name}, C = {C}', header_image(C, total, segs, 1, 1)))
    # a body one word short of what the header announces, for each optional part
    for name, t in (('plain', replace(b, seg_offsets=None, seg_end=None, seg_gain=None, chan_flags=None)),
                    ('segments', replace(b, chan_flags=None)), ('flags', replace(b, seg_offsets=None, seg_end=None, seg_gain=None)),
                    ('segments and flags', b)):
        image = t.to_bytes()
        assert judge_image(image).admitted
        cases += [image_case(f'{name}: one word short', image[:-4]), image_case(f'{name}: one byte short', image[:-1]),
                  image_case(f'{name}: one word short by count', image, len(image) - 4)]
    words = list(struct.unpack(f'<{len(good) // 4}i', good))

    def patched(pos, value):
        w = list(words)
        w[pos] = value
        return struct.pack(f'<{len(w)}i', *w)

    # (positions in the base image: 8 header words, tap_off at 8..10, idx 11..16, w 17..22, seg_off 23..25, seg_end 26..29)
    assert words[10] == 6 and words[25] == 4
    cases += [image_case('tap_off[C] below total', patched(10, 5)), image_case('tap_off[C] above total', patched(10, 7)),
              image_case('header total below tap_off[C]', patched(3, 5)),
              image_case('seg_off[C] below segs', patched(25, 3)), image_case('seg_off[C] above segs', patched(25, 5)),
              image_case('header segs below seg_off[C]', patched(4, 3))]
    # a consistent header around a body vnd_taps_create must refuse: every malformed table an image can express
    # (an image has no null arrays and takes its channel count and totals from its own rows)
    for t in malformed_tables():
        if t.tap_offsets is None or t.tap_index is None or t.tap_weight is None or t.C != len(t.tap_offsets) - 1:
            continue
        if t.seg_offsets is not None and (t.seg_end is None or t.seg_gain is None):
            continue
        if not 0 <= int(t.tap_offsets[t.C]) <= len(t.tap_index):
            continue
        if t.seg_offsets is not None and not 0 <= int(t.seg_offsets[t.C]) <= min(len(t.seg_end), len(t.seg_gain)):
            continue
        case = image_case(f'image of: {t.name}', t.to_bytes())
        assert case.verdict == judge_create(t), t.name
        cases.append(case)
    cases += [m for m in mutated_images() if not m.verdict.admitted]
    assert not any(c.verdict.admitted for c in cases), [c.name for c in cases if c.verdict.admitted]
    return cases


def call_case(lib, ctx, case: Case):
    """Replay ``case`` on the loaded library (prototypes as ``_native.load_library`` declares them) with context pointer
    ``ctx``: (status, normalised message, the value left in ``*taps``).  Every array is handed over at its exact size."""
    import ctypes
    out = ctypes.c_void_p(0xDEAD)                          # the entry must clear it
    ctx = None if case.null_ctx else ctx
    if case.entry == 'create':
        t = case.table
        ptr = lambda a, ct: None if a is None else a.ctypes.data_as(ctypes.POINTER(ct))     # noqa: E731
        rc = lib.vnd_taps_create(ctx, t.C, ptr(t.tap_offsets, ctypes.c_int32), ptr(t.tap_index, ctypes.c_int32),
                                 ptr(t.tap_weight, ctypes.c_float), ptr(t.seg_offsets, ctypes.c_int32), ptr(t.seg_end, ctypes.c_int32),
                                 ptr(t.seg_gain, ctypes.c_float), ptr(t.chan_flags, ctypes.c_uint8), int(t.apply_gain),
                                 None if case.null_out else ctypes.byref(out))
    else:
        nbytes = (len(case.image) if case.image is not None else 0) if case.nbytes is None else case.nbytes
        buf = None
        if case.image is not None:
            raw = ctypes.create_string_buffer(len(case.image) + 8)
            shift = (-ctypes.addressof(raw)) % 4 + (1 if case.misaligned else 0)
            ctypes.memmove(ctypes.addressof(raw) + shift, case.image, len(case.image))
            buf = ctypes.c_void_p(ctypes.addressof(raw) + shift)
        rc = lib.vnd_taps_deserialize(ctx, buf, nbytes, None if case.null_out else ctypes.byref(out))
    return rc, normalise(lib.vnd_last_error() or b''), (None if case.null_out else out.value)


# ---- the mutation corpus ---------------------------------------------------------------------------------------------
def small_tables(seed: int = 20240611) -> List[Table]:
    """Six small valid tables: function and class path, with and without flags and gains, C = 1, 2, 8."""
    rng = np.random.default_rng(seed)

    def function_path(name, C, flags=False):
        counts = rng.integers(1, 4, C)
        offsets = np.concatenate([[0], np.cumsum(counts)])
        idx = np.concatenate([np.sort(rng.choice(40, k, replace=False)) for k in counts])
        w = rng.choice([0.5, -0.5, 0.85, -0.2, 1.0, -1.0], len(idx))
        return Table(name, C, offsets, idx, w, chan_flags=(rng.integers(0, 2, C) if flags else None))

    def class_path(name, C, gains, flags=True):
        offsets, so, idx, w, se, sg, fl = [0], [0], [], [], [], [], []
        for c in range(C):
            copied = flags and C > 1 and c == C - 1
            fl.append(int(copied))
            for s in range(0 if copied else int(rng.integers(1, 4))):
                k = int(rng.integers(0, 3))                      # (empty segments among them)
                idx += [int(v) for v in rng.integers(0, 40, k)]
                w += [float(v) for v in np.sort(rng.choice([-1.0, 1.0], k))]
                se.append(len(idx))
                sg.append(float(rng.choice([0.9, 0.5, 0.2])) if gains else 1.0)
            offsets.append(len(idx))
            so.append(len(se))
        return Table(name, C, offsets, idx, w, seg_offsets=so, seg_end=se, seg_gain=sg, chan_flags=fl if flags else None,
                     apply_gain=int(gains))

    tables = [function_path('function path, C = 1', 1), function_path('function path, C = 2, flags', 2, flags=True),
              function_path('function path, C = 8', 8), class_path('class path, C = 1, gains', 1, True, flags=False),
              class_path('class path, C = 2, gains, flags', 2, True), class_path('class path, C = 8, no gains, flags', 8, False)]
    for t in tables:
        assert judge_create(t).admitted, t.name
    return tables


MUTANT_VALUES = (('0', lambda v: 0), ('-1', lambda v: -1), ('1', lambda v: 1), ('INT_MAX', lambda v: INT_MAX),
                 ('INT_MIN', lambda v: INT_MIN), ('value + 1', lambda v: v + 1), ('value - 1', lambda v: v - 1))


def image_regions(t: Table):
    """[(name, first word, words)] of an admitted table's image."""
    C, total = t.C, t.total
    segs = int(t.seg_offsets[C]) if t.seg_offsets is not None else 0
    regions, pos = [('header', 0, 8)], 8
    for name, count in (('tap_off', C + 1), ('idx', total), ('w', total)):
        regions.append((name, pos, count))
        pos += count
    if t.seg_offsets is not None:
        for name, count in (('seg_off', C + 1), ('seg_end', segs), ('seg_gain', segs)):
            regions.append((name, pos, count))
            pos += count
    if t.chan_flags is not None:
        regions.append(('flags', pos, (C + 3) // 4))
    return regions


def mutated_images(seed: int = 20240611) -> List[Case]:
    """Every word of every small table's image set to each of MUTANT_VALUES, and the image cut after every word and in
    the middle of its last one; each labelled by the mirror.  ``case.name`` says which region the word lies in."""
    cases = []
    for t in small_tables(seed):
        image = t.to_bytes()
        nwords = len(image) // 4
        words = struct.unpack(f'<{nwords}i', image)
        region_of = {}
        for name, first, count in image_regions(t):
            for p in range(first, first + count):
                region_of[p] = f'{name}[{p - first}]'
        for pos in range(nwords):
            for label, f in MUTANT_VALUES:
                value = f(words[pos])
                if value == words[pos] or not INT_MIN <= value <= INT_MAX:
                    continue
                w = list(words)
                w[pos] = value
                cases.append(image_case(f'{t.name}: {region_of[pos]} = {label}', struct.pack(f'<{nwords}i', *w)))
        for cut in range(nwords):
            cases.append(image_case(f'{t.name}: cut to {cut} words', image[:4 * cut]))
        cases.append(image_case(f'{t.name}: cut inside the last word', image[:-2]))
    for case in cases:
        case.group = 'mutant'
    return cases


# ---- what the gate admits at its edges (GPU tier) -------------------------------------------------------------------------
_WEIGHTS = np.array([1.0, -1.0, 0.5, -0.5, 0.85, -0.2, 1e-3, -3.0], np.float32)
SPAN = 700                                                # (offsets of the ordinary taps: the fuzz tier's first shape)


def _ordinary(rng, C, most=12, span=SPAN):
    """Per channel a few unique ascending indices and weights: the ordinary taps an edge is planted among."""
    rows = []
    for _ in range(C):
        k = int(rng.integers(most // 2, most + 1))
        rows.append((np.sort(rng.choice(span, k, replace=False)).astype(np.int64), rng.choice(_WEIGHTS, k).astype(np.float32)))
    return rows


def _from_rows(name, rows, **kw) -> Table:
    offsets = np.concatenate([[0], np.cumsum([len(i) for i, _ in rows])])
    idx = np.concatenate([i for i, _ in rows]) if rows else np.zeros(0)
    w = np.concatenate([w for _, w in rows]) if rows else np.zeros(0)
    return Table(name, len(rows), offsets, idx, w, **kw)


def _with_tap(rows, c, at, index, weight):
    i, w = rows[c]
    rows = list(rows)
    rows[c] = (np.insert(i, at, index), np.insert(w, at, np.float32(weight)))
    return rows


def _class(name, rng, layout, gains, apply_gain, flags=None) -> Table:
    """``layout[c]``: taps per segment of channel c (0 = an empty segment; [] = no segment); weights -1 first, then +1."""
    offsets, so, idx, w, se = [0], [0], [], [], []
    for segs in layout:
        for k in segs:
            idx += [int(v) for v in rng.choice(SPAN, k, replace=False)]
            neg = int(rng.integers(0, k + 1)) if k else 0
            w += [-1.0] * neg + [1.0] * (k - neg)
            se.append(len(idx))
        offsets.append(len(idx))
        so.append(len(se))
    sg = [gains[s % len(gains)] for s in range(len(se))]
    return Table(name, len(layout), offsets, idx, w, seg_offsets=so, seg_end=se, seg_gain=sg, chan_flags=flags, apply_gain=apply_gain)


def edge_tables(n: int = 10000, seed: int = 77) -> List[Table]:
    """The tables of the GPU tier, all admitted.  ``n``: the signal length the index edges sit around."""
    rng = np.random.default_rng(seed)
    out = []

    def unsorted_dup(C, tag=''):
        rows = _ordinary(rng, C)
        desc = [(i[::-1].copy(), w[::-1].copy()) for i, w in rows]
        shuffled = []
        for i, w in rows:
            p = rng.permutation(len(i))
            shuffled.append((i[p], w[p]))
        equal, cancel = rows, rows
        for c in range(C):                                # (an index of its own, past the ordinary taps: the table stays ascending)
            for weights, which in (((0.85, 0.85), 'equal'), ((1.0, -1.0), 'cancel')):
                grown = equal if which == 'equal' else cancel
                for wt in weights:
                    grown = _with_tap(grown, c, len(grown[c][0]), SPAN + 1 + c, wt)
                if which == 'equal':
                    equal = grown
                else:
                    cancel = grown
        return [_from_rows(f'unsorted descending{tag}', desc), _from_rows(f'unsorted shuffled{tag}', shuffled),
                _from_rows(f'duplicate 0.85 0.85{tag}', equal), _from_rows(f'duplicate +1 -1{tag}', cancel)]

    out += unsorted_dup(2)
    rows = _ordinary(rng, 2)
    zeros = rows
    for c in range(2):
        zeros = _with_tap(_with_tap(zeros, c, 2, 5 + c, 0.0), c, 5, 611 + c, -0.0)
    out.append(_from_rows('zero weights +0 -0', zeros))
    out.append(_from_rows('channel 1 empty', [rows[0], (np.zeros(0, np.int64), np.zeros(0, np.float32))]))
    out.append(Table('no taps at all', 2, [0, 0, 0], None, None))
    for label, top in (('n - 1', n - 1), ('n', n), ('2^24 - 2', (1 << 24) - 2), ('2^24 - 1', (1 << 24) - 1), ('2^24', 1 << 24),
                       ('2^30', MAX_INDEX)):
        edge = _with_tap(_with_tap(_ordinary(rng, 2), 0, 3, top, 0.5), 1, 0, top - (top % 2 == 0), -1.0)
        edge = _with_tap(edge, 1, 4, top, 0.85)
        out.append(_from_rows(f'largest index {label}', edge))
    out += [_class('empty first segment', rng, [[0, 5, 4], [0, 3, 6]], [0.9, 0.5, 0.2], 1),
            _class('empty middle segment', rng, [[5, 0, 4], [4, 0, 0, 3]], [0.9, 0.5, 0.2], 1),
            _class('empty last segment', rng, [[5, 4, 0], [6, 0]], [0.9, 0.5, 0.2], 1),
            _class('segments and no taps', rng, [[5, 4], [0, 0, 0]], [0.9, 0.5], 1),
            _class('one segment holds every tap', rng, [[11], [9]], [0.7], 1),
            _class('gains ignored', rng, [[5, 4, 3], [4, 4, 4]], [0.9, 0.0, float('inf'), -2.0], 0),
            _class('gains 0 -0 1', rng, [[5, 4, 3], [4, 4, 4]], [0.0, -0.0, 1.0], 1),
            _class('copy-through channel with taps', rng, [[5, 4], [6, 3]], [0.9, 0.5], 1, flags=[1, 0]),
            _class('copy-through channel with taps, second', rng, [[5, 4], [6, 3]], [0.9, 0.5], 1, flags=[0, 1]),
            _class('gain inf', rng, [[5, 4], [6, 3]], [0.9, float('inf')], 1),
            _class('gain nan', rng, [[5, 4], [6, 3]], [float('nan'), 0.5], 1)]
    for C in (1, 3, 4, 6, 8):
        out += unsorted_dup(C, f', C = {C}')
    for t in out:
        assert judge_create(t).admitted, t.name
    assert len({t.name for t in out}) == len(out)
    return out


def per_table_scope(t: Table, mode_exact: bool) -> bool:
    """Whether the per-table (run-time compiled) kernels may take the table, from what DESIGN.md says of their scope: an even
    channel count up to 64, at least one tap, every channel filtered, finite weights and gains, indices below 2^24; in the exact
    mode no empty segment."""
    if t.C % 2 or t.C > 64 or t.total == 0 or t.max_index >= 1 << 24:
        return False
    if t.max_index >= 1 << 20:                           # (a halo no workgroup's LDS holds: the index-testing kernel)
        return False
    if t.chan_flags is not None and (t.chan_flags[:t.C] & 1).any():
        return False
    if not np.isfinite(t.tap_weight[:t.total]).all():
        return False
    if t.seg_offsets is not None:
        segs = int(t.seg_offsets[t.C])
        if t.apply_gain and not np.isfinite(t.seg_gain[:segs]).all():
            return False
        if mode_exact:
            for c in range(t.C):
                prev = int(t.tap_offsets[c])
                for s in range(int(t.seg_offsets[c]), int(t.seg_offsets[c + 1])):
                    if int(t.seg_end[s]) == prev:
                        return False
                    prev = int(t.seg_end[s])
    return True

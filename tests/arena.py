"""A guarded arena for the one-shot device entries (tests/test_gpu_footprint.py): ONE int32 device tensor laid out as

    [guard | x | guard | y | guard | workspace (declared bytes) | guard | aux inputs (tables, delays, h, ...) | guard]

so that a call's whole memory footprint is checked, not only the values it returns.  Every segment starts on a 16-byte
boundary plus an optional skew of 4 or 8 bytes (the alignment-dependent store shapes, the "generic kernel because misaligned"
route).  Guards hold SENTINEL, y holds POISON, the workspace a third pattern: NaNs that no arithmetic on finite inputs yields.
After the call, `check` waits for the device and asserts, naming the first offender:

  * every byte outside y and the workspace - guards in front of and behind every segment, x, every aux input - is what was uploaded;
  * no element of y still holds POISON.

`reset(invert_workspace=True)` restores the image with the workspace's bits inverted: a result that is the same for both
fills does not depend on what the workspace held."""
import numpy as np

POISON = 0x7FA5A5A5                  # y, float32: marks elements nobody wrote
SENTINEL = 0x7FB0B0B0                # guards
POISON64 = 0x7FF4A5A5A5A5A5A5        # y, float64
SENTINEL64 = 0x7FF5B0B0B0B0B0B0      # guards of an arena with a float64 output
WS_POISON64 = 0x7FF6C3C37FA9C3C3     # workspace: a NaN read as float64 on 8-byte boundaries, and both halves NaNs read as float32
GUARD_BYTES = 256 << 10              # the largest tile of any form is 128 KiB (split 64-frame runs, 256 lanes); never below 256 KiB
ALIGN = 16


def _words(pattern64, first_word, count):
    """`count` int32 words of a 64-bit pattern laid on 8-byte boundaries of the arena, starting at word `first_word`."""
    lo, hi = pattern64 & 0xFFFFFFFF, pattern64 >> 32
    out = np.empty(count, np.uint32)
    out[(first_word % 2)::2] = lo
    out[1 - (first_word % 2)::2] = hi
    return out


class Arena:
    def __init__(self, torch, device, *, x, y, workspace_bytes=0, aux=None, skew=None, guard_bytes=GUARD_BYTES):
        """x: a NumPy array (uploaded as it is); y: (shape, dtype) of the output; workspace_bytes: the declared size, to the byte;
        aux: {name: NumPy array} of further inputs, laid out in the order given; skew: {segment name: 0, 4 or 8} bytes."""
        skew = dict(skew or {})
        y_shape, y_dtype = tuple(y[0]), np.dtype(y[1])
        assert y_dtype in (np.dtype(np.float32), np.dtype(np.float64)), y_dtype
        self.torch, self.y_shape, self.y_dtype = torch, y_shape, y_dtype
        self.wide = y_dtype == np.dtype(np.float64)
        assert guard_bytes >= GUARD_BYTES and guard_bytes % ALIGN == 0, guard_bytes
        inputs = [('x', np.ascontiguousarray(x))] + [(k, np.ascontiguousarray(v)) for k, v in (aux or {}).items()]
        y_bytes = int(np.prod(y_shape, dtype=np.int64)) * y_dtype.itemsize
        sizes = [('x', inputs[0][1].nbytes), ('y', y_bytes), ('ws', int(workspace_bytes))] + [(k, v.nbytes) for k, v in inputs[1:]]
        assert len({k for k, _ in sizes}) == len(sizes), 'segment names must be distinct'
        assert set(skew) <= {k for k, _ in sizes} and all(s in (0, 4, 8) for s in skew.values()), skew
        self.offset, self.nbytes, self.order = {}, {}, [k for k, _ in sizes]
        at = guard_bytes
        for k, b in sizes:
            at += skew.get(k, 0)
            self.offset[k], self.nbytes[k] = at, b
            at = (at + b + ALIGN - 1) // ALIGN * ALIGN + guard_bytes
        self.total = at
        image = _words(SENTINEL64, 0, at // 4) if self.wide else np.full(at // 4, SENTINEL, np.uint32)
        self.image = image.view(np.uint8)
        for k, v in inputs:
            self.image[self.offset[k]:self.offset[k] + v.nbytes] = v.reshape(-1).view(np.uint8)
        self._fill('y', POISON64 if self.wide else POISON | (POISON << 32))
        self._fill('ws', WS_POISON64)
        self.fixed = np.ones(at, bool)                      # bytes no call may change
        for k in ('y', 'ws'):
            self.fixed[self.offset[k]:self.offset[k] + self.nbytes[k]] = False
        self.buf = torch.empty(at // 4, dtype=torch.int32, device=device)
        assert self.buf.data_ptr() % ALIGN == 0
        self.reset()

    def _fill(self, name, pattern64, invert=False):
        off, b = self.offset[name], self.nbytes[name]
        assert off % 4 == 0
        words = _words(pattern64, off // 4, (b + 3) // 4)
        if invert:
            words = ~words
        self.image[off:off + b] = words.view(np.uint8)[:b]

    def reset(self, invert_workspace=False):
        """The pristine image back on the device (the workspace's fill inverted bit by bit if asked)."""
        self._fill('ws', WS_POISON64, invert_workspace)
        self.buf.copy_(self.torch.from_numpy(self.image.view(np.int32)))       # (from pageable memory: done when it returns)

    def ptr(self, name):
        return self.buf.data_ptr() + self.offset[name]

    def tensor(self, name='y'):
        """The y segment as a torch view of its own shape and dtype (for the harness's own tests: no kernel needs it)."""
        assert name == 'y'
        off, b = self.offset['y'], self.nbytes['y']
        assert off % self.y_dtype.itemsize == 0
        flat = self.buf[off // 4:(off + b) // 4]
        return flat.view(self.torch.float64 if self.wide else self.torch.float32).view(self.y_shape)

    def _where(self, byte):
        """Names an arena byte: the segment it lies in, or the guard and its distance from the neighbouring segments."""
        before = None
        for k in self.order:
            lo, hi = self.offset[k], self.offset[k] + self.nbytes[k]
            if lo <= byte < hi:
                return f'{k} + {byte - lo} bytes'
            if byte < lo:
                front = f'{lo - byte} bytes in front of {k}'
                return front if before is None else f'{byte - before[1]} bytes past the end of {before[0]}, {front}'
            before = (k, hi)
        return f'{byte - before[1]} bytes past the end of {before[0]}'

    def check(self, where=''):
        """Waits for the device, holds the arena to the footprint contract and returns (y, workspace bytes) as NumPy arrays."""
        if self.buf.is_cuda:
            self.torch.cuda.synchronize()
        got = self.buf.cpu().numpy().view(np.uint8)
        bad = np.flatnonzero((got != self.image) & self.fixed)
        if len(bad):
            first = int(bad[0])
            inside = [k for k in self.order if self.offset[k] <= first < self.offset[k] + self.nbytes[k]]
            what = f'input {inside[0]} was changed' if inside else 'a guard was written'
            detail = ''
            yo, ye = self.offset['y'], self.offset['y'] + self.nbytes['y']
            if not inside and len(self.y_shape) == 3 and (ye <= first < ye + GUARD_BYTES or yo - GUARD_BYTES <= first < yo):
                # as an index of y's own layout, continued past its end (or before its start)
                elem = (first - yo) // self.y_dtype.itemsize
                S, n, C = self.y_shape
                detail = f'; as (stream, frame, channel) of y {(elem // (n * C), elem // C % n if n else 0, elem % C)} of {self.y_shape}'
            raise AssertionError(f'{where}: {what}: {len(bad)} bytes differ, the first at {self._where(first)} '
                                 f'(arena byte {first}){detail}')
        yo, yb = self.offset['y'], self.nbytes['y']
        ybytes = got[yo:yo + yb].copy()
        y = ybytes.view(self.y_dtype).reshape(self.y_shape)
        raw = ybytes.view(np.uint64 if self.wide else np.uint32).reshape(self.y_shape)
        hole = np.argwhere(raw == (POISON64 if self.wide else POISON))
        if len(hole):
            raise AssertionError(f'{where}: {len(hole)} elements of y were never written, the first at index '
                                 f'{tuple(int(i) for i in hole[0])} of {self.y_shape}')
        wo, wb = self.offset['ws'], self.nbytes['ws']
        return y, got[wo:wo + wb].copy()

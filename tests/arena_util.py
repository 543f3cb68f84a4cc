"""The arena of tests/test_gpu_addressing.py: ONE device allocation in which every address a kernel could reach with a wrong 32-bit offset is memory the test
owns.  The kernels address a plane -- and an output -- with unsigned 32-bit byte offsets from the address they are handed (profiles/addressing_limits.txt).  A
sign-extended offset lands up to 2^32 bytes BELOW that address, a truncated or late-scaled one anywhere in the 2^32 bytes above it: with a margin of 2^32 bytes
on both sides of every such address the wrong access reads (or overwrites) the arena's fill byte and shows as a bit mismatch or a damaged margin, never as a fault.
The address in question is the one the KERNEL computes from: the crop origin of tsvpp_convert, the box origin of the ROI calls (the host advances the planes
to it with 64-bit arithmetic), the frame's own planes in the calls that sample the whole frame, the output pointer.

Host logic (the pitch and placement rules) is plain Python; only Arena touches the device."""
import numpy as np
import torch

FILL = 0xA7
MARGIN = 1 << 32
SLACK = 256 << 20                    # room for the planes of a batch side by side, and for an output's offset
ARENA_BYTES = 2 * MARGIN + SLACK     # 8.25 GiB
SPAN_LIMIT = (1 << 32) - 16          # include/tsvpp.h: TSVPP_SOURCE_SPAN_LIMIT
SLOT = 8192                          # the planes of a call start in columns of their own, this far apart (the widest frame of the grid is 3840 bytes)


def span(rows, row_bytes, pitch):
    return (rows - 1) * pitch + row_bytes


def class_range(rows, row_bytes, cls):
    """[least, greatest] pitch that puts the span of `rows` rows of `row_bytes` bytes into
    class "A": (2^31, 2^31 + one row]  -- just past the sign bit;
    class "B": [limit - one row, limit) -- within one row under TSVPP_SOURCE_SPAN_LIMIT."""
    assert rows >= 5, "fewer than 5 rows: the pitch would not fit 31 bits"
    if cls == "A":
        lo, hi = ((1 << 31) - row_bytes) // (rows - 1) + 1, ((1 << 31) - row_bytes) // (rows - 2)   # span > 2^31; (rows - 2) * pitch + row_bytes <= 2^31
        ok = lambda p: (1 << 31) < span(rows, row_bytes, p) <= (1 << 31) + p
    else:
        lo, hi = -((row_bytes - SPAN_LIMIT) // rows), (SPAN_LIMIT - 1 - row_bytes) // (rows - 1)    # rows * pitch + row_bytes >= limit; span < limit
        ok = lambda p: SPAN_LIMIT - p <= span(rows, row_bytes, p) < SPAN_LIMIT
    assert lo + 32 <= hi and ok(lo) and ok(hi) and not ok(lo - 1) and not ok(hi + 1) and row_bytes <= lo and hi < (1 << 31), (rows, row_bytes, cls, lo, hi)
    return lo, hi


def pitch_pair(rows, row_bytes, residues, cls):
    """(luma pitch, chroma pitch) for a region of `rows` luma rows and rows / 2 chroma rows, congruent to `residues` mod 16, each plane's span in class `cls`.
    The luma pitch is the greatest of its class; the chroma pitch is one of its own -- the least of its class that is at least twice the luma pitch (there is
    one: the classes of rows / 2 rows start at or below that) -- so that chroma row s stays within a few KiB of luma row 2 s, to its right, and the planes of
    several frames can interleave column by column.  A chroma pitch far from twice the luma pitch sweeps its rows across every column of a tall frame."""
    lo, hi = class_range(rows, row_bytes, cls)
    py = hi - (hi - residues[0]) % 16
    lo2, hi2 = class_range(rows // 2, row_bytes, cls)
    t = max(lo2, 2 * py)
    puv = t + (residues[1] - t) % 16
    assert lo <= py <= hi and lo2 <= puv <= hi2 and py % 16 == residues[0] and puv % 16 == residues[1] and puv != py, (rows, row_bytes, residues, cls, py, puv)
    return py, puv


class Plane:
    """rows [first, first + rows) x `row_bytes` bytes of a plane whose row 0 starts `lead` bytes before the address the kernel is handed"""

    def __init__(self, rows, row_bytes, pitch, lead=0, first=0, total_bytes=None):
        self.rows, self.row_bytes, self.pitch, self.lead, self.first = rows, row_bytes, pitch, lead, first
        self.width_bytes = row_bytes if total_bytes is None else total_bytes  # bytes written per row (the frame's whole width), from the row's first byte
        self.base = None  # arena offset of the plane's row 0, byte 0 (what the library is given)

    @property
    def seen(self):
        """arena offset of the address the kernel is handed"""
        return self.base + self.lead

    def intervals(self):
        s = self.base + (self.first + np.arange(self.rows, dtype=np.int64)) * self.pitch
        return s, s + self.width_bytes


def place(planes):
    """gives every plane a base: 256-byte aligned (what tsvpp_describe assumes), the kernel's address at least MARGIN from both ends of the arena, no two rows
    of the call overlapping (planes of differing pitch interleave: a slot is moved until its rows are clear of every row placed before)"""
    starts, ends = np.empty(0, np.int64), np.empty(0, np.int64)
    for q, p in enumerate(planes):
        for k in range(256):
            want = MARGIN + (q + len(planes) * k) * SLOT  # the least offset the kernel's address may have
            p.base = -((p.lead - want) // 256) * 256       # least multiple of 256 with base + lead >= want
            assert p.base >= 0, f"plane {q}: its row 0 lies {p.lead} bytes before the kernel's address, beyond the margin"
            s, e = p.intervals()
            i = np.searchsorted(ends, s, side="right")      # per row: the first placed row that ends after it starts
            hit = i < len(starts)
            if not (starts[i[hit]] < e[hit]).any():          # ... and none of those starts before it ends
                break
        else:
            raise AssertionError(f"plane {q}: no free slot")
        order = np.argsort(np.concatenate([starts, s]), kind="stable")
        starts, ends = np.concatenate([starts, s])[order], np.concatenate([ends, e])[order]
        assert (starts[1:] >= ends[:-1]).all(), "rows of the call overlap"
        check_margins(p.seen, span(p.rows, p.row_bytes, p.pitch))
    return planes


def check_margins(seen, nbytes):
    """THE requirement of the design: [seen - 2^32, seen + 2^32) is arena -- and so is whatever is legitimately addressed from `seen`"""
    assert seen - MARGIN >= 0 and seen + MARGIN <= ARENA_BYTES, f"the address at arena offset {seen} has no margin of 2^32 bytes on both sides"
    assert 0 < nbytes <= MARGIN and seen + nbytes <= ARENA_BYTES


class Arena:
    def __init__(self, device):
        self.buf = torch.full((ARENA_BYTES,), FILL, dtype=torch.uint8, device=device)  # (an allocation that fails raises: the test fails, it does not skip)
        assert self.buf.data_ptr() % 256 == 0
        self.words = self.buf.view(torch.int64)
        self.fill_word = int(np.frombuffer(bytes([FILL]) * 8, np.int64)[0])

    def rows(self, plane):
        """the written rows of a placed plane as a strided (rows, width_bytes) view"""
        return self.buf.as_strided((plane.rows, plane.width_bytes), (plane.pitch, 1), plane.base + plane.first * plane.pitch)

    def handle(self, plane):
        """what the facade reads of a plane -- data_ptr() and stride(0): a two-row view at the plane's base (the frame may be taller than the arena)"""
        return self.buf.as_strided((2, plane.width_bytes), (plane.pitch, 1), plane.base)

    def write(self, plane, data):
        self.rows(plane).copy_(data)

    def erase(self, plane):
        self.rows(plane).fill_(FILL)

    def untouched(self, lo, hi):
        """does [lo, hi) (multiples of 8) still hold the fill byte?  One reduction on the device."""
        assert lo % 8 == 0 and hi % 8 == 0 and 0 <= lo <= hi <= ARENA_BYTES
        return not bool((self.words[lo // 8: hi // 8] != self.fill_word).any())

    def first_touched(self, lo, hi):
        bad = torch.nonzero(self.buf[lo:hi] != FILL)
        return None if bad.numel() == 0 else lo + int(bad[0])

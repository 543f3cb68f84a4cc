"""The guard-byte arena of the tile paths' test_unaligned_outputs_and_guard_bytes: output slots carved out of one patterned buffer, so that a store before or
after an output shows.  Written against a `device` argument: tests/test_guard_arena_cpu.py runs it without a GPU."""
import bisect

import torch

GUARD = 256    # bytes of pattern before the first slot, after the last, and at least that between two
POISON = 0xA5  # what the slots hold before the call


def arena(nbytes, off, device="cuda", what="output", where=""):
    """one slot of nbytes[k] bytes per output, each `off` bytes past a 16-byte boundary, in a buffer of a period-4096 pattern -> (buf, slots, verify): the
    buffer, the slots as uint8 tensors (poisoned), and verify(), which raises unless every byte outside the slots still equals the pattern, saying which
    output the first damaged byte belongs to and at what distance from its start"""
    starts, base = [], 0
    for nb in nbytes:
        starts.append(base + GUARD + off)
        base += ((GUARD + off + nb + 15) // 16 * 16 + GUARD + 255) // 256 * 256
    total = base + GUARD
    tile = (torch.arange(4096, device=device, dtype=torch.int32) * 131 + 17).remainder(251).to(torch.uint8)
    pat = tile.repeat((total + 4095) // 4096)[:total]
    buf = pat.clone()
    assert buf.data_ptr() % 16 == 0
    slots = []
    for s, nb in zip(starts, nbytes):
        buf[s:s + nb] = POISON
        slots.append(buf[s:s + nb])
        assert slots[-1].data_ptr() % 16 == off

    def verify():
        want = buf.clone()
        for s, nb in zip(starts, nbytes):
            want[s:s + nb] = pat[s:s + nb]
        if not torch.equal(want, pat):
            bad = torch.nonzero(want != pat).flatten()[0].item()
            k = bisect.bisect_right(starts, bad + GUARD + off) - 1  # a slot's stride begins GUARD + off bytes before it; the bytes after the last slot are its own
            raise AssertionError(f"guard byte damaged at {bad - starts[k]} relative to {what} {k} of {nbytes[k]} bytes (offset {off}, {where})")

    return buf, slots, verify

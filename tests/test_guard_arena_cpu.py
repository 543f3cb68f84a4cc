"""CPU: tests/guard_util.py's arena on device="cpu" -- the one shared piece whose failure would be to check nothing, silently."""
import pytest
import torch

from guard_util import GUARD, POISON, arena

SIZES = [100, 37, 4096]  # no multiple of 16 among the first two: the gaps between the slots are of different lengths


def fill(slots):
    for s in slots:
        s.fill_(7)


@pytest.mark.parametrize("off", [0, 1, 4])
@pytest.mark.parametrize("nbytes", [SIZES, [100]])
def test_slots_sit_at_the_offset_and_writes_inside_them_pass(nbytes, off):
    buf, slots, verify = arena(nbytes, off, device="cpu")
    assert len(slots) == len(nbytes) and buf.device.type == "cpu"
    for s, nb in zip(slots, nbytes):
        assert s.data_ptr() % 16 == off and s.numel() == nb and s.dtype == torch.uint8 and bool((s == POISON).all())
    assert slots[0].data_ptr() - buf.data_ptr() == GUARD + off
    for a, b in zip(slots, slots[1:]):
        assert b.data_ptr() - (a.data_ptr() + a.numel()) >= GUARD
    assert buf.data_ptr() + buf.numel() - (slots[-1].data_ptr() + slots[-1].numel()) >= GUARD
    verify()  # poisoned slots, untouched guards
    fill(slots)
    verify()
    assert all(bool((s == 7).all()) for s in slots)  # the slots are views of the buffer verify() looks at


@pytest.mark.parametrize("off", [0, 1, 4])
@pytest.mark.parametrize("nbytes", [SIZES, [100]])
def test_a_byte_outside_the_slots_is_found_and_named(nbytes, off):
    n = len(nbytes)
    buf, slots, verify = arena(nbytes, off, device="cpu", what="output", where="here")
    starts = [s.data_ptr() - buf.data_ptr() for s in slots]
    fill(slots)

    def damaged(at):
        """verify()'s message while the byte at buffer offset `at` is changed; it passes again once the byte is back"""
        buf[at] ^= 0xFF
        with pytest.raises(AssertionError) as e:
            verify()
        buf[at] ^= 0xFF
        verify()
        return str(e.value)

    def message(distance, k):
        return f"guard byte damaged at {distance} relative to output {k} of {nbytes[k]} bytes (offset {off}, here)"
    assert damaged(0) == message(-starts[0], 0)
    assert damaged(starts[0] - 1) == message(-1, 0)                     # the byte just before the first slot
    assert damaged(starts[-1] + nbytes[-1]) == message(nbytes[-1], n - 1)  # ... just after the last
    assert damaged(buf.numel() - 1) == message(buf.numel() - 1 - starts[-1], n - 1)
    if n > 1:  # the gap between slots 0 and 1: its first byte, and its last, which lies in slot 1's stride
        assert damaged(starts[0] + nbytes[0]) == message(nbytes[0], 0)
        assert damaged(starts[1] - 1) == message(-1, 1)

"""CPU: the arena helper of the memory-contract tests (tests/arena.py) itself."""
import pytest
import torch

from tests.arena import ALIGN, GUARD, PATTERN, Arena, ArenaError


def _arena():
    ar = Arena(1 << 20, "cpu")
    a = ar.carve((3, 5, 7), torch.float32, name="a")
    v = ar.carve_view((3, 4, 6), torch.float32, (4 * 40, 40, 1), name="v")
    i = ar.carve_view((3, 4, 5), torch.int64, (33, 7, 1), name="i")
    m = ar.carve((3, 5, 1), torch.uint8, name="m")
    return ar, a, v, i, m


def test_pattern_reads_as_nan_and_minus_one():
    ar = Arena(4096 + 12 * GUARD, "cpu")
    for dt in (torch.float32, torch.float64, torch.bfloat16):
        assert torch.isnan(ar.carve((9,), dt)).all()
    for dt in (torch.int32, torch.int64):
        assert (ar.carve((9,), dt) == -1).all()
    assert (ar.carve((9,), torch.uint8) == PATTERN).all()
    ar.check()


def test_clean_arena_passes_and_writes_inside_tensors_are_free():
    ar, a, v, i, m = _arena()
    ar.check()
    a.normal_()
    v.copy_(torch.randn(3, 4, 6))
    i.copy_(torch.randint(0, 5, (3, 4, 5)))
    m.zero_()
    ar.check()
    assert torch.isfinite(a).all() and torch.isfinite(v).all() and (i >= 0).all()


def test_carved_tensors_have_the_promised_shape_alignment_and_strides():
    ar, a, v, i, m = _arena()
    assert a.shape == (3, 5, 7) and a.is_contiguous()
    assert v.shape == (3, 4, 6) and v.stride() == (160, 40, 1)
    assert i.shape == (3, 4, 5) and i.stride() == (33, 7, 1) and i.dtype == torch.int64
    for t in (a, v, i, m):
        assert t.data_ptr() % ALIGN == 0
    # float strides are multiples of 4 elements: every row starts 16-byte aligned
    for b in range(3):
        for t in range(4):
            assert v[b, t].data_ptr() % ALIGN == 0
    with pytest.raises(ValueError, match="multiple of 4"):
        ar.carve_view((2, 3, 4), torch.float32, (50, 6, 1))
    with pytest.raises(ValueError, match="overlap"):
        ar.carve_view((2, 3, 8), torch.float32, (12, 4, 1))
    with pytest.raises(ValueError, match="guard"):
        ar.carve((4,), torch.float32, guard=64)
    # the guards: the tensors lie at least GUARD bytes apart and from the buffer's ends
    spans = sorted((base, end) for _, _, base, end, _ in ar.entries)
    assert spans[0][0] >= GUARD and ar.buf.numel() - spans[-1][1] >= GUARD
    for (_, e0), (b1, _) in zip(spans, spans[1:]):
        assert b1 - e0 >= GUARD


def test_a_view_shares_no_byte_with_its_gaps():
    ar, a, v, i, m = _arena()
    v.fill_(1.0)
    base = next(b for n, _, b, _, _ in ar.entries if n == "v")
    raw = ar.buf[base:base + 4 * (2 * 160 + 3 * 40 + 6)].view(torch.float32)
    assert torch.isnan(raw[6:40]).all() and torch.isnan(raw[3 * 40 + 6:160]).all() and (raw[:6] == 1).all()
    ar.check()


@pytest.mark.parametrize("side", ["before", "after"])
def test_a_byte_flipped_in_a_guard_names_the_tensor(side):
    ar, a, v, i, m = _arena()
    _, lo, base, end, hi = next(e for e in ar.entries if e[0] == "i")
    ar.buf[base - 3 if side == "before" else end + 5] = 0
    with pytest.raises(ArenaError, match=f"guard {side} i"):
        ar.check()


def test_a_byte_flipped_in_a_gap_names_the_view():
    ar, a, v, i, m = _arena()
    base = next(b for n, _, b, _, _ in ar.entries if n == "v")
    ar.buf[base + 4 * 6] = 0  # the first float after row [0, 0]'s six
    with pytest.raises(ArenaError, match="gap between the rows of v"):
        ar.check("after the launch")
    ar.buf[base + 4 * 6] = PATTERN
    ar.check()


def test_full_arena_raises():
    ar = Arena(4 * GUARD, "cpu")
    ar.carve((16,), torch.float32)
    with pytest.raises(ArenaError, match="full"):
        ar.carve((1 << 16,), torch.float32)

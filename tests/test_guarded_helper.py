"""tests/guarded.py on CPU tensors: the evidence that the guard-band harness of
tests/test_gpu_bounds.py bites — an untouched buffer passes, one changed byte in the front
guard, the back guard or a pitch gap fails with its offset named, and the two-poison rule
catches an element a kernel never wrote.  No kernel is involved (and none is ever made to
write out of bounds to show this)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from guarded import (GUARD_MIN, POISONS, guard_bytes_for, guarded, guarded_pitched,  # noqa: E402
                     padded_input, skewed)


@pytest.mark.parametrize("poison", POISONS)
def test_untouched_buffer_passes(poison):
    t, check = guarded(torch, (5, 512), torch.float32, poison, device="cpu")
    assert t.shape == (5, 512) and t.dtype == torch.float32 and t.is_contiguous()
    assert t.data_ptr() % 256 == 0
    assert (t.view(torch.uint8) == poison).all()           # the payload is poisoned too
    check()
    t.fill_(1.0)                                            # writing the payload is allowed
    check()


def test_guard_size():
    """At least 64 KB and at least two rows of the case at hand."""
    assert guard_bytes_for(512) == GUARD_MIN
    assert guard_bytes_for(4444 * 4 * 5) >= 2 * 4444 * 4 * 5
    t, check = guarded(torch, (3, 40000), torch.float32, 0xA5, device="cpu")
    off = check.off
    assert off >= 2 * 160000 and check.buf.numel() - off - t.numel() * 4 >= 2 * 160000
    # one row, one 16-row block or one 512-column tile past a [5, 512] fp32 payload stays inside
    t, check = guarded(torch, (5, 512), torch.float32, 0xA5, device="cpu")
    assert check.buf.numel() - check.off - 5 * 2048 >= 16 * 2048


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("where,offset", [("front", -1), ("front", -4096), ("back", 0),
                                          ("back", 3 * 2048 + 17)])
def test_one_changed_guard_byte_fails_with_offset(poison, where, offset):
    t, check = guarded(torch, (7, 512), torch.int8, poison, device="cpu", name="out8")
    nbytes = 7 * 512
    rel = offset if where == "front" else nbytes + offset
    check.buf[check.off + rel] = poison ^ 0xFF
    with pytest.raises(AssertionError) as e:
        check()
    msg = str(e.value)
    assert f"{where} guard" in msg and f"byte offset {rel} " in msg and "out8" in msg


def test_first_change_is_reported():
    t, check = guarded(torch, (4,), torch.float32, 0x5A, device="cpu")
    check.buf[check.off + 16 + 100] = 0
    check.buf[check.off + 16 + 7] = 0
    with pytest.raises(AssertionError, match="byte offset 23 "):
        check()


@pytest.mark.parametrize("poison", POISONS)
def test_pitched_gap_is_guard(poison):
    """Q|K|V rows of 1536 bytes at a pitch of 1600: the 64 gap bytes of every row are guard."""
    M = 7
    t, check = guarded_pitched(torch, M, 1536, 1600, torch.int8, poison, device="cpu")
    assert t.shape == (M, 1536) and t.stride() == (1600, 1) and t.data_ptr() % 256 == 0
    check()
    t.fill_(3)                       # every payload byte written: the gaps stay poisoned
    check()
    assert (check.buf[check.off:check.off + 6 * 1600 + 1536].view(torch.int8) == 3).sum() == M * 1536
    at = 4 * 1600 + 1536 + 9         # a byte in the gap after row 4
    check.buf[check.off + at] = poison ^ 0x01
    with pytest.raises(AssertionError) as e:
        check()
    assert "pitch gap after row 4" in str(e.value) and f"byte offset {at} " in str(e.value)
    check.buf[check.off + at] = poison
    check()
    check.buf[check.off + 6 * 1600 + 1536] = 0     # the byte after the last row: back guard
    with pytest.raises(AssertionError, match="back guard changed at byte offset 11136 "):
        check()


def test_pitched_floats():
    """Scales [3][M] with a tile stride of M + 3 floats: the 3 gap floats per tile are guard."""
    M = 5
    t, check = guarded_pitched(torch, 3, 4 * M, 4 * (M + 3), torch.float32, 0xA5, device="cpu")
    assert t.shape == (3, M) and t.stride() == (M + 3, 1)
    t.copy_(torch.arange(15, dtype=torch.float32).view(3, M))
    check()
    flat = check.buf[check.off:check.off + 4 * (2 * (M + 3) + M)].view(torch.float32)
    flat[M] = 0.0                                   # the first gap float of tile 0
    with pytest.raises(AssertionError, match=f"pitch gap after row 0 changed at byte offset {4 * M} "):
        check()


def _run_fake_kernel(poison, skip):
    """A stand-in for a kernel + oracle comparison: writes every expected element except
    (when skip) one whose expected bytes equal one of the poisons; returns whether the full
    payload equals the expectation."""
    want = np.arange(64, dtype=np.int8).reshape(4, 16)
    want[2, 5] = np.int8(np.uint8(0xA5).view(np.int8))      # an expected value that IS a poison
    t, check = guarded(torch, want.shape, torch.int8, poison, device="cpu")
    out = torch.from_numpy(want.copy())
    if skip:
        out[2, 5] = t[2, 5]                                  # "never written": keeps the poison
    t.copy_(out)
    check()
    return np.array_equal(t.numpy(), want)


def test_two_poisons_catch_an_unwritten_element():
    """An unwritten element can equal the expectation under one poison (here the expected
    byte is 0xA5 itself), never under both: the case fails for at least one parameter."""
    assert all(_run_fake_kernel(p, skip=False) for p in POISONS)
    results = [_run_fake_kernel(p, skip=True) for p in POISONS]
    assert results == [True, False]          # 0xA5 hides it, 0x5A exposes it
    # the same for a ReLU hidden's most common code, 0, over what would be a zeroed buffer
    for p in POISONS:
        t, _ = guarded(torch, (8,), torch.int8, p, device="cpu")
        assert not (t == 0).any()
    # and for fp32: neither poison pattern is a value a kernel result compares equal to
    for p in POISONS:
        t, _ = guarded(torch, (8,), torch.float32, p, device="cpu")
        v = float(t[0])
        assert v != 0.0 and (abs(v) > 1e12 or abs(v) < 1e-12)


def test_padded_input_rows():
    x = np.arange(12, dtype=np.float32).reshape(3, 4)
    t = padded_input(torch, x, 7, np.nan, device="cpu").numpy()
    assert t.size >= 3 * 7 + 7
    for r in range(3):
        np.testing.assert_array_equal(t[7 * r:7 * r + 4], x[r])
        assert np.isnan(t[7 * r + 4:7 * (r + 1)]).all()
    assert np.isnan(t[3 * 7:]).all()                 # the tail after the last row
    q = np.full((2, 8), -3, np.int8)
    t = padded_input(torch, q, 24, 0x7f, device="cpu").numpy()
    assert (t[8:24] == 127).all() and (t[24:32] == -3).all() and (t[32:] == 127).all()


def test_padded_input_mask_complement():
    """A [B, Sq, Sk] mask at strides (m_bs, m_is) = (Sq * m_is + 11, Sk + 5): every gap holds
    the complement of the neighbouring mask value, so a kernel that reads a gap as a mask
    element sees the opposite decision."""
    B, Sq, Sk = 2, 3, 4
    m = np.ones((B, Sq, Sk), np.uint8)
    m[0, 1, 2:] = 0
    m[1, :, 3] = 0
    m_is, m_bs = Sk + 5, Sq * (Sk + 5) + 11
    t = padded_input(torch, m, (m_bs, m_is), "complement", device="cpu").numpy()
    for b in range(B):
        for i in range(Sq):
            o = b * m_bs + i * m_is
            np.testing.assert_array_equal(t[o:o + Sk], m[b, i])
            nxt = (b * m_bs + (i + 1) * m_is) if i + 1 < Sq else (b + 1) * m_bs
            assert (t[o + Sk:nxt] == (m[b, i, -1] == 0)).all()
    assert t.size >= B * m_bs


# ---- skew: payloads at the least alignment include/qtx.h accepts (16 mod 256) -------------
@pytest.mark.parametrize("skew", [0, 16, 48, 240])
def test_skew_sets_the_address_residue(skew):
    t, check = guarded(torch, (5, 512), torch.float32, 0xA5, device="cpu", skew=skew)
    assert t.data_ptr() % 256 == skew and t.data_ptr() == check.buf.data_ptr() + check.off
    assert t.shape == (5, 512) and t.is_contiguous() and (t.view(torch.uint8) == 0xA5).all()
    # the guards keep their minimum sizes
    assert check.off >= GUARD_MIN and check.buf.numel() - check.off - 5 * 2048 >= GUARD_MIN
    check()
    p, pc = guarded_pitched(torch, 7, 1536, 1600, torch.int8, 0xA5, device="cpu", skew=skew)
    assert p.data_ptr() % 256 == skew and p.stride() == (1600, 1)
    assert pc.off >= GUARD_MIN and pc.buf.numel() - pc.off - (6 * 1600 + 1536) >= GUARD_MIN
    pc()
    x = np.arange(35, dtype=np.float32).reshape(5, 7)
    s = skewed(torch, x, skew, device="cpu")
    assert s.data_ptr() % 256 == skew and s.is_contiguous()
    np.testing.assert_array_equal(s.numpy(), x)
    ids = skewed(torch, np.arange(6, dtype=np.int64).reshape(2, 3), skew, device="cpu")
    assert ids.data_ptr() % 256 == skew and ids.dtype == torch.int64
    q = padded_input(torch, np.full((2, 8), -3, np.int8), 24, 0x7f, device="cpu", skew=skew)
    assert q.data_ptr() % 256 == skew
    assert (q.numpy()[8:24] == 127).all() and (q.numpy()[24:32] == -3).all()


@pytest.mark.parametrize("skew", [4, 8, 24, 256, -16])
def test_skew_must_be_a_multiple_of_16_below_256(skew):
    with pytest.raises(AssertionError):
        guarded(torch, (4,), torch.float32, 0xA5, device="cpu", skew=skew)
    with pytest.raises(AssertionError):
        skewed(torch, np.zeros(4, np.float32), skew, device="cpu")


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("where,offset", [("front", -1), ("front", -16), ("front", -4096),
                                          ("back", 0), ("back", 15), ("back", 3 * 2048 + 17)])
def test_skewed_guard_byte_fails_with_offset(poison, where, offset):
    """The byte just before and just after a payload at 16 (mod 256) is guard, and a change
    is reported relative to the payload, not to the 256-byte boundary below it."""
    t, check = guarded(torch, (7, 512), torch.int8, poison, device="cpu", name="out8", skew=16)
    nbytes = 7 * 512
    rel = offset if where == "front" else nbytes + offset
    raw = check.buf.numpy()
    addr = t.data_ptr() + rel - check.buf.data_ptr()        # located through the payload's address
    raw[addr] = poison ^ 0xFF
    with pytest.raises(AssertionError) as e:
        check()
    msg = str(e.value)
    assert f"{where} guard" in msg and f"byte offset {rel} " in msg and "out8" in msg
    raw[addr] = poison
    t.fill_(1)                                               # the payload itself is not guard
    check()


def test_skewed_pitched_gaps_are_checked():
    M = 7
    t, check = guarded_pitched(torch, M, 1536, 1600, torch.int8, 0x5A, device="cpu", skew=16)
    t.fill_(3)
    check()
    raw = check.buf.numpy()
    base = t.data_ptr() - check.buf.data_ptr()
    assert (raw[base:base + 6 * 1600 + 1536].view(np.int8) == 3).sum() == M * 1536
    at = 2 * 1600 + 1536                   # the first gap byte after row 2
    raw[base + at] = 0
    with pytest.raises(AssertionError) as e:
        check()
    assert "pitch gap after row 2" in str(e.value) and f"byte offset {at} " in str(e.value)
    raw[base + at] = 0x5A
    raw[base - 1] = 0                      # the byte before row 0
    with pytest.raises(AssertionError, match="front guard changed at byte offset -1 "):
        check()
    raw[base - 1] = 0x5A
    raw[base + 6 * 1600 + 1536] = 0        # the byte after the last row
    with pytest.raises(AssertionError, match="back guard changed at byte offset 11136 "):
        check()

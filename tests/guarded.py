"""Guard-band buffers for the kernel tests (a helper module, not a conftest).

A kernel output is allocated inside one uint8 buffer laid out as

    front guard | payload | back guard

and the whole buffer is filled with one poison byte before the call.  After the call
check() asserts that both guards (and, for a pitched payload, the gaps between its rows)
still hold the poison, and reports the byte offset of the first change relative to the
payload.  Each guard is at least 64 KB and at least two rows (pitches) of the payload, so a
realistic stray store — one row, one 16-row block, one 512-column tile past the end — lands
inside the allocation, where the check sees it, and never outside it.

Two poison bytes (POISONS) are used as a parametrize of every GPU case: the full payload
is compared with the oracle, and an element the kernel never wrote holds the poison, which
cannot equal the expected value under both bytes.

padded_input() embeds an *input's* rows at a wider pitch and fills the gaps and a tail with
a value that changes the result if a kernel uses it (NaN for fp32 rows and partial maxima,
0x7f for int8 codes, the complement of the neighbouring value for masks); it asserts only
through results.

Every payload and input is 256-byte aligned by default; skew=16 (any multiple of 16 below
256) puts it at that residue instead — 16 (mod 256) is the least alignment include/qtx.h
accepts, the case of a caller that sub-allocates one arena or passes a view.  skewed() does
the same for a plain exact-size input.

Works on CPU tensors too (tests/test_guarded_helper.py), device="cpu".
"""
import numpy as np

POISONS = (0xA5, 0x5A)
GUARD_MIN = 64 * 1024
ALIGN = 256


def _round_up(n, a):
    return (n + a - 1) // a * a


def _first_change(seg, poison):
    """Index of the first byte of the uint8 tensor `seg` that is not `poison`, or -1."""
    bad = seg != poison
    if not bool(bad.any()):
        return -1
    return int(bad.nonzero()[0, 0])


class _Check:
    """check() of one guarded buffer; callable, and keeps the whole buffer alive."""

    def __init__(self, buf, off, segments, poison, name):
        self.buf, self.off, self.segments, self.poison, self.name = buf, off, segments, poison, name

    def __call__(self):
        # segments: (start, stop, label) in bytes relative to the payload start
        for start, stop, label in self.segments:
            i = _first_change(self.buf[self.off + start:self.off + stop], self.poison)
            if i >= 0:
                got = int(self.buf[self.off + start + i])
                raise AssertionError(
                    f"{self.name}: {label} changed at byte offset {start + i} relative to the "
                    f"payload (poison 0x{self.poison:02X}, found 0x{got:02X})")


def _check_skew(skew):
    assert 0 <= skew < ALIGN and skew % 16 == 0, f"skew {skew}: a multiple of 16 below {ALIGN}"
    return int(skew)


def _alloc(torch, payload_bytes, guard_bytes, poison, device, skew=0):
    skew = _check_skew(skew)
    total = 2 * guard_bytes + payload_bytes + ALIGN + skew
    buf = torch.full((total,), poison, dtype=torch.uint8, device=device)
    off = guard_bytes + (-(buf.data_ptr() + guard_bytes)) % ALIGN + skew
    assert (buf.data_ptr() + off) % ALIGN == skew and off + payload_bytes + guard_bytes <= total
    return buf, off, total


def guard_bytes_for(pitch_bytes):
    """At least 64 KB and at least two rows of the case at hand, a multiple of 256."""
    return _round_up(max(GUARD_MIN, 2 * int(pitch_bytes)), ALIGN)


def guarded(torch, shape, dtype, poison, device="cuda", name="buffer", pitch_bytes=None,
            skew=0):
    """A contiguous payload of `shape` / `dtype` between two poisoned guards.

    Returns (payload, check): payload is a view of the buffer (poisoned; its address is
    `skew` mod 256, skew a multiple of 16: 0 by default, 16 = the least alignment
    include/qtx.h accepts), check() asserts that both guards still hold the poison.
    pitch_bytes: the row size the guards are sized for (default: the payload's last
    dimension)."""
    shape = tuple(int(s) for s in (shape if hasattr(shape, "__len__") else (shape,)))
    item = torch.empty((), dtype=dtype).element_size()
    n = int(np.prod(shape)) if shape else 1
    nbytes = n * item
    row = pitch_bytes if pitch_bytes is not None else (shape[-1] if shape else 1) * item
    gb = guard_bytes_for(row)
    buf, off, total = _alloc(torch, nbytes, gb, poison, device, skew)
    payload = buf[off:off + nbytes].view(dtype).view(shape)
    segs = [(-off, 0, "front guard"), (nbytes, total - off, "back guard")]
    return payload, _Check(buf, off, segs, poison, name)


def guarded_pitched(torch, rows, row_bytes, pitch_bytes, dtype, poison, device="cuda",
                    name="buffer", skew=0):
    """`rows` rows of `row_bytes` bytes, `pitch_bytes` apart; the gap bytes between the rows
    are guard too (the payload ends with the last row's last byte).

    Returns (payload, check): payload is a strided [rows, row_bytes / itemsize] view."""
    item = torch.empty((), dtype=dtype).element_size()
    assert row_bytes <= pitch_bytes and row_bytes % item == 0 and pitch_bytes % item == 0
    nbytes = (rows - 1) * pitch_bytes + row_bytes
    gb = guard_bytes_for(pitch_bytes)
    buf, off, total = _alloc(torch, nbytes, gb, poison, device, skew)
    flat = buf[off:off + _round_up(nbytes, item)].view(dtype)
    payload = torch.as_strided(flat, (rows, row_bytes // item), (pitch_bytes // item, 1))
    segs = [(-off, 0, "front guard")]
    if pitch_bytes > row_bytes and rows > 1:
        segs.append(("gaps", row_bytes, pitch_bytes, rows - 1))
    segs.append((nbytes, total - off, "back guard"))
    return payload, _PitchedCheck(buf, off, segs, poison, name)


class _PitchedCheck(_Check):
    def __call__(self):
        plain = [s for s in self.segments if s[0] != "gaps"]
        for _, row_bytes, pitch, ngaps in (s for s in self.segments if s[0] == "gaps"):
            # gap g covers [g * pitch + row_bytes, (g + 1) * pitch): one strided view of them all
            base = self.buf[self.off:self.off + ngaps * pitch].view(ngaps, pitch)[:, row_bytes:]
            bad = base != self.poison
            if bool(bad.any()):
                g, c = (int(v) for v in bad.nonzero()[0])
                at = g * pitch + row_bytes + c
                got = int(self.buf[self.off + at])
                raise AssertionError(
                    f"{self.name}: pitch gap after row {g} changed at byte offset {at} relative "
                    f"to the payload (poison 0x{self.poison:02X}, found 0x{got:02X})")
        _Check(self.buf, self.off, plain, self.poison, self.name)()


def skewed(torch, array, skew=0, device="cuda"):
    """A plain exact-size input: the device copy of the numpy `array` at an address that is
    `skew` mod 256 (a view into a slightly larger allocation, which it keeps alive)."""
    a = np.ascontiguousarray(array)
    skew = _check_skew(skew)
    src = torch.from_numpy(a)
    if skew == 0 and device != "cpu":
        return src.to(device)                   # a fresh allocation: at least 256-byte aligned
    nbytes = a.size * a.itemsize
    buf = torch.zeros((nbytes + 2 * ALIGN,), dtype=torch.uint8, device=device)
    off = (-buf.data_ptr()) % ALIGN + skew
    t = buf[off:off + nbytes].view(src.dtype).view(a.shape)
    assert t.data_ptr() % ALIGN == skew
    t.copy_(src)
    return t


def padded_input(torch, array, pitch, fill, device="cuda", skew=0):
    """The rows of `array` embedded at wider strides, gaps and a tail filled with `fill`.

    array: numpy [..., W].  pitch: the row stride in elements (2-D arrays), or a tuple of
    element strides of the leading dimensions (N-D arrays, e.g. (m_bs, m_is) of a mask).
    fill: a value of the array's dtype (NaN, 0x7f, ...) or "complement": each gap element
    holds the complement (0 <-> 1) of the nearest payload element before it.
    Returns the flat device tensor; element [i, j, ..., w] sits at i*stride0 + j*stride1 + w.
    The tail after the last row is one more outermost stride (at least 64 elements).
    skew: the tensor's address mod 256, as in skewed()."""
    a = np.ascontiguousarray(array)
    strides = (pitch,) if np.isscalar(pitch) else tuple(pitch)
    assert len(strides) == a.ndim - 1 and strides[-1] >= a.shape[-1]
    for d in range(len(strides) - 1):
        assert strides[d] >= strides[d + 1] * a.shape[d + 1]
    lead = np.indices(a.shape[:-1]).reshape(a.ndim - 1, -1)
    row0 = sum(lead[d].astype(np.int64) * int(strides[d]) for d in range(a.ndim - 1))
    idx = (row0[:, None] + np.arange(a.shape[-1])[None, :]).reshape(-1)
    n = int(idx.max()) + 1 + max(int(strides[0]), 64)
    rows = a.reshape(-1)
    if isinstance(fill, str):
        assert fill == "complement"
        is_payload = np.zeros(n, bool)
        is_payload[idx] = True
        flat = np.zeros(n, a.dtype)
        flat[idx] = rows
        last = np.maximum.accumulate(np.where(is_payload, np.arange(n), 0))
        flat = np.where(is_payload, flat, (flat[last] == 0).astype(a.dtype))
    else:
        flat = np.full(n, fill, a.dtype)
        flat[idx] = rows
    return skewed(torch, flat, skew, device)

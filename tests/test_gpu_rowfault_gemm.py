"""qtx_linear_i8_rowfaults (include/qtx.h; csrc/qtx_rowfault.hip k_gemm_rowfault): the M = B GEMM
of the trials decode's eager step, where every row carries a fault of its own, against a numpy
int64 restatement of the epilogue, bit for bit.

The restatement: acc = A . W^T in int64; INPUT on row r: acc[r, lo:hi] += (flip(a) - a) *
W[lo:hi, col]; WEIGHT on row r: acc[r, wrow] += (flip(w) - w) * A[r, col], for that row alone;
y = ((float32(acc) * sa) * sw) + b; OUTPUT on row r: y[r, col] = value + b[col]; ReLU; residual.
Shapes: M = 3 and 5 (inside one 32-row tile), M = 33 (across it); N = 512 / 1536 / 2048; K = 512 /
2048.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from guarded import POISONS, guarded  # noqa: E402

pytestmark = pytest.mark.gpu
S0 = C.c_void_p(0)
f32 = np.float32
OK, E_INVALID = 0, 1
RELU, RESID = 1, 2
SHAPES = [(3, 512, 512, 0), (33, 1536, 512, 0), (33, 512, 2048, RESID), (5, 2048, 512, RELU)]
_MEMO = {}


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else S0


def F(kind, **kw):
    from qtx.fault import Fault
    return Fault(kind, 1, 0, "Q", **kw)


def table(M, N, K):
    """Row -> fault: rows 0, 31, 32 and M - 1, columns 0 and N - 1 / K - 1, INPUT16 windows at a
    32-column tile edge and at the end of the row, a WEIGHT16 window with and without row 0,
    OUTPUT, different kinds on neighbouring rows; every other row NONE."""
    t = {0: F("INPUT", row=0, col=0, bit=7),
         1: F("WEIGHT", row=N - 1, col=K - 1, bit=6),
         M - 1: F("OUTPUT", row=0, col=N - 1, value=123.5)}
    if M == 5:
        t[2] = F("WEIGHT16", row=40, col=3, bit=7, win_start=1, win_len=3)      # misses row 0
        t[3] = F("INPUT16", row=0, col=K - 1, bit=5, win_start=24, win_len=16)  # columns 24..39
    if M > 32:
        t[2] = F("OUTPUT", row=0, col=0, value=-7.25)
        t[3] = F("INPUT16", row=0, col=K - 1, bit=5, win_start=24, win_len=16)
        t[29] = F("WEIGHT16", row=64, col=70, bit=7, win_start=0, win_len=2)    # holds row 0
        t[30] = F("WEIGHT16", row=33, col=9, bit=7, win_start=1, win_len=3)     # misses row 0
        t[31] = F("INPUT16", row=0, col=7, bit=7, win_start=N - 16, win_len=16)
        t[32] = F("WEIGHT", row=0, col=0, bit=7)
    return t


def flip(v, bit):
    return np.array([v], np.int8).view(np.uint8).__xor__(np.uint8(1 << bit)).view(np.int8)[0]


def restate(qx, sx, qw, sw, b, res, flags, tab):
    M, N = qx.shape[0], qw.shape[0]
    acc = qx.astype(np.int64) @ qw.astype(np.int64).T
    for r, f in tab.items():
        c = int(f.col)
        if f.kind in ("INPUT", "INPUT16"):
            lo = int(f.win_start) if f.kind == "INPUT16" else 0
            hi = lo + int(f.win_len) if f.kind == "INPUT16" else N
            delta = int(flip(qx[r, c], f.bit)) - int(qx[r, c])
            acc[r, lo:hi] += delta * qw[lo:hi, c].astype(np.int64)
        elif f.kind in ("WEIGHT", "WEIGHT16"):
            if f.kind == "WEIGHT16" and not f.win_start <= 0 < f.win_start + f.win_len:
                continue
            n = int(f.row)
            delta = int(flip(qw[n, c], f.bit)) - int(qw[n, c])
            acc[r, n] += delta * int(qx[r, c])
    assert np.abs(acc).max() < 2 ** 31
    y = ((acc.astype(f32) * sx[:, None].astype(f32)) * sw[None, :].astype(f32)) + b[None, :]
    for r, f in tab.items():
        if f.kind == "OUTPUT":
            y[r, int(f.col)] = f32(f.value) + b[int(f.col)]
    if flags & RELU:
        y = np.where(y > 0, y, f32(0)).astype(f32)
    if flags & RESID:
        y = res + y
    return y.astype(f32)


def inputs(M, N, K):
    def make():
        rng = np.random.default_rng(1000 * M + N + K)
        qx = rng.integers(-127, 128, (M, K)).astype(np.int8)
        qw = rng.integers(-127, 128, (N, K)).astype(np.int8)
        sx = (rng.random(M) * 0.02 + 0.001).astype(f32)
        sw = (rng.random(N) * 0.002 + 0.0001).astype(f32)
        b = rng.standard_normal(N).astype(f32)
        res = rng.standard_normal((M, N)).astype(f32)
        return qx, sx, qw, sw, b, res
    key = (M, N, K)
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


def c_table(M, tab):
    from qtx import _lib
    arr = (_lib.Fault * M)()
    for r, f in tab.items():
        arr[r] = f.to_c()
    return arr


def run(torch, M, N, K, flags, tab, out=None, alias=False):
    from qtx import _lib
    qx, sx, qw, sw, b, res = inputs(M, N, K)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    resd = d(res) if flags & RESID else None
    if out is None:
        out = resd if alias else torch.empty((M, N), dtype=torch.float32, device="cuda")
    ins = [d(a) for a in (qx, sx, qw, sw, b)]      # alive until the call has run
    _lib.call("qtx_linear_i8_rowfaults", *[P(t) for t in ins], M, N, K, flags, P(resd), P(out),
              c_table(M, tab), S0)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("M,N,K,flags", SHAPES, ids=lambda v: str(v))
def test_matches_the_restatement(torch, M, N, K, flags):
    from qtx import _lib
    qx, sx, qw, sw, b, res = inputs(M, N, K)
    tab = table(M, N, K)
    want = restate(qx, sx, qw, sw, b, res, flags, tab)
    got = run(torch, M, N, K, flags, tab).cpu().numpy()
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    # rows without a fault — and the rows whose WEIGHT16 window misses row 0 — are qtx_linear_i8's
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    plain = torch.empty((M, N), dtype=torch.float32, device="cuda")
    ins = [d(a) for a in (qx, sx, qw, sw, b, res)]
    _lib.call("qtx_linear_i8", *[P(t) for t in ins[:5]], M, N, K, 8, flags,
              P(ins[5]) if flags & RESID else S0, P(plain), S0)
    plain = plain.cpu().numpy()
    base = restate(qx, sx, qw, sw, b, res, flags, {})
    np.testing.assert_array_equal(plain.view(np.uint32), base.view(np.uint32))
    miss = [r for r, f in tab.items() if f.kind == "WEIGHT16" and f.win_start > 0]
    for r in range(M):
        same = np.array_equal(got[r].view(np.uint32), plain[r].view(np.uint32))
        if r not in tab or r in miss:
            assert same, r
        else:   # (a ReLU can mask a fault: the restatement says whether the row changes)
            assert same == np.array_equal(want[r].view(np.uint32), base[r].view(np.uint32)), r
    assert not np.array_equal(got[0].view(np.uint32), plain[0].view(np.uint32))
    assert not np.array_equal(got[M - 1].view(np.uint32), plain[M - 1].view(np.uint32))
    # the empty table is qtx_linear_i8
    np.testing.assert_array_equal(run(torch, M, N, K, flags, {}).cpu().numpy().view(np.uint32),
                                  plain.view(np.uint32))


def test_residual_in_place(torch):
    """out aliases res, as the decoder's residual stream does."""
    M, N, K, flags = SHAPES[2]
    tab = table(M, N, K)
    want = restate(*inputs(M, N, K), flags, tab)
    got = run(torch, M, N, K, flags, tab, alias=True).cpu().numpy()
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


def test_a_weight_fault_is_seen_by_its_own_row_only(torch):
    """The same WEIGHT fault on rows 1 and 32, nothing on the others: two rows change."""
    M, N, K, flags = SHAPES[1]
    f = F("WEIGHT", row=700, col=100, bit=7)
    tab = {1: f, 32: f}
    want = restate(*inputs(M, N, K), flags, tab)
    base = restate(*inputs(M, N, K), flags, {})
    got = run(torch, M, N, K, flags, tab).cpu().numpy()
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    changed = sorted(set(np.nonzero((got.view(np.uint32) != base.view(np.uint32)).any(1))[0]))
    assert changed == [1, 32]


@pytest.mark.parametrize("poison", POISONS, ids=lambda p: "poison%02X" % p)
def test_extents(torch, poison):
    """Exactly out [M, N] is written, in full, at M = 33 (the second row tile holds one row)."""
    M, N, K, flags = SHAPES[1]
    tab = table(M, N, K)
    out, check = guarded(torch, (M, N), torch.float32, poison, name="out")
    run(torch, M, N, K, flags, tab, out=out)
    check()
    want = restate(*inputs(M, N, K), flags, tab)
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32))


def test_refusals(torch):
    from qtx import _lib
    M, N, K, flags = SHAPES[0]
    L_ = _lib.lib()
    qx, sx, qw, sw, b, res = inputs(M, N, K)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    out, check = guarded(torch, (M, N), torch.float32, 0x5A, name="out")
    args = [d(qx), d(sx), d(qw), d(sw), d(b)]

    def call(tab, k=K):
        rc = L_.qtx_linear_i8_rowfaults(*[P(a) for a in args], M, N, k, flags, S0, P(out),
                                        c_table(M, tab), S0)
        torch.cuda.synchronize()
        if rc != OK:
            assert bool((out.view(torch.uint8) == 0x5A).all())
        check()
        return rc

    assert call({1: F("INPUT", row=1, col=0, bit=7)}) == E_INVALID       # B = 1 coordinates: row 0
    assert call({1: F("OUTPUT", row=0, col=N, value=1.0)}) == E_INVALID
    assert call({2: F("INPUT", row=0, col=K, bit=7)}) == E_INVALID
    assert call({0: F("WEIGHT", row=N, col=0, bit=7)}) == E_INVALID
    assert call({0: F("WEIGHT", row=0, col=0, bit=8)}) == E_INVALID
    assert call({0: F("INPUT16", row=0, col=0, bit=7, win_start=N - 8, win_len=16)}) == E_INVALID
    assert call({0: F("WEIGHT16", row=0, col=0, bit=7, win_start=0, win_len=17)}) == E_INVALID
    assert call({}, k=K - 32) != OK
    assert call({0: F("INPUT", row=0, col=K - 1, bit=0)}) == OK

"""qtx_linear_rows_faults (include/qtx_enctrials.h; csrc/qtx_gemm.hip k_gemm_row's table form): the
row-complete int8 GEMM at M = B * S where every token row carries the fault entry of its own
sentence's trial, against a numpy restatement, bit for bit.

The restatement: acc = A . W^T in int64; for the entries that name this (layer, gemm) launch,
INPUT on row r: acc[r, lo:hi] += (flip(a) - a) * W[lo:hi, col]; WEIGHT on row r: acc[r, wrow] +=
(flip(w) - w) * A[r, col]; y = ((float32(acc) * sa) * sw) + b; OUTPUT on row r: y[r, col] = value +
b[col]; then the row-complete part with the oracle's quant_rows / layer_norm (ReLU first for epi
2 / 3).  M = 5 (one ragged tile), 128 (the FULL instance), 129 and 257 (a one-row last tile, entries
on both sides of a tile edge); (N, K, epi) = (512, 512, 0 and 1), (1536, 512, 0) — three column
tiles, the column offsets of Q | K | V —, (2048, 512, 2 then 3), (512, 2048, 1).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from oracle import qtx_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from guarded import POISONS  # noqa: E402
from test_gpu_bounds import Guards, P, S0, assert_ok, lib, np_, torch  # noqa: E402,F401

pytestmark = pytest.mark.gpu
f32 = np.float32
OK, E_INVALID, E_UNSUPPORTED = 0, 1, 4
NONE, INPUT, WEIGHT, OUTPUT = 0, 1, 2, 3
LAYER, GEMM = 2, 1                       # "this launch"; every other pair must be ignored
MS = [5, 128, 129, 257]
SHAPES = [(512, 512, 0), (512, 512, 1), (1536, 512, 0), (2048, 512, 23), (512, 2048, 1)]
_MEMO = {}


def memo(key, fn):
    if key not in _MEMO:
        _MEMO[key] = fn()
    return _MEMO[key]


def E(kind, layer=LAYER, gemm=GEMM, bit=0, col=0, wrow=0, lo=0, hi=0, value=0.0):
    return dict(kind=kind, layer=layer, gemm=gemm, bit=bit, col=col, wrow=wrow, lo=lo, hi=hi,
                value=value)


def table(M, N, K):
    """Row -> entry.  An INPUT over every column; an INPUT16 window (across the 512-column tile
    edge where there is one); an OUTPUT that a ReLU zeroes and one it keeps; one WEIGHT over a
    window of rows that ends at M or crosses the 128-row tile edge (rows 120 .. 135); entries that
    name another layer or another gemm; with M > 129 an INPUT on the last row."""
    w0 = 504 if N > 512 else N - 16
    t = {0: E(INPUT, bit=7, col=0, lo=0, hi=N),
         1: E(INPUT, bit=5, col=K - 1, lo=w0, hi=w0 + 16),
         2: E(OUTPUT, col=N - 1, value=-50.0),
         3: E(INPUT, layer=LAYER + 1, bit=7, col=3, lo=0, hi=N)}          # another layer
    wf = E(WEIGHT, bit=7, col=100, wrow=N - 13)
    if M == 5:
        t[4] = wf
        return t
    t[5] = E(OUTPUT, col=0, value=123.5)
    t[6] = E(OUTPUT, gemm=GEMM + 1, col=7, value=1e4)                     # another gemm
    t[7] = E(WEIGHT, layer=0, bit=6, col=1, wrow=2)                       # another layer
    for r in range(120, min(136, M)):
        t[r] = wf
    if M > 136:
        t[M - 1] = E(INPUT, bit=6, col=K // 2, lo=0, hi=N)
    return t


def flip(v, bit):
    return np.array([v], np.int8).view(np.uint8).__xor__(np.uint8(1 << bit)).view(np.int8)[0]


def inputs(M, N, K):
    def make():
        rng = np.random.default_rng(1000 * M + N + K)
        x = rng.standard_normal((M, K))
        qx, sx = O.quant_rows((np.maximum(x, 0) if K == 2048 else x).astype(f32))
        qw, sw = O.quant_weight((rng.standard_normal((N, K)) * 0.05).astype(f32), 8)
        return dict(qx=qx, sx=sx, qw=qw, sw=sw, b=rng.standard_normal(N).astype(f32),
                    res=(rng.standard_normal((M, 512)) * 2).astype(f32),
                    la=(1 + 0.1 * rng.standard_normal(512)).astype(f32),
                    lb=(0.1 * rng.standard_normal(512)).astype(f32))
    return memo(("in", M, N, K), make)


def restate_y(r, tab):
    """The MatMul output with bias, before any ReLU: the entries that name (LAYER, GEMM) applied."""
    qx, qw = r["qx"], r["qw"]
    acc = qx.astype(np.int64) @ qw.astype(np.int64).T
    mine = {k: f for k, f in tab.items() if f["layer"] == LAYER and f["gemm"] == GEMM}
    for k, f in mine.items():
        c = f["col"]
        if f["kind"] == INPUT:
            delta = int(flip(qx[k, c], f["bit"])) - int(qx[k, c])
            acc[k, f["lo"]:f["hi"]] += delta * qw[f["lo"]:f["hi"], c].astype(np.int64)
        elif f["kind"] == WEIGHT:
            delta = int(flip(qw[f["wrow"], c], f["bit"])) - int(qw[f["wrow"], c])
            acc[k, f["wrow"]] += delta * int(qx[k, c])
    assert np.abs(acc).max() < 2 ** 31
    y = ((acc.astype(f32) * r["sx"][:, None]) * r["sw"][None, :]) + r["b"][None, :]
    for k, f in mine.items():
        if f["kind"] == OUTPUT:
            y[k, f["col"]] = f32(f["value"]) + r["b"][f["col"]]
    return y.astype(f32)


def expect(M, N, K, epi, tab, key):
    """The documented outputs of the epilogue(s), by name."""
    def make():
        r = inputs(M, N, K)
        y = restate_y(r, tab)
        if epi == 0:
            qs = [O.quant_rows(y[:, 512 * t:512 * (t + 1)]) for t in range(N // 512)]
            return dict(out8=np.stack([q for q, _ in qs]), os=np.stack([s for _, s in qs]))
        if epi == 1:
            x = r["res"] + y
            q, s = O.quant_rows(O.layer_norm(x, r["la"], r["lb"]))
            return dict(xout=x, lnq=q, lns=s)
        h = np.where(y > 0, y, f32(0)).astype(f32)
        q, s = O.quant_rows(h)
        pmax = np.stack([np.abs(h[:, 512 * t:512 * (t + 1)]).max(1) for t in range(N // 512)])
        return dict(pmax=pmax.astype(f32), out8=q, os=s)
    return memo(("exp", M, N, K, epi, key), make)


def c_table(M, tab):
    from qtx import _lib
    arr = (_lib.RowFault * M)()
    for k, f in tab.items():
        for name, v in f.items():
            setattr(arr[k], name, v)
    return arr


def faults_rc(tab, layer=LAYER, gemm=GEMM, **kw):
    from qtx._lib import RowGemm
    a = RowGemm()
    for k, v in kw.items():
        setattr(a, k, v.data_ptr() if hasattr(v, "data_ptr") else v)
    return lib().qtx_linear_rows_faults(C.byref(a), c_table(kw["M"], tab) if tab is not None else None,
                                        layer, gemm, S0)


def run(gb, M, N, K, epi, tab):
    """The launch(es) on guarded outputs; returns the outputs as numpy, by name."""
    r = inputs(M, N, K)
    base = dict(A=gb.dev(r["qx"]), sa=gb.dev(r["sx"]), W=gb.dev(r["qw"]), sw=gb.dev(r["sw"]),
                bias=gb.dev(r["b"]), M=M, N=N, K=K, kp=0)
    if epi == 0:
        T = N // 512
        out = dict(out8=gb.new((T, M, 512), np.int8, "out8"), os=gb.new((T, M), f32, "os"))
        assert_ok(faults_rc(tab, epi=0, ldo8=512, o8_ts=M * 512, os_ts=M, **out, **base), "epi 0")
    elif epi == 1:
        xd = gb.init(r["res"], "xout")
        out = dict(xout=xd, lnq=gb.new((M, 512), np.int8, "lnq"), lns=gb.new((M,), f32, "lns"))
        assert_ok(faults_rc(tab, epi=1, res=xd, ln_a=gb.dev(r["la"]), ln_b=gb.dev(r["lb"]), **out,
                            **base), "epi 1")
    else:                                 # FFN1's two passes, the same table in both
        pmax = gb.new((N // 512, M), f32, "pmax")
        assert_ok(faults_rc(tab, epi=2, pmax_out=pmax, **base), "epi 2")
        out = dict(out8=gb.new((M, N), np.int8, "out8"), os=gb.new((M,), f32, "os"))
        assert_ok(faults_rc(tab, epi=3, pmax_in=pmax, pmax_n=N // 512, ldo8=N, **out, **base), "epi 3")
        out["pmax"] = pmax
    gb.check()                            # only the documented outputs were written
    return {k: np_(v) for k, v in out.items()}


def assert_same(got, want):
    assert sorted(got) == sorted(want)
    for k in want:
        a, b = got[k], want[k]
        if a.dtype == np.float32:
            a, b = a.view(np.uint32), b.view(np.uint32)
        np.testing.assert_array_equal(a, b, err_msg=k)


def changed_rows(a, b):
    """The token rows on which any output differs."""
    rows = set()
    for k in a:
        d = a[k].view(np.uint32) != b[k].view(np.uint32) if a[k].dtype == np.float32 else a[k] != b[k]
        m_axis = 1 if d.ndim == 3 or (d.ndim == 2 and k in ("os", "pmax")) else 0
        rows |= set(np.flatnonzero(d.any(tuple(x for x in range(d.ndim) if x != m_axis))))
    return rows


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("N,K,epi", SHAPES, ids=lambda v: str(v))
def test_matches_the_restatement(torch, M, N, K, epi):
    gb = Guards(torch, POISONS[0])
    tab = table(M, N, K)
    want = expect(M, N, K, epi, tab, "tab")
    base = expect(M, N, K, epi, {}, "none")
    # the table is not vacuous: exactly rows with an entry for this launch may change, and the
    # INPUT on row 0 does change its row
    mine = {k for k, f in tab.items() if f["layer"] == LAYER and f["gemm"] == GEMM}
    ch = changed_rows(want, base)
    assert 0 in ch and ch <= mine and len(ch) >= 3, (sorted(ch), sorted(mine))
    assert_same(run(gb, M, N, K, epi, tab), want)


@pytest.mark.parametrize("M,N,K,epi", [(129, 1536, 512, 0), (128, 512, 512, 1), (5, 2048, 512, 23)])
def test_null_and_foreign_tables_are_the_plain_gemm(torch, M, N, K, epi):
    """A null table, and a table whose entries all name other launches: qtx_linear_rows' results."""
    base = expect(M, N, K, epi, {}, "none")
    assert_same(run(Guards(torch, POISONS[1]), M, N, K, epi, None), base)
    foreign = {k: dict(f, layer=LAYER + 1) for k, f in table(M, N, K).items()}
    assert_same(run(Guards(torch, POISONS[1]), M, N, K, epi, foreign), base)


def test_minimum_alignment(torch):
    """Every device pointer at 16 (mod 256)."""
    M, N, K, epi = 129, 1536, 512, 0
    tab = table(M, N, K)
    assert_same(run(Guards(torch, POISONS[0], skew=16), M, N, K, epi, tab),
                expect(M, N, K, epi, tab, "tab"))


def test_refusals(torch):
    """Refused before any launch, the table row named; the outputs stay poisoned."""
    M, N, K = 5, 512, 512
    r = inputs(M, N, K)
    gb = Guards(torch, POISONS[0])
    base = dict(A=gb.dev(r["qx"]), sa=gb.dev(r["sx"]), W=gb.dev(r["qw"]), sw=gb.dev(r["sw"]),
                bias=gb.dev(r["b"]), M=M, N=N, K=K)
    out8, os_ = gb.new((1, M, 512), np.int8, "out8"), gb.new((1, M), f32, "os")

    def rc(tab, kp=0):
        code = faults_rc(tab, epi=0, ldo8=512, o8_ts=M * 512, os_ts=M, out8=out8, os=os_, kp=kp, **base)
        gb.check()
        if code != OK:
            gb.assert_poison(out8, "out8")
            gb.assert_poison(os_, "os")
        return code, lib().qtx_last_error().decode()

    for row, bad in [(1, E(INPUT, bit=7, col=K, lo=0, hi=N)), (2, E(INPUT, bit=8, col=0, lo=0, hi=N)),
                     (3, E(INPUT, bit=0, col=0, lo=8, hi=N + 1)), (4, E(WEIGHT, bit=0, col=0, wrow=N)),
                     (0, E(OUTPUT, col=N, value=1.0)), (2, E(4)),
                     (1, E(INPUT, layer=LAYER + 1, bit=7, col=-1, lo=0, hi=N))]:   # any launch's
        code, msg = rc({row: bad})
        assert code == E_INVALID and f"row {row}" in msg, (row, bad, code, msg)
    assert rc(table(M, N, K), kp=1)[0] == E_UNSUPPORTED
    # the boundaries are accepted
    assert rc({4: E(INPUT, bit=7, col=K - 1, lo=N - 1, hi=N)})[0] == OK
    assert rc({0: E(WEIGHT, bit=7, col=K - 1, wrow=N - 1), 4: E(OUTPUT, col=N - 1, value=2.0)})[0] == OK

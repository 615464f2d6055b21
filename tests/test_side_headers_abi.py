"""The accounting of include/qtx_wide_vocab.h and include/qtx_beam_long.h: what tests/test_abi.py
and tests/test_gpu_min_align.py pin for include/qtx.h and tests/test_enctrials_abi.py for
include/qtx_enctrials.h.  Every function a side header declares is exported by the library and
sits in that header's ctypes table of qtx/_lib.py (and nothing else does); every one with a
pointer parameter is named in COVERED beside the test of this module that calls it with every
device pointer at 16 (mod 256) — the least alignment include/qtx.h accepts, which the side
headers take over with its conventions — or in EXEMPT with a reason.

The four GPU cases are their home tests' (tests/test_gpu_wide_vocab.py, tests/test_gpu_beam_long.py)
at their smallest shapes, with the same oracle expressions; inputs are tests/guarded.py's skewed()
copies, everything written sits in guarded buffers at the same residue."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch as _torch  # noqa: F401  (before the CPU tests load the library: a process that loads
#                                     libqtx.so first ends up with two HIP runtimes, and the GPU
#                                     tests of this module, run on its own, then find no device)

from oracle import qtx_oracle as O
from qtx import _build, _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from guarded import guarded, skewed  # noqa: E402
from test_gpu_min_align import SKEW, torch  # noqa: E402,F401
from test_gpu_wide_vocab import tail_models  # noqa: E402,F401

f32 = np.float32
# header -> its ctypes table in qtx/_lib.py
HEADERS = {"qtx_wide_vocab.h": "SIGNATURES_WIDE_VOCAB", "qtx_beam_long.h": "SIGNATURES_BEAM_LONG"}
# entry -> the test of this module that calls it at 16 (mod 256)
COVERED = {
    "qtx_decode_tok_wide": "test_tok_wide",
    "qtx_decode_top2_wide": "test_top2_wide",
    "qtx_decode_attention_beam": "test_attention_beam",
    "qtx_beam_ancestry": "test_beam_ancestry",
}
EXEMPT = {}     # entry -> why no alignment case can say anything about it


def declarations(header):
    """name -> parameter text of every function the header declares (comments removed)."""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(_build.REPO, "include", header)).read(), flags=re.S)
    return {n: " ".join(p.split()) for n, p in re.findall(r"\b(qtx_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)}


# =====================================================================================
# the headers' functions, their tables and who covers them (CPU)
# =====================================================================================
@pytest.mark.parametrize("header", sorted(HEADERS))
def test_header_symbols_exported_and_in_the_table(header):
    decl = declarations(header)
    names = _lib.header_symbols(os.path.join(_build.REPO, "include", header))
    assert len(names) == 2 and names == sorted(decl)
    L = ctypes.CDLL(_build.build())
    assert not [n for n in names if not hasattr(L, n)]
    table = getattr(_lib, HEADERS[header])
    assert sorted(table) == names
    others = [_lib.SIGNATURES, _lib.SIGNATURES_ENCTRIALS] + [getattr(_lib, t) for h, t in HEADERS.items()
                                                            if h != header]
    for other in others:
        assert not set(table) & set(other)
    assert set(_lib.header_symbols()) == set(_lib.SIGNATURES)      # qtx.h keeps its own set
    for n in names:     # lib() applies the table; one ctypes argument per declared parameter
        fn = getattr(_lib.lib(), n)
        assert fn.argtypes is not None and len(fn.argtypes) == len(table[n][1]) == decl[n].count(",") + 1
        for ct, param in zip(table[n][1], decl[n].split(",")):
            assert (ct is ctypes.c_void_p) == ("*" in param), (n, param)


def test_every_pointer_entry_is_accounted_for():
    with_ptr = sorted(n for h in HEADERS for n, params in declarations(h).items() if "*" in params)
    assert len(with_ptr) == 4
    assert with_ptr == sorted(set(COVERED) | set(EXEMPT))
    assert not set(COVERED) & set(EXEMPT)
    assert all(callable(globals().get(t)) for t in COVERED.values())
    assert all(isinstance(r, str) and r for r in EXEMPT.values())


# =====================================================================================
# the four entries with every device pointer at 16 (mod 256) (GPU)
# =====================================================================================
pytest_gpu = pytest.mark.gpu      # (not a module-wide pytestmark: the tests above run on the CPU)


class At16:
    """The device buffers of one call, all at 16 (mod 256): inputs (skewed) and guarded in/out
    buffers; P() hands out their addresses and records them."""

    def __init__(self, torch):
        self.torch, self.checks, self.keep, self.given = torch, [], [], []

    def dev(self, a):
        t = skewed(self.torch, a, SKEW)
        self.keep.append(t)
        return t

    def new(self, a, name):
        """A guarded buffer holding `a`."""
        a = np.ascontiguousarray(a)
        t, c = guarded(self.torch, a.shape, getattr(self.torch, str(a.dtype)), 0x5A, name=name, skew=SKEW)
        t.copy_(self.torch.from_numpy(a))
        self.checks.append(c)
        return t

    def P(self, t):
        assert t.data_ptr() % 256 == SKEW
        self.given.append(t.data_ptr())
        return ctypes.c_void_p(t.data_ptr())

    def check(self, n_pointers):
        try:
            self.torch.cuda.synchronize()
        except RuntimeError as e:       # a device fault: nothing more may run on this GPU
            pytest.exit(f"GPU error at synchronize, stopping the session: {e}", returncode=3)
        assert len(self.given) == n_pointers
        for c in self.checks:
            c()


WIDE_V = 8193                       # one element past a 4096-element chunk
# of rows_of(8193): the maximum twice (a near-tie: the streamed path), a winner two above the
# runner-up, the logp collision, a NaN row, two random rows
WIDE_ROWS = [5, 7, 8, 10, 13, 14]


def _wide_tail(torch, tail_models, oracle_model, kind):
    """test_gpu_wide_vocab.py::test_wide_tail on six rows: ids, top ids, logp bits, x_next and
    the step counter == the oracle; the other columns and the guard bands stay."""
    import test_gpu_wide_vocab as W
    S0 = ctypes.c_void_p(0)
    gm, lut = tail_models(WIDE_V)
    lg, want_id, want_i, want_v = (np.ascontiguousarray(a[WIDE_ROWS]) for a in W.rows_of(WIDE_V))
    M, ids_bs, s = len(lg), 7, 3
    top = np.sort(lg[:3], -1)
    assert top[0, -1] == top[0, -2] and top[1, -1] - top[1, -2] > 0.5 and 0 < top[2, -1] - top[2, -2] < 4e-6
    assert want_v[2, 0] == want_v[2, 1] and np.isnan(lg[3]).any() and np.isnan(want_v[3]).all()
    assert np.array_equal(want_i[:, 0], want_id)
    b = At16(torch)
    ids0 = np.arange(M * ids_bs, dtype=np.int64).reshape(M, ids_bs) - 50
    rng = np.random.default_rng(M)
    before = {"top_ids": rng.integers(-9, 0, (M, ids_bs - 1, 2)).astype(np.int64),
              "top_logp": rng.standard_normal((M, ids_bs - 1, 2)).astype(f32)}
    ids, step = b.new(ids0, "ids"), b.new(np.array([s, 0], np.int32), "step")
    top_ids, top_logp = b.new(before["top_ids"], "top_ids"), b.new(before["top_logp"], "top_logp")
    x_next = b.new(np.full((M, 512), np.nan, f32), "x_next")
    lgd = b.dev(lg)
    if kind == "tok":
        rec = b.dev(W.strip_records(lg))
        W.call("qtx_decode_tok_wide", gm.handle, b.P(lgd), b.P(rec), M, b.P(ids), ids_bs, b.P(step),
               b.P(x_next), S0)
    else:
        W.call("qtx_decode_top2_wide", gm.handle, b.P(lgd), M, b.P(ids), ids_bs, b.P(top_ids),
               b.P(top_logp), b.P(step), b.P(x_next), S0)
    b.check(5 if kind == "tok" else 6)
    ids1 = ids0.copy()
    ids1[:, s + 1] = want_id
    np.testing.assert_array_equal(ids.cpu().numpy(), ids1)
    np.testing.assert_array_equal(step.cpu().numpy(), [s + 1, 0])
    np.testing.assert_array_equal(x_next.cpu().numpy(),
                                  oracle_model.embed(want_id[:, None], lut, pos0=s + 1)[:, 0])
    if kind == "top2":
        before["top_ids"][:, s], before["top_logp"][:, s] = want_i, want_v
    np.testing.assert_array_equal(top_ids.cpu().numpy(), before["top_ids"])
    np.testing.assert_array_equal(top_logp.cpu().numpy().view(np.uint32), before["top_logp"].view(np.uint32))


@pytest_gpu
def test_tok_wide(torch, tail_models, oracle_model):
    _wide_tail(torch, tail_models, oracle_model, "tok")


@pytest_gpu
def test_top2_wide(torch, tail_models, oracle_model):
    _wide_tail(torch, tail_models, oracle_model, "top2")


@pytest_gpu
def test_attention_beam(torch):
    """test_gpu_beam_long.py::test_attention_op at kv_bs = 140, step 129, 2 sentences of 3 beam
    rows, the "cycle" table: every 4-key value group is gathered from three slots."""
    import test_gpu_beam_long as T
    from test_gpu_fused import head_max, vgroup4
    S0 = ctypes.c_void_p(0)
    K, step, kv_bs = 3, 129, 140
    R, n = T.NS * K, step + 1
    rng = np.random.default_rng(1000 * K + step)
    y = rng.standard_normal((R, 1536)).astype(f32)
    kc, vc = (rng.integers(-127, 128, (R, kv_bs, 512)).astype(np.int8) for _ in range(2))
    skc, svc = (rng.uniform(0.002, 0.03, (R, kv_bs)).astype(f32) for _ in range(2))
    anc = T.table("cycle", K, kv_bs)
    anc[:K, 0] = K
    anc[:, step:] = (anc[:, step:] + 1) % K
    assert all(len(set(anc[r, 4 * g:4 * g + 4].tolist())) >= 2 for r in range(R) for g in range(n // 4))
    rows = (np.arange(R)[:, None] // K) * K + np.minimum(anc, K - 1)     # [R, kv_bs] cache rows
    j = np.arange(kv_bs)[None, :]
    gk, gv, gsk, gsv = kc[rows, j], vc[rows, j], skc[rows, j], svc[rows, j]
    qq, sq = O.quant_rows(y[:, :512])
    kc[:, step], skc[:, step] = gk[:, step], gsk[:, step] = O.quant_rows(y[:, 512:1024])
    vc[:, step], svc[:, step] = gv[:, step], gsv[:, step] = O.quant_rows(y[:, 1024:])
    ctx, _ = O.attention(qq[:, None], sq[:, None], gk[:, :n], gsk[:, :n], gv[:, :n], gsv[:, :n],
                         np.ones((R, 1, n), np.uint8), dec=True)
    stale = rng.integers(-127, 128, (2, R, 512)).astype(np.int8)         # row `step` before the call
    b = At16(torch)
    kcd, vcd, skd, svd = (b.new(a, nm) for a, nm in ((kc, "kc"), (vgroup4(vc), "vc"), (skc, "skc"),
                                                     (svc, "svc")))
    kcd[:, step] = torch.from_numpy(stale[0]).cuda()
    vcd[:, step >> 2, :, step & 3] = torch.from_numpy(stale[1]).cuda()
    skd[:, step], svd[:, step] = 7.0, 9.0
    ctxd, pm = b.new(np.full((R, 512), np.nan, f32), "ctx"), b.new(np.full((8, R), np.nan, f32), "pmax")
    T.call("qtx_decode_attention_beam", b.P(b.dev(y)), 1536, b.P(kcd), b.P(vcd), b.P(skd), b.P(svd),
           kv_bs, b.P(b.dev(np.array([step], np.int32))), b.P(b.dev(anc)), K, R, b.P(ctxd), b.P(pm), S0)
    b.check(9)
    for got, want in ((ctxd, ctx[:, 0]), (pm, head_max(ctx[:, 0])), (kcd, kc), (vcd, vgroup4(vc)),
                      (skd, skc), (svd, svc)):
        np.testing.assert_array_equal(got.cpu().numpy(), want)


@pytest_gpu
def test_beam_ancestry(torch):
    """test_gpu_beam_long.py::test_ancestry_op at 2 sentences of 3 beam rows, max_len 140, n =
    130: the prefix == a numpy gather by parent; the bytes past it, the guards and the step
    words stay."""
    import test_gpu_beam_long as T
    S0 = ctypes.c_void_p(0)
    parents, n, ML = (2, 0, 0), 130, 140
    K = len(parents)
    par = np.array([parents, np.roll(parents, 1)], np.int32).reshape(-1)
    anc = np.random.default_rng(n + K).integers(0, K, (T.NS * K, ML)).astype(np.uint8)
    b = At16(torch)
    ancd = b.new(anc, "anc")
    step = b.new(np.array([n, 0, 0, 0], np.int32), "step")
    T.call("qtx_beam_ancestry", b.P(ancd), T.NS, K, ML, b.P(step), b.P(b.dev(par)), S0)
    b.check(3)
    want = anc.copy()
    want[:, :n] = anc[(np.arange(T.NS)[:, None] * K + par.reshape(T.NS, K)).reshape(-1), :n]
    assert (want != anc).any()
    np.testing.assert_array_equal(ancd.cpu().numpy(), want)
    np.testing.assert_array_equal(step.cpu().numpy(), [n, 0, 0, 0])

"""The long-target regime on the GPU: 129 to 512 decoder positions, against the oracle — bit for
bit, every comparison assert_array_equal.

Every decoder-side entry point accepts up to 512 target positions (and never more than the
model's positional table).  Above 128 the library runs what no other test runs: the unfused
decode step whose self-attention (k_attention) reads its key count from the device counter,
full-prefix passes through k_attention with a [T, T] mask and the decoder's PV order over more
than one 128-row tile, the beam reorder of ungrouped V caches, and the attention fault rows past
128 keys.  The rule of tests/test_gpu_model_configs.py — nothing accepted at the door may fail
or be wrong later — is enforced here for the target length.

Models, inputs and the memoised oracle results: tests/long_target.py (L = 140: keys to 139, two
full 64-lane rounds plus a ragged 11).  That the oracle's results are not degenerate (distinct
tokens past 128, faults that change tokens, a beam that reorders past 128) is asserted on the
CPU by tests/test_long_target_ref.py.  The defects each test would catch are named in its
docstring.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from oracle import qtx_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import long_target as LT  # noqa: E402
from guarded import POISONS, guarded  # noqa: E402
from test_gpu_beam import assert_same, gpu_beam, reorder_case  # noqa: E402
from test_gpu_dfault_cached import check_scored  # noqa: E402
from test_gpu_kvfault import check as check_kvfault  # noqa: E402
from test_gpu_scored import gpu_scored  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
S0 = C.c_void_p(0)
OK, E_INVALID, E_WORKSPACE, E_UNSUPPORTED = 0, 1, 3, 4
B, S, L = LT.B, LT.S, LT.L
IDS = [LT.cfg_id(c) for c in LT.CONFIGS]
_KEEP = []   # device tensors must outlive the C call that receives their raw pointers


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def models(torch):
    """get((d_ff, weight_bits), pe_rows = 192) -> (QtxModel, OracleModel), built once."""
    from qtx.model import QtxModel
    cache = {}

    def get(c, pe_rows=LT.PE_ROWS):
        if (c, pe_rows) not in cache:
            cfg, sd, om = LT.state(*c, pe_rows)
            cache[(c, pe_rows)] = (QtxModel(sd, cfg), om)
        return cache[(c, pe_rows)]
    yield get
    cache.clear()


@pytest.fixture(autouse=True)
def _release():
    yield
    _KEEP.clear()


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else S0


def dev(torch, a):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    _KEEP.append(t)
    return t


def u8(torch, m):
    return dev(torch, np.asarray(m).reshape(m.shape[0], m.shape[-1]).astype(np.uint8))


def lib():
    from qtx import _lib
    return _lib.lib()


def call(name, *args):
    from qtx import _lib
    _lib.call(name, *args)


# =====================================================================================
# a. the attention op at and around the limits
# =====================================================================================
ATT_B, ATT_SQ = 2, 5


def last_round_key(Sk):
    """A key index in the last 64-lane round of Sk keys (>= 448 for Sk = 511 and 512)."""
    j0 = 64 * ((Sk - 1) // 64)
    return Sk - 3 if Sk - 3 >= j0 else Sk - 1


def attention_case(Sk, form):
    """q, k, v codes and scales of [2, 5 | Sk, 512] and a mask.
      key   one key mask per sentence (m_is = 0): sentence 0 loses its last third, sentence 1
            every seventh key
      full  a [B, Sq, Sk] mask: sentence 0 causal with the offset Sk - Sq (query i sees the keys
            0 .. Sk - Sq + i), sentence 1 seeded rows, of which row 1 is fully masked and row 2
            keeps one key only, in the last lane round"""
    def make():
        rng = np.random.default_rng(1000 * Sk + len(form))
        q = rng.integers(-127, 128, (ATT_B, ATT_SQ, 512)).astype(np.int8)
        k = rng.integers(-127, 128, (ATT_B, Sk, 512)).astype(np.int8)
        v = rng.integers(-127, 128, (ATT_B, Sk, 512)).astype(np.int8)
        sq, sk, sv = (rng.uniform(0.002, 0.03, (ATT_B, n)).astype(f32) for n in (ATT_SQ, Sk, Sk))
        mask = np.ones((ATT_B, ATT_SQ, Sk), np.uint8)
        if form == "key":
            km = np.ones((ATT_B, Sk), np.uint8)
            km[0, Sk - Sk // 3:] = 0
            km[1, 1::7] = 0
            mask[:] = km[:, None, :]
            mdev, m_bs, m_is = km, Sk, 0
        else:
            mask[0] = np.tril(np.ones((ATT_SQ, Sk), np.uint8), k=Sk - ATT_SQ)
            mask[1] = rng.integers(0, 2, (ATT_SQ, Sk))
            mask[1, 1] = 0
            mask[1, 2] = 0
            mask[1, 2, last_round_key(Sk)] = 1
            mdev, m_bs, m_is = mask, ATT_SQ * Sk, Sk
        res = {}
        for dec in (0, 1):
            res[dec] = O.attention(q, sq, k, sk, v, sv, mask, 8, dec=bool(dec))
        acc = np.einsum("bhid,bhjd->bhij", O.split_heads(q, 8).astype(np.int64),
                        O.split_heads(k, 8).astype(np.int64)).astype(f32)
        return dict(q=q, k=k, v=v, sq=sq, sk=sk, sv=sv, mask=mask, mdev=mdev, m_bs=m_bs,
                    m_is=m_is, res=res, acc=acc)
    return LT.memo(("attn", Sk, form), make)


@pytest.mark.parametrize("dec", [0, 1])
@pytest.mark.parametrize("form", ["key", "full"])
@pytest.mark.parametrize("Sk", [129, 192, 511, 512])
def test_attention_op(torch, Sk, form, dec):
    """qtx_attention_i8 (k_attention: every Sk here is past k_attn_mfma's 128 keys) and
    qtx_attention_trace (ctx, qk_acc, p_codes) == oracle attention at Sq = 5 and Sk = 129 (one
    key in the third lane round), 192, 511 and the cap 512.  Fails under a key count clamped to
    128, a softmax that drops lane rounds past the second (the row whose only kept key lies in
    the last round would turn uniform; the causal rows lose probability mass), a mask read
    with the wrong row stride (the fully masked row and the one-key row sit between seeded
    rows), and a PV chain that stops short of Sk."""
    c = attention_case(Sk, form)
    if form == "full":
        j = last_round_key(Sk)
        assert c["mask"][1, 2].sum() == 1 and c["mask"][1, 2, j] and j >= 64 * ((Sk - 1) // 64)
        assert Sk < 511 or j >= 448
        assert not c["mask"][1, 1].any()
        qp = c["res"][dec][1]
        assert (qp[1, :, 2, j] == 127).all() and qp[1, :, 2].sum() == 8 * 127
    co, qp = c["res"][dec]
    args = [P(dev(torch, c[n])) for n in ("q", "sq", "k", "sk", "v", "sv")]
    args += [P(dev(torch, c["mdev"])), c["m_bs"], c["m_is"], ATT_B, 8, ATT_SQ, Sk]
    ctx, chk = guarded(torch, (ATT_B, ATT_SQ, 512), torch.float32, POISONS[dec], name="ctx")
    call("qtx_attention_i8", *args, P(ctx), dec, S0)
    torch.cuda.synchronize()
    chk()
    np.testing.assert_array_equal(ctx.cpu().numpy(), co)
    ctx2, chk2 = guarded(torch, (ATT_B, ATT_SQ, 512), torch.float32, POISONS[dec], name="ctx")
    qk, cq = guarded(torch, (ATT_B, 8, ATT_SQ, Sk), torch.float32, POISONS[dec], name="qk_acc")
    pc, cp = guarded(torch, (ATT_B, 8, ATT_SQ, Sk), torch.float32, POISONS[dec], name="p_codes")
    call("qtx_attention_trace", *args, P(ctx2), P(qk), P(pc), dec, S0)
    torch.cuda.synchronize()
    for ch in (chk2, cq, cp):
        ch()
    np.testing.assert_array_equal(qk.cpu().numpy(), c["acc"])
    np.testing.assert_array_equal(pc.cpu().numpy(), qp.astype(f32))
    np.testing.assert_array_equal(ctx2.cpu().numpy(), co)


@pytest.mark.parametrize("entry", ["qtx_attention_i8", "qtx_attention_trace"])
def test_attention_op_refuses_513_keys(torch, entry):
    """Sk = 513 is one above the kernels' LDS staging: an error before anything is launched,
    the poisoned ctx untouched."""
    Sk = 513
    q = torch.zeros((ATT_B, ATT_SQ, 512), dtype=torch.int8, device="cuda")
    k = torch.zeros((ATT_B, Sk, 512), dtype=torch.int8, device="cuda")
    sq = torch.ones((ATT_B, ATT_SQ), dtype=torch.float32, device="cuda")
    sk = torch.ones((ATT_B, Sk), dtype=torch.float32, device="cuda")
    ctx, chk = guarded(torch, (ATT_B, ATT_SQ, 512), torch.float32, 0x5A, name="ctx")
    args = [P(q), P(sq), P(k), P(sk), P(k), P(sk), S0, 0, 0, ATT_B, 8, ATT_SQ, Sk, P(ctx)]
    if entry == "qtx_attention_trace":
        args += [S0, S0]
    rc = getattr(lib(), entry)(*args, 1, S0)
    torch.cuda.synchronize()
    assert rc == E_UNSUPPORTED, rc
    chk()
    assert bool((ctx.view(torch.uint8) == 0x5A).all())


# =====================================================================================
# b. qtx_decoder_forward == om.decode
# =====================================================================================
def gpu_full_pass(torch, gm, p):
    tm = p["tgt_mask"]
    tmd = dev(torch, tm[0] if tm.shape[0] == 1 else tm)
    return gm.decode(dev(torch, p["y"]), dev(torch, p["memory"]), u8(torch, p["src_mask"]),
                     tmd).cpu().numpy()


@pytest.mark.parametrize("c", LT.CONFIGS, ids=IDS)
def test_decoder_forward_causal(torch, models, c):
    """(B, T, S) = (2, 139, 9) under the shared causal [T, T] mask: 278 rows, three 128-row
    tiles on every GEMM chain, and k_attention with m_is = T.  Fails under a key count clamped
    to 128 and a softmax that drops lane rounds past the second (the positions 128 .. 138
    differ), and under a [T, T] mask read with the wrong row stride."""
    gm, _ = models(c)
    p = LT.full_pass(c)
    assert p["y"].shape == (B, LT.T_FULL, 512) and p["tgt_mask"].shape == (1, LT.T_FULL, LT.T_FULL)
    np.testing.assert_array_equal(gpu_full_pass(torch, gm, p), p["out"])


@pytest.mark.parametrize("c", [(512, 8), (256, 8)], ids=["dff512_w8", "dff256_w8"])
def test_decoder_forward_batched_mask(torch, models, c):
    """tgt_mask_batched = 1: a [B, T, T] mask, causal AND a pad pattern with holes below and
    above position 128, one query row fully masked.  The two sentences' masks differ, so a
    wrong batch or row stride of the mask shows."""
    gm, _ = models(c)
    p = LT.full_pass(c, "padded")
    assert p["tgt_mask"].shape == (B, LT.T_FULL, LT.T_FULL)
    np.testing.assert_array_equal(gpu_full_pass(torch, gm, p), p["out"])


@pytest.mark.parametrize("c", [(1024, 8), (256, 8)], ids=["dff1024_w8", "dff256_w8"])
def test_decoder_forward_long_source(torch, models, c):
    """(2, 130, 132): self- and cross-attention both past 128 keys with Sq > 1 (the second
    sentence's memory masked from 70 on)."""
    gm, _ = models(c)
    p = LT.full_pass(c, "long")
    assert p["y"].shape == (B, LT.LONG_T, 512) and p["memory"].shape == (B, LT.LONG_S, 512)
    np.testing.assert_array_equal(gpu_full_pass(torch, gm, p), p["out"])


def test_decoder_forward_cap(torch, models):
    """(1, 512, 9): the cap, on the model with a 512-row positional table — four full 128-row
    tiles and all eight lane rounds of k_attention."""
    c = (512, 8)
    gm, _ = models(c, LT.CAP_ROWS)
    p = LT.full_pass(c, "cap")
    assert p["y"].shape == (1, LT.CAP_ROWS, 512)
    np.testing.assert_array_equal(gpu_full_pass(torch, gm, p), p["out"])


@pytest.mark.parametrize("rows,T", [(LT.CAP_ROWS, 513), (LT.PE_ROWS, LT.PE_ROWS + 1)],
                         ids=["T513", "T_table_plus_1"])
def test_decoder_forward_refusals(torch, models, rows, T):
    """T = 513, and T one above the positional table: QTX_E_INVALID before anything is
    launched, out and the workspace untouched; the table's last row itself is accepted."""
    gm, _ = models((512, 8), rows)
    L_ = lib()
    need = int(L_.qtx_decoder_workspace_size(gm.handle, 1, rows, S))
    assert need > 0
    y = torch.zeros((1, T, 512), dtype=torch.float32, device="cuda")
    mem = torch.zeros((1, S, 512), dtype=torch.float32, device="cuda")
    sm = torch.ones((1, S), dtype=torch.uint8, device="cuda")
    tm = torch.ones((T, T), dtype=torch.uint8, device="cuda").tril_()
    out, co = guarded(torch, (1, T, 512), torch.float32, 0x5A, name="out")
    ws, cw = guarded(torch, (2 * need,), torch.uint8, 0x5A, name="workspace")
    rc = L_.qtx_decoder_forward(gm.handle, P(y), P(mem), P(sm), P(tm), 0, 1, T, S, P(out), P(ws),
                                2 * need, S0)
    torch.cuda.synchronize()
    assert rc == E_INVALID, rc
    co()
    cw()
    assert bool((out.view(torch.uint8) == 0x5A).all()) and bool((ws == 0x5A).all())
    rc = L_.qtx_decoder_forward(gm.handle, P(y), P(mem), P(sm), P(tm), 0, 1, T - 1, S, P(out),
                                P(ws), 2 * need, S0)
    gm.check()
    assert rc == OK
    co()
    cw()


# =====================================================================================
# c. greedy and scored decode, L = 140
# =====================================================================================
@pytest.mark.parametrize("c", LT.CONFIGS, ids=IDS)
def test_greedy_and_scored_decode(torch, models, c):
    """ids, top_ids and top_logp of the 139 unfused steps == the oracle's scored decode, and
    the plain decode's ids == the scored ones.  The self-attention of the steps 128 .. 138
    reads 129 .. 139 keys by the device counter: a key count clamped to 128 or a cache row
    written modulo 128 (position 128 over position 0) changes the tokens there — the oracle's
    decode holds at least three distinct tokens at 129 and up (tests/test_long_target_ref.py).
    A wrong (max_len - 1) stride of top_ids / top_logp shows in sentence 1."""
    from qtx.decode import greedy_decode
    gm, _ = models(c)
    src, m = LT.inputs()
    oy, oi, ov = LT.scored(c)
    gy, gi, gv = gpu_scored(gm, src, m, L)
    np.testing.assert_array_equal(gy, oy)
    np.testing.assert_array_equal(gi, oi)
    np.testing.assert_array_equal(gv, ov)
    np.testing.assert_array_equal(greedy_decode(gm, src, m, L, 0), gy)


@pytest.mark.parametrize("c", LT.CONFIGS, ids=IDS)
def test_greedy_workspace_and_extents(torch, models, c):
    """The workspace carving for max_len > 128: the exact qtx_greedy*_workspace_size succeeds
    between guard bands (nothing written outside ids, top_ids, top_logp or the workspace), one
    byte less is QTX_E_WORKSPACE before anything is written."""
    gm, _ = models(c)
    L_ = lib()
    src, m = LT.inputs()
    oy, oi, ov = LT.scored(c)
    srcd = dev(torch, src)
    md = u8(torch, m)
    for scored in (True, False):
        size = L_.qtx_greedy_scored_workspace_size if scored else L_.qtx_greedy_workspace_size
        need = int(size(gm.handle, B, S, L))
        assert need > 0
        ids, c0 = guarded(torch, (B, L), torch.int64, 0x5A, name="ids")
        ti, c1 = guarded(torch, (B, L - 1, 2), torch.int64, 0x5A, name="top_ids")
        tl, c2 = guarded(torch, (B, L - 1, 2), torch.float32, 0x5A, name="top_logp")
        ws, c3 = guarded(torch, (need,), torch.uint8, 0x5A, name="workspace")
        head = (gm.handle, P(srcd), P(md), B, S, L, 0, P(ids))
        if scored:
            run = lambda n: L_.qtx_greedy_decode_scored(*head, P(ti), P(tl), P(ws), n, None, S0)
        else:
            run = lambda n: L_.qtx_greedy_decode(*head, P(ws), n, S0)
        assert run(need - 1) == E_WORKSPACE
        torch.cuda.synchronize()
        for t in (ids, ti, tl, ws):
            assert bool((t.view(torch.uint8) == 0x5A).all())
        assert run(need) == OK
        gm.check()
        for ch in (c0, c1, c2, c3):
            ch()
        np.testing.assert_array_equal(ids.cpu().numpy(), oy)
        if scored:
            np.testing.assert_array_equal(ti.cpu().numpy(), oi)
            np.testing.assert_array_equal(tl.cpu().numpy(), ov)
        else:
            assert bool((ti.view(torch.uint8) == 0x5A).all()) and bool((tl.view(torch.uint8) == 0x5A).all())


# =====================================================================================
# d. causal invariance on the GPU
# =====================================================================================
@pytest.mark.parametrize("c", LT.CONFIGS, ids=IDS)
def test_score_targets_of_the_decode(torch, models, c):
    """decode.score_targets on the decoded ids (one full-prefix pass at T = 139) gives rank 0
    everywhere, tok_logp == the scored decode's top_logp[..., 0], top_ids == its top_ids, and
    all outputs == score_ref: the full pass under the [T, T] causal mask computes what the 139
    cached steps computed, bit for bit.  A key count clamped to 128 in either, or a mask row
    stride off by one, breaks the equality from position 128 on."""
    from qtx.decode import score_targets
    gm, _ = models(c)
    src, m = LT.inputs()
    gy, gi, gv = gpu_scored(gm, src, m, L)
    ts = score_targets(gm, src, m, gy, pad=-1)
    assert ts.rank.shape == (B, L - 1) and (ts.rank == 0).all()
    np.testing.assert_array_equal(ts.tok_logp, gv[..., 0])
    np.testing.assert_array_equal(ts.top_ids, gi)
    np.testing.assert_array_equal(ts.top_logp, gv)
    ref = LT.score_golden(c)
    np.testing.assert_array_equal(gy, LT.scored(c)[0])
    np.testing.assert_array_equal(ts.tok_logp, ref["tok_logp"])
    np.testing.assert_array_equal(ts.rank, ref["rank"])
    np.testing.assert_array_equal(ts.top_ids, ref["top_ids"])
    np.testing.assert_array_equal(ts.top_logp, ref["top_logp"])


def test_score_targets_pad_beyond_128(torch, models):
    """pad >= 0 with pad tokens at the positions 131 and 137 of sentence 1: the pad-aware
    [R, T, T] mask built on the device drops keys past position 128."""
    from qtx.decode import score_targets
    c = (512, 8)
    gm, _ = models(c)
    src, m = LT.inputs()
    tgt, ref = LT.score_padded(c)
    ts = score_targets(gm, src, m, tgt, pad=2)
    np.testing.assert_array_equal(ts.tok_logp, ref["tok_logp"])
    np.testing.assert_array_equal(ts.rank, ref["rank"])
    np.testing.assert_array_equal(ts.top_ids, ref["top_ids"])
    np.testing.assert_array_equal(ts.top_logp, ref["top_logp"])


# =====================================================================================
# e. the decoder-fault decode at fault_step 133
# =====================================================================================
def test_dfault_at_step_133(torch, models):
    """qtx_greedy_decode_dfault with the fault at step 133: 133 cached golden steps, the faulty
    full-prefix pass at T = 134 (a linear target; a QK WEIGHT fault on key 130; a PV INPUT fault
    at column h * Sk + 131: launch_attn_fault_rows past 128 keys), cached steps after it — and
    one resume on the same workspace.  Every trial changes the token of step 133 in the oracle
    (tests/test_long_target_ref.py).  Fails when the fault rows' key count, or the K/V rows the
    golden steps cached at positions >= 128, are wrong."""
    from qtx.decode import _record, Scores, greedy_decode_fault
    c = LT.FAULT_CFG
    gm, _ = models(c)
    src, m = LT.inputs()
    tin = LT.DF_STEP + 1
    trials = LT.dfault_trials()
    for name, f in trials.items():
        exp = LT.dfault_trial(name)
        got = greedy_decode_fault(gm, src, m, L, 0, fault=f, target_inference_number=tin,
                                  return_scores=True, kv_cache=True)
        check_scored(got, exp, tin, L)
    # one trial on a workspace of its own, then a resume with another fault at the same step
    names = sorted(trials)
    srcd, md = dev(torch, src), u8(torch, m)
    ws = gm.dfault_workspace(B, S, L)
    first = gm.greedy_dfault(srcd, md, trials[names[0]], LT.DF_STEP, max_len=L, scores=True, ws=ws)
    gm.check()
    np.testing.assert_array_equal(first[0].cpu().numpy(), LT.dfault_trial(names[0])[0])
    ys, ti, tl, ri, rl, changed = gm.greedy_dfault_resume(ws, B, S, trials[names[1]], LT.DF_STEP,
                                                          max_len=L)
    gm.check()
    exp = LT.dfault_trial(names[1])
    got = (ys.cpu().numpy(), Scores(ti.cpu().numpy(), tl.cpu().numpy(), _record(LT.DF_STEP, ri, rl)))
    check_scored(got, exp, tin, L)
    np.testing.assert_array_equal(changed != 0, exp[3][0][:, 0] != exp[3][2][:, 0])


# =====================================================================================
# f. faults of the cached decode itself
# =====================================================================================
@pytest.mark.parametrize("name", sorted(LT.kvfault_cases()))
def test_kvfault_past_128(torch, models, name):
    """qtx_greedy_decode_kvfault == tests/kvfault_ref.py: a K-projection fault at step 131 whose
    row every later step reads, a stored K code of position 129 and a stored V scale of a
    position >= 128 upset before a later step, and the step's own attention MatMuls at keys
    j >= 128.  Each changes tokens in the reference.  Fails when the upset's row b * max_len + j
    or the step's K/V row placement at dst_off >= 128 is computed modulo 128."""
    c = LT.FAULT_CFG
    gm, om = models(c)
    f, u, step = LT.kvfault_cases()[name]
    check_kvfault(gm, om, f, u, step, ("long" + LT.cfg_id(c), LT.inputs(), L))


# =====================================================================================
# g. beam
# =====================================================================================
@pytest.mark.parametrize("c", LT.BEAM_CONFIGS, ids=IDS[:2])
def test_beam_decode(torch, models, c):
    """beam = 3, max_len = 140 == beam_ref (hyp_ids, hyp_len, hyp_score bits, steps_run): the
    search reorders the ungrouped V caches at steps >= 129.  On the d_ff 1024 model the final
    hypotheses descend through rows moved at those steps (long_target.beam_late_moves), so a
    reorder that stops at 128 positions changes their tokens or scores; the d_ff 512 model's
    search keeps its best hypothesis in slot 0 throughout and pins the workspace carving for
    B * beam rows at max_len > 128, the beam tail and steps_run (the reorder itself:
    test_reorder_op_past_128)."""
    gm, _ = models(c)
    src, m = LT.inputs()
    ref = LT.beam_reference(c)
    assert ref["steps_run"] == L - 1
    assert_same(gpu_beam(gm, src, m, LT.BEAM, max_len=L), ref)


@pytest.mark.parametrize("grouped", [1, 0])
@pytest.mark.parametrize("t", [129, 137])
@pytest.mark.parametrize("parents", [(2, 0, 0), (7, 0, 0, 3, 5, 6, 1, 2)], ids=["beam3", "beam8"])
def test_reorder_op_past_128(torch, parents, t, grouped):
    """qtx_beam_reorder at max_len = 140 with 130 and 138 valid positions, both V layouts: the
    moved prefix == a numpy gather, everything behind it (and the guards) untouched."""
    reorder_case(torch, parents, t, grouped, POISONS[grouped], ML=L)

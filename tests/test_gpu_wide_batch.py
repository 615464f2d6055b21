"""Every driver of the KV-cached decode step at 33 to 200 rows, past the step's row-block
switches, against the oracle, bit for bit: ids, top-2 ids, log-probability bits, records,
hypotheses.  The per-op tests pin the switches kernel by kernel (tests/test_gpu_bounds.py,
tests/test_gpu_absmax_lanes.py); here each driver wraps the wide step in what is its own — the
scored tail, graphs that end at a fault step, an eager faulty step at M = B, the trial table, the
beam select / reorder on B * beam rows.

Batches and expectations: tests/wide_batch.py (three distinct sentences cycled over the rows,
per-sentence oracle results indexed by the cycle; tests/test_wide_batch_ref.py licenses the
expansion on the CPU).  Default model: tests/dfault_cases.py's sentences, S = 14, max_len = 8.

The row counts and the instances they reach, M the step's rows.  This was read from the code that
selects them, not observed in a kernel trace:

  csrc/qtx_decode.hip skinny_mode — M <= 4: 4-row blocks; M <= QTX_SKINNY8_MAXM (32): the d_ff
    2048 FFN2 on k_skinny8_ffn2; M >= 96 ("big"): every K = 512 GEMM on the N-split k_skinny_wide
    with 8-row blocks, the int8 K = 2048 GEMM on 16-row blocks (4-row blocks below).
  csrc/qtx_api.hip greedy_step_fused — `ffn_qkernel = ... || B >= 96`: from 96 rows on the FFN
    hidden is quantized by its own kernel (k_quant_h2048, one workgroup per row) and FFN2 is the
    int8 K = 2048 GEMM.  So skinny_mode's fp32-prologue K = 2048 row blocks (8 from 96 rows, 16
    from 192) are never reached by a decode: below 96 rows they are 4-row blocks, from 96 on FFN2
    has no fp32 prologue.  They stay pinned at op level only (qtx_skinny_linear at M = 97 / 193).
  csrc/qtx_decode.hip launch_skinny_tok — the folded tail: k_skinny_wide_tok<8> from M >= 96,
    <4> below.  launch_generator_mfma: 16-row blocks.  k_top2_embed / k_argmax_embed /
    k_beam_select: one workgroup per row / per sentence.
  csrc/qtx_rowfault.hip launch_gemm_rowfault — the kvtrials driver's per-row-fault GEMM has
    32-row tiles (the 128-row tiles are the enctrials table GEMM's, over B * S token rows);
    launch_trial_record: 64 rows per workgroup.

  33   above k_skinny8_ffn2's cap: the fp32-prologue FFN2 on 4-row skinny blocks, the ninth
       4-row block ragged (one row), a ragged third 16-row generator block.
  97   the "big" instances: 8-row k_skinny_wide and k_skinny_wide_tok<8> blocks (the 13th ragged,
       one row), k_quant_h2048 + the int8 FFN2 on 16-row blocks (the 7th ragged), the generator's
       7th block ragged; a fourth, one-row 32-row tile of the row-fault GEMM; B * S = 1358 token
       rows: 11 tiles of the enctrials table GEMM, the last ragged.
  130  (kvtrials) rows 128 and 129: a ragged fifth 32-row tile of the row-fault GEMM, a ragged
       third block of the record kernel, ragged 8- and 16-row blocks of two rows.
  193  25 8-row and 13 16-row blocks, the last of each one row.  QTX_DECODE_GROUPS=2:
       split_groups (csrc/qtx_carve.h) gives Bg = ceil(193 / 2) = 97, groups of 97 and 96 rows,
       both at the "big" switch — 96 is its first row count, all blocks full.
  99, 104, 200  beam rows B * beam: as 97 / 193 with k_beam_select and k_beam_reorder behind.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_ref as BR  # noqa: E402
import dfault_cases as D  # noqa: E402
import test_gpu_beam as GB  # noqa: E402
import test_gpu_enctrials as EN  # noqa: E402
import test_gpu_kvtrials as KV  # noqa: E402
import wide_batch as W  # noqa: E402
from guarded import POISONS, guarded  # noqa: E402

pytestmark = pytest.mark.gpu
S0 = C.c_void_p(0)
S, L = D.S, D.L
bits = W.bits


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else S0


def same3(got, want):
    """ids, top_ids, top_logp bits."""
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    np.testing.assert_array_equal(bits(got[2]), bits(want[2]))


def same_rec(r, want, step):
    """A FaultStepRecord with [B, 2] arrays against (golden ids, golden logp, faulty ids, faulty
    logp)."""
    assert r is not None and r.step == step
    np.testing.assert_array_equal(r.golden_ids, want[0])
    np.testing.assert_array_equal(bits(r.golden_logp), bits(want[1]))
    np.testing.assert_array_equal(r.faulty_ids, want[2])
    np.testing.assert_array_equal(bits(r.faulty_logp), bits(want[3]))


def golden(om, B):
    return W.golden_rows(om, *D.make_src(), B, L)


# =====================================================================================
# 1. plain and scored greedy, default model
# =====================================================================================
NO_GRAPH, NO_FOLD, GROUPS2 = {"QTX_NO_GRAPH": 1}, {"QTX_NO_TAIL_FOLD": 1}, {"QTX_DECODE_GROUPS": 2}
GREEDY = [(B, env) for B in (33, 97, 193) for env in ({}, NO_GRAPH, NO_FOLD)] + [(193, GROUPS2)]


@pytest.mark.parametrize("B,env", GREEDY, ids=lambda v: str(v) if isinstance(v, int) else
                         "-".join(k[4:].lower() for k in v) or "default")
def test_greedy(torch, gpu_model, oracle_model, knob_env, B, env):
    """The default model's plain decode (the folded tail on a 4444-word vocabulary: <4> at 33
    rows, <8> at 97 and 193; QTX_NO_TAIL_FOLD: k_argmax_embed on every step) and scored decode
    (k_top2_embed, never folded; not run again under QTX_NO_TAIL_FOLD, which it does not read),
    the d_ff 2048 FFN2 on each of its row blocks (the module docstring, 33 / 97 / 193).
    QTX_DECODE_GROUPS=2 at 193: groups of 97 and 96 rows on streams of their own, the second
    one's rows 97 .. 192 starting at sentence 97 % 3 = 1."""
    from qtx.decode import greedy_decode
    for k, v in env.items():
        knob_env(k, v)
    src, m = W.default_batch(B)
    exp = golden(oracle_model, B)
    np.testing.assert_array_equal(greedy_decode(gpu_model, src, m, L, 0), exp[0])
    if env is not NO_FOLD:
        ys, sc = greedy_decode(gpu_model, src, m, L, 0, return_scores=True)
        same3((ys, sc.top_ids, sc.top_logp), exp)


# =====================================================================================
# 2. kvtrials: B = 97 and B = 130
# =====================================================================================
def kv_pairs():
    """The six (sentence, trial) pairs of test_gpu_kvtrials' B = 33 test, by sentence."""
    mx, per = KV.mixes(), [[] for _ in range(W.CYCLE)]
    for name, i in KV.PAIRS33:
        per[KV.SENT[i]].append(mx[name][i])
    assert all(per)
    return per


# B -> the rows that must carry a trial: row 0, the last row, and both sides of every block edge
# near the end — 97: the one-row ragged blocks are row 96 (32-, 16- and 8-row blocks alike), 95
# the last row of the full ones, 31 / 32 and 63 / 64 the first tile edges of the row-fault GEMM;
# 130: rows 128, 129 the ragged fifth tile (and the ragged 8- / 16-row blocks and record block),
# 127 the last row of the fourth, 95 / 96 the edge before
KV_EDGES = {97: (0, 31, 32, 63, 64, 95, 96), 130: (0, 95, 96, 127, 128, 129)}


def kv_table(B):
    return W.place(B, kv_pairs(), KV_EDGES[B])


@pytest.mark.parametrize("B", [97, 130])
def test_kvtrials(torch, gpu_model, oracle_model, B):
    """The trial table over 97 / 130 rows: golden graphs up to steps 0, 2 and 5, at each an eager
    faulty step at M = B on the row-fault GEMM (32-row tiles: the last tile one row at 97, two at
    130) and the cache upsets, then graphs again.  One row in five carries no trial and equals
    the golden decode; the trials are the B = 33 test's memoised pairs."""
    from qtx.decode import greedy_decode_kvfault_trials
    trials = kv_table(B)
    none = [r for r, t in enumerate(trials) if t is None]
    assert len(none) >= B // 6 and all(trials[r] is not None for r in KV_EDGES[B])
    assert sorted({t[1] for t in trials if t is not None}) == [0, 2, 5]
    src3, m3 = D.make_src()
    exp = W.kvtrials_rows(oracle_model, src3, m3, L, trials)
    gold = golden(oracle_model, B)
    src, m = W.default_batch(B)
    ys, sc, recs = greedy_decode_kvfault_trials(gpu_model, src, m, L, 0, trials)
    same3((ys, sc.top_ids, sc.top_logp), exp)
    for b, tr in enumerate(trials):
        KV.same_record(recs[b], exp[3][b], None if tr is None else tr[1])
    # the rows without a trial are the golden decode; the trials change tokens in some rows
    same3((ys[none], sc.top_ids[none], sc.top_logp[none]), [a[none] for a in gold])
    assert all(recs[r] is None for r in none)
    assert sum(not np.array_equal(exp[0][r], gold[0][r]) for r in range(B)) >= B // 6


# =====================================================================================
# 3. enctrials: B = 97
# =====================================================================================
def enc_table(B):
    """test_gpu_enctrials' six memoised pairs by sentence, cycled; the last row (sentence 0) takes
    the WEIGHT fault on the memory K projection, the one pair the B = 33 test does not hold."""
    cs, per = EN.T.cases(), [[] for _ in range(W.CYCLE)]
    for name, i in EN.PAIRS33:
        per[EN.T.SENT[i]].append(cs[name][0][i])
    assert all(per)
    faults = W.place(B, per, (0, B - 1))
    faults[B - 1] = cs["B"][0][2]
    assert faults[B - 1].module == 1 and faults[B - 1].linear == "CK"
    return faults


def test_enctrials(torch, gpu_model, oracle_model):
    """97 sentences, 1358 token rows through the table GEMM (11 row tiles, the last ragged), then
    the scored decode on the "big" instances; CK / CV trials (sentence 1's INPUT on CV, sentence
    2's WEIGHT on CK among the cycled pairs) and one more on the last row."""
    from qtx.decode import greedy_decode_enctrials
    B = 97
    faults = enc_table(B)
    none = [r for r, f in enumerate(faults) if f is None]
    assert len(none) >= B // 6
    assert sum(f is not None and f.module == 1 for f in faults) >= 3
    src3, m3 = D.make_src()
    exp = W.enctrials_rows(oracle_model, src3, m3, L, faults)
    gold = golden(oracle_model, B)
    src, m = W.default_batch(B)
    ys, sc = greedy_decode_enctrials(gpu_model, src, m, L, 0, faults)
    same3((ys, sc.top_ids, sc.top_logp), exp)
    same3((ys[none], sc.top_ids[none], sc.top_logp[none]), [a[none] for a in gold])
    assert not np.array_equal(bits(exp[2][B - 1]), bits(gold[2][B - 1]))


# =====================================================================================
# 4. kvfault: B = 97
# =====================================================================================
def kvfault_cases():
    """name -> (trial in the coordinates of its sentence alone, step, row): pairs that
    test_gpu_kvtrials' tables hold for sentence 0 (rows 0 and 96)."""
    from qtx.fault import CacheUpset as U
    from qtx.fault import Fault as F
    return {"output_row96": (F("OUTPUT", 1, 5, "FFN2", row=0, col=100, value=3.0e4), 2, 96),
            "input_row0": (F("INPUT", 1, 2, "V", row=0, col=50, bit=7), 2, 0),
            "self_k_row96": (U("self_k", 0, row=1, col=33, bit=7), 3, 96),
            "cross_v_row96": (U("cross_v", 2, row=13, col=300, bit=7), 0, 96)}


@pytest.mark.parametrize("name", sorted(kvfault_cases()))
def test_kvfault(torch, gpu_model, oracle_model, name):
    """One step fault or upset on one row of 97: golden graphs to the step, the eager faulty
    step at M = 97 (csrc/qtx_fault.hip kvfault_step: the fault-aware linear() and the row
    quantizers, not launch_skinny's instances), graphs after it.  The faulted row is
    tests/kvfault_ref.py's on that sentence alone, every other row — the 32 others that hold the
    same sentence among them — golden."""
    from qtx.decode import greedy_decode_kvfault
    from qtx.fault import Fault
    B = 97
    what, step, row = kvfault_cases()[name]
    src3, m3 = D.make_src()
    exp = W.kvfault_rows(oracle_model, src3, m3, B, L, row, what, step)
    gold = golden(oracle_model, B)
    assert not np.array_equal(bits(exp[2][row]), bits(gold[2][row]))
    wb = W.kv_to_batch(what, row, S, L)
    kw = {"fault": wb} if isinstance(what, Fault) else {"upset": wb}
    src, m = W.default_batch(B)
    ys, sc = greedy_decode_kvfault(gpu_model, src, m, L, 0, step=step, return_scores=True, **kw)
    same3((ys, sc.top_ids, sc.top_logp), exp)
    same_rec(sc.fault_step, exp[3], step)


# =====================================================================================
# 5. dfault and a resume: B = 97
# =====================================================================================
def dfault_trials():
    """[(Fault in the coordinates of sentence 0 alone, target_inference_number)]: OUTPUT faults
    on the last layer's FFN2 at the last token, steps 2 then 1 (a resume goes down)."""
    t = D.trials()
    return [t["output_ffn2"], t["output_ffn2_t2"]]


def test_dfault_and_resume(torch, gpu_model, oracle_model):
    """A linear OUTPUT fault on the last token of sentence 96 at step 2 — golden graphs, the
    faulty full-prefix pass over 97 * 3 token rows, cached steps after it — then a resume on the
    same workspace at step 1.  Both change row 96's token and no other row's."""
    from qtx.model import to_u8_mask
    B, b = 97, 96
    src3, m3 = D.make_src()
    src, m = W.default_batch(B)
    srcd = torch.from_numpy(src).to(gpu_model.device)
    md = to_u8_mask(m, gpu_model.device).reshape(B, S)
    ws = gpu_model.dfault_workspace(B, S, L)
    (f1, tin1), (f2, tin2) = dfault_trials()
    assert tin2 < tin1
    for k, (f, tin) in enumerate(((f1, tin1), (f2, tin2))):
        exp = W.dfault_rows(oracle_model, src3, m3, B, L, b, f, tin)
        fb = W.dfault_to_batch(f, b, tin)
        if k == 0:
            out = gpu_model.greedy_dfault(srcd, md, fb, tin - 1, max_len=L, start=0, scores=True,
                                          ws=ws)
        else:
            out = gpu_model.greedy_dfault_resume(ws, B, S, fb, tin - 1, max_len=L)
        gpu_model.check()
        ys, ti, tl, ri, rl = (t.cpu().numpy() for t in out[:5])
        same3((ys, ti, tl), exp)
        np.testing.assert_array_equal(ri[:, 0], exp[3][0])
        np.testing.assert_array_equal(bits(rl[:, 0]), bits(exp[3][1]))
        np.testing.assert_array_equal(ri[:, 1], exp[3][2])
        np.testing.assert_array_equal(bits(rl[:, 1]), bits(exp[3][3]))
        changed = exp[3][0][:, 0] != exp[3][2][:, 0]
        assert changed.nonzero()[0].tolist() == [b]
        if k == 1:
            np.testing.assert_array_equal(out[5] != 0, changed)


# =====================================================================================
# 6. beam search: 104, 200 and 99 rows
# =====================================================================================
def beam_expect(d_ff, B, beam):
    return W.beam_rows(lambda s: BR.reference(d_ff, 8, 97, beam, rows=(s,)), B)


BEAM = [(512, 13, 8), (2048, 13, 8), (2048, 25, 8), (512, 33, 3)]


@pytest.mark.parametrize("d_ff,B,beam", BEAM)
def test_beam(torch, d_ff, B, beam):
    """B * beam = 104, 200, 99 rows of the fused step (the "big" instances; d_ff 512: FFN2 a
    K = 512 GEMM on k_skinny_wide; d_ff 2048: k_quant_h2048 + the int8 16-row blocks), then
    k_beam_select on B sentences and k_beam_reorder on their caches.  The sentence of the last
    row block (rows >= 96) reorders at some step, so cache rows above row 96 were permuted; at
    (33, 3) two of the three sentences finish after 5 steps and ride along while the batch goes
    on to step 13 (early_exit both ways there)."""
    gm = GB.gpu_model(d_ff)
    src3, m3 = BR.inputs(d_ff)
    src, m = W.batch(src3, m3, B)
    exp = beam_expect(d_ff, B, beam)
    last = (B - 1) % W.CYCLE
    assert (B - 1) * beam >= 96 and W.reorders(exp["refs"][last])
    GB.assert_same(GB.gpu_beam(gm, src, m, beam, early_exit=True), exp, 8, True)
    if (d_ff, B, beam) == BEAM[-1]:
        GB.assert_same(GB.gpu_beam(gm, src, m, beam, early_exit=False), exp, 8, False)


# =====================================================================================
# 7. the workspace: exactly the queried size between guards, one case per driver at its widest B
# =====================================================================================
def dev_inputs(torch, model, src, m):
    B, S_ = src.shape
    return (torch.from_numpy(np.ascontiguousarray(src)).to(model.device),
            torch.from_numpy(np.ascontiguousarray(m).reshape(B, S_).astype(np.uint8)).to(model.device))


def scored_outs(torch, B, rec=False):
    outs = [torch.empty((B, L), dtype=torch.int64, device="cuda"),
            torch.empty((B, L - 1, 2), dtype=torch.int64, device="cuda"),
            torch.empty((B, L - 1, 2), dtype=torch.float32, device="cuda")]
    if rec:
        outs += [torch.empty((B, 2, 2), dtype=torch.int64, device="cuda"),
                 torch.empty((B, 2, 2), dtype=torch.float32, device="cuda")]
    return outs


def host3(outs):
    return [t.cpu().numpy() for t in outs[:3]]


def same_rec_arrays(ri, rl, want):
    ri, rl = ri.cpu().numpy(), rl.cpu().numpy()
    np.testing.assert_array_equal(ri[:, 0], want[0])
    np.testing.assert_array_equal(bits(rl[:, 0]), bits(want[1]))
    np.testing.assert_array_equal(ri[:, 1], want[2])
    np.testing.assert_array_equal(bits(rl[:, 1]), bits(want[3]))


def guarded_ws(torch, need, poison):
    assert need > 0
    return guarded(torch, (int(need),), torch.uint8, poison, name="workspace")


def ws_greedy(torch, model, om, lib, call, poison):
    B = 193
    src, m = W.default_batch(B)
    srcd, md = dev_inputs(torch, model, src, m)
    need = lib.qtx_greedy_workspace_size(model.handle, B, S, L)
    ws, chk = guarded_ws(torch, need, poison)
    ids = torch.empty((B, L), dtype=torch.int64, device="cuda")
    call("qtx_greedy_decode", model.handle, P(srcd), P(md), B, S, L, 0, P(ids), P(ws), need, S0)
    model.check()
    chk()
    np.testing.assert_array_equal(ids.cpu().numpy(), golden(om, B)[0])


def ws_scored(torch, model, om, lib, call, poison):
    B = 193
    src, m = W.default_batch(B)
    srcd, md = dev_inputs(torch, model, src, m)
    need = lib.qtx_greedy_scored_workspace_size(model.handle, B, S, L)
    ws, chk = guarded_ws(torch, need, poison)
    outs = scored_outs(torch, B)
    call("qtx_greedy_decode_scored", model.handle, P(srcd), P(md), B, S, L, 0, *[P(t) for t in outs],
         P(ws), need, None, S0)
    model.check()
    chk()
    same3(host3(outs), golden(om, B))


def ws_kvtrials(torch, model, om, lib, call, poison):
    B = 130
    trials = kv_table(B)
    src, m = W.default_batch(B)
    srcd, md = dev_inputs(torch, model, src, m)
    need = lib.qtx_greedy_kvtrials_workspace_size(model.handle, B, S, L)
    ws, chk = guarded_ws(torch, need, poison)
    outs = scored_outs(torch, B, rec=True)
    call("qtx_greedy_decode_kvtrials", model.handle, P(srcd), P(md), B, S, L, 0,
         *[P(t) for t in outs], P(ws), need, KV.c_trials(trials), S0)
    model.check()
    chk()
    exp = W.kvtrials_rows(om, *D.make_src(), L, trials)
    same3(host3(outs), exp)
    wri, wrl = KV.rec_arrays(exp)
    np.testing.assert_array_equal(outs[3].cpu().numpy(), wri)
    np.testing.assert_array_equal(bits(outs[4].cpu().numpy()), bits(wrl))


def ws_enctrials(torch, model, om, lib, call, poison):
    B = 97
    faults = enc_table(B)
    src, m = W.default_batch(B)
    srcd, md = dev_inputs(torch, model, src, m)
    need = lib.qtx_greedy_enctrials_workspace_size(model.handle, B, S, L)
    ws, chk = guarded_ws(torch, need, poison)
    outs = scored_outs(torch, B)
    call("qtx_greedy_decode_enctrials", model.handle, P(srcd), P(md), B, S, L, 0,
         *[P(t) for t in outs], P(ws), need, EN.c_faults(faults), S0)
    model.check()
    chk()
    same3(host3(outs), W.enctrials_rows(om, *D.make_src(), L, faults))


def ws_kvfault(torch, model, om, lib, call, poison):
    B = 97
    what, step, row = kvfault_cases()["self_k_row96"]
    src, m = W.default_batch(B)
    srcd, md = dev_inputs(torch, model, src, m)
    need = lib.qtx_greedy_kvfault_workspace_size(model.handle, B, S, L)
    ws, chk = guarded_ws(torch, need, poison)
    outs = scored_outs(torch, B, rec=True)
    u = W.kv_to_batch(what, row, S, L).to_c()
    call("qtx_greedy_decode_kvfault", model.handle, P(srcd), P(md), B, S, L, 0,
         *[P(t) for t in outs], P(ws), need, None, C.byref(u), step, S0)
    model.check()
    chk()
    exp = W.kvfault_rows(om, *D.make_src(), B, L, row, what, step)
    same3(host3(outs), exp)
    same_rec_arrays(outs[3], outs[4], exp[3])


def ws_dfault(torch, model, om, lib, call, poison):
    B, b = 97, 96
    src, m = W.default_batch(B)
    srcd, md = dev_inputs(torch, model, src, m)
    need = lib.qtx_greedy_dfault_workspace_size(model.handle, B, S, L)
    ws, chk = guarded_ws(torch, need, poison)
    for k, (f, tin) in enumerate(dfault_trials()):
        outs = scored_outs(torch, B, rec=True)
        fc = W.dfault_to_batch(f, b, tin).to_c()
        if k == 0:
            call("qtx_greedy_decode_dfault", model.handle, P(srcd), P(md), B, S, L, 0,
                 *[P(t) for t in outs], P(ws), need, C.byref(fc), tin - 1, S0)
        else:
            changed = (C.c_int32 * B)()
            call("qtx_greedy_dfault_resume", model.handle, B, S, L, *[P(t) for t in outs], P(ws),
                 need, C.byref(fc), tin - 1, changed, S0)
        model.check()
        chk()
        exp = W.dfault_rows(om, *D.make_src(), B, L, b, f, tin)
        same3(host3(outs), exp)
        same_rec_arrays(outs[3], outs[4], exp[3])


def ws_beam(torch, _model, _om, lib, call, poison):
    d_ff, B, beam = 2048, 25, 8
    ML = BR.MAX_LEN
    gm = GB.gpu_model(d_ff)
    src, m = W.batch(*BR.inputs(d_ff), B)
    S_ = src.shape[1]
    srcd, md = dev_inputs(torch, gm, src, m)
    need = lib.qtx_beam_workspace_size(gm.handle, B, S_, ML, beam)
    ws, chk = guarded_ws(torch, need, poison)
    ids = torch.empty((B, beam, ML), dtype=torch.int64, device="cuda")
    sc = torch.empty((B, beam), dtype=torch.float32, device="cuda")
    ln = torch.empty((B, beam), dtype=torch.int32, device="cuda")
    steps = C.c_int32(-1)
    call("qtx_beam_decode", gm.handle, P(srcd), P(md), B, S_, ML, beam, BR.START, BR.EOS, BR.PAD, 1,
         P(ids), P(sc), P(ln), C.byref(steps), P(ws), need, S0)
    gm.check()
    chk()
    exp = beam_expect(d_ff, B, beam)
    np.testing.assert_array_equal(ids.cpu().numpy(), exp["hyp_ids"])
    np.testing.assert_array_equal(ln.cpu().numpy(), exp["hyp_len"])
    np.testing.assert_array_equal(bits(sc.cpu().numpy()), bits(exp["hyp_score"]))


WS_CASES = {"greedy193": ws_greedy, "scored193": ws_scored, "kvtrials130": ws_kvtrials,
            "enctrials97": ws_enctrials, "kvfault97": ws_kvfault, "dfault97": ws_dfault,
            "beam25x8": ws_beam}


@pytest.mark.parametrize("poison", POISONS, ids=lambda p: "poison%02X" % p)
@pytest.mark.parametrize("name", list(WS_CASES))
def test_workspace(torch, gpu_model, oracle_model, name, poison):
    """Each driver at its widest B on a workspace of exactly the size its query returns, between
    the guards of tests/guarded.py, under both poison bytes: an odd B moves every carved offset,
    so a carve that overlaps shows as a wrong result (a buffer read before it is written holds
    another poison each time) and one that overruns as a changed guard."""
    from qtx import _lib
    WS_CASES[name](torch, gpu_model, oracle_model, _lib.lib(), _lib.call, poison)

"""Teacher-forced target scoring (include/qtx.h, target scoring) on the GPU against
tests/score_ref.py, bit for bit: the tail kernel on crafted rows, the chunked generator, the
whole call on every kind of model, against the scored KV-cached decode and the beam search,
fault trials, refusals, and that the neighbouring entry points are left alone.

Expected values never come from the code under test (score_ref restates the contract over the
oracle); floats are compared by their bit patterns (NaN against NaN).  Outputs sit between
poisoned guard bands (tests/guarded.py) under both poisons: a call writes exactly its outputs.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from oracle import qtx_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_ref as BR  # noqa: E402
import model_cfgs as MC  # noqa: E402
import score_ref as SR  # noqa: E402
from guarded import POISONS, guarded  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
S0 = C.c_void_p(0)
OK, E_INVALID, E_WORKSPACE, E_UNSUPPORTED = 0, 1, 3, 4
_MODELS = {}


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else S0


def status(name, *args):
    from qtx import _lib
    return getattr(_lib.lib(), name)(*args)


def same(got, exp, what=""):
    """Equal shapes and dtypes; floats equal by bit pattern, NaN matching NaN."""
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape, got.dtype)
    if got.dtype == f32:
        np.testing.assert_array_equal(np.isnan(got), np.isnan(exp), err_msg=what)
        ok = ~np.isnan(exp)
        np.testing.assert_array_equal(got.view(np.uint32)[ok], exp.view(np.uint32)[ok], err_msg=what)
    else:
        np.testing.assert_array_equal(got, exp, err_msg=what)


def gpu_model(d_ff, weight_bits=8, tgt_vocab=97, boosted=False):
    """(QtxModel, OracleModel) of one small config, built once per process."""
    from qtx.model import QtxModel
    key = (d_ff, weight_bits, tgt_vocab, boosted)
    if key not in _MODELS:
        if boosted:
            cfg, sd, om = BR.boosted_state(d_ff, weight_bits, tgt_vocab)
        elif key[:3] in MC.SEEDS:
            cfg, sd, om = MC.small_state(d_ff, weight_bits, tgt_vocab)
        else:                       # a vocabulary of the per-op tests only
            from qtx.weights import synthetic_state_dict
            cfg = MC.small_cfg(d_ff, weight_bits, tgt_vocab)
            sd = synthetic_state_dict(1, cfg, ln_random=True)
            om = O.OracleModel(sd, n_layers=cfg.n_layers, n_bits=weight_bits)
        _MODELS[key] = (QtxModel(sd, cfg), om)
    return _MODELS[key]


def outputs(torch, lead, poison, top2=True):
    """Guarded tok_logp / rank [lead] and top_ids / top_logp [lead, 2]; (tensors, checks)."""
    spec = [(lead, torch.float32, "tok_logp"), (lead, torch.int32, "rank")]
    if top2:
        spec += [(lead + (2,), torch.int64, "top_ids"), (lead + (2,), torch.float32, "top_logp")]
    made = [guarded(torch, shp, dt, poison, name=n) for shp, dt, n in spec]
    ts = [m[0] for m in made] + [None] * (4 - len(made))
    return ts, [m[1] for m in made]


def to_np(ts):
    return [None if t is None else t.cpu().numpy() for t in ts]


def score_call(torch, gm, src, mask, tgt, pad=SR.PAD, K=1, faults=(), poison=POISONS[0], top2=True):
    """qtx_score_targets into guarded outputs -> [tok_logp, rank, top_ids, top_logp] (numpy,
    with the trial axis), the guards checked."""
    from qtx import _lib
    B, S = src.shape
    R, L = tgt.shape
    N = len(faults)
    dev = gm.device
    srcd = torch.from_numpy(np.ascontiguousarray(src)).to(dev)
    md = torch.from_numpy(np.ascontiguousarray(np.asarray(mask).reshape(B, S)).astype(np.uint8)).to(dev)
    tgtd = torch.from_numpy(np.ascontiguousarray(tgt)).to(dev)
    ts, checks = outputs(torch, (N + 1, R, L - 1), poison, top2)
    need = _lib.lib().qtx_score_workspace_size(gm.handle, B, S, L, K, N)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    farr = (_lib.Fault * N)(*[f.to_c() for f in faults]) if N else None
    _lib.call("qtx_score_targets", gm.handle, P(srcd), P(md), B, S, P(tgtd), L, K, int(pad), farr, N,
              *[P(t) for t in ts], P(ws), need, S0)
    gm.check()
    for c in checks:
        c()
    return to_np(ts)


def same_ref(got, ref, trial=0, what=""):
    for g, k in zip(got, ("tok_logp", "rank", "top_ids", "top_logp")):
        if g is not None:
            same(g[trial], ref[k], f"{what} {k}")


# =====================================================================================
# 1. the tail alone on crafted rows
# =====================================================================================
@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("M", [1, 5])
@pytest.mark.parametrize("V", [2, 97, 4444, 8200])
def test_score_logits_on_crafted_rows(torch, V, M, poison):
    from qtx import _lib
    x, y = SR.crafted_rows(V)
    n = len(y)
    starts = range(n) if M == 1 else (0, 5, n - 5)
    for s0 in starts:
        xs, ys = x[s0:s0 + M], y[s0:s0 + M]
        exp = SR.score_logits(xs, ys)
        xd, yd = torch.from_numpy(xs.copy()).cuda(), torch.from_numpy(ys.copy()).cuda()
        for top2 in (True, False):
            ts, checks = outputs(torch, (M,), poison, top2)
            _lib.call("qtx_score_logits", P(xd), P(yd), M, V, *[P(t) for t in ts], S0)
            torch.cuda.synchronize()
            for c in checks:
                c()
            for g, e, k in zip(to_np(ts), exp, ("tok_logp", "rank", "top_ids", "top_logp")):
                if g is not None:
                    same(g, e, f"V={V} rows {s0}..+{M} {k}")


# =====================================================================================
# 2. generator chunks + tail
# =====================================================================================
@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("V", [97, 4444])
def test_score_rows_chunks(torch, V, poison):
    """M = 37 rows with workspace for exactly 16 rows (chunks of 16, 16 and 5), for 37 rows (32
    and 5) and for 48 (one chunk): each == the oracle, so equal to each other."""
    from qtx import _lib
    gm, om = gpu_model(512, 8, V)
    M = 37
    rng = np.random.default_rng(V)
    x = rng.standard_normal((M, 512)).astype(f32)
    y = rng.integers(0, V, M).astype(np.int64)
    y[3], y[20], y[36] = V, -1, V - 1
    exp = SR.score_logits(om.logits(x), y)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    for rows in (16, 37, 48):
        ws = torch.empty(rows * V * 4, dtype=torch.uint8, device="cuda")
        ts, checks = outputs(torch, (M,), poison)
        _lib.call("qtx_score_rows", gm.handle, P(xd), M, P(yd), *[P(t) for t in ts], P(ws),
                  ws.numel(), S0)
        torch.cuda.synchronize()
        for c in checks:
            c()
        for g, e, k in zip(to_np(ts), exp, ("tok_logp", "rank", "top_ids", "top_logp")):
            same(g, e, f"ws rows {rows} {k}")
    # fewer than 16 rows' worth of workspace: refused, nothing written
    ts, checks = outputs(torch, (M,), poison)
    ws = torch.empty(16 * V * 4 - 1, dtype=torch.uint8, device="cuda")
    assert status("qtx_score_rows", gm.handle, P(xd), M, P(yd), *[P(t) for t in ts], P(ws),
                  ws.numel(), S0) == E_WORKSPACE
    torch.cuda.synchronize()
    assert all(bool((t.view(torch.uint8) == poison).all()) for t in ts)


# =====================================================================================
# 3. end to end == score_ref
# =====================================================================================
@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("pad", [SR.PAD, -1])
@pytest.mark.parametrize("rows", [None, (0,)], ids=["B3", "B1"])
@pytest.mark.parametrize("cfg", SR.MODELS, ids=str)
def test_end_to_end_equals_the_oracle(torch, cfg, rows, pad, poison):
    gm, _ = gpu_model(*cfg)
    src, mask = SR.inputs()
    tgt = SR.targets(*cfg)
    if rows is not None:
        src, mask, tgt = src[list(rows)], mask[list(rows)], tgt[list(rows)]
    ref = SR.reference(*cfg, pad=pad, rows=rows)
    got = score_call(torch, gm, src, mask, tgt, pad=pad, poison=poison)
    same_ref(got, ref, what=f"{cfg} pad {pad}")            # pad-label positions included
    if poison == POISONS[0]:                               # and without the top 2
        got = score_call(torch, gm, src, mask, tgt, pad=pad, poison=poison, top2=False)
        same_ref(got, ref, what=f"{cfg} pad {pad} no top2")


# =====================================================================================
# 4. against the scored KV-cached decode
# =====================================================================================
@pytest.mark.parametrize("cfg", SR.MODELS, ids=str)
def test_full_prefix_pass_equals_the_cached_scored_decode(torch, cfg):
    """tgt = the GPU's own greedy ids: the full-prefix pass and the (fused or unfused) cached
    step are two independent paths to the same top 2; every label has rank 0."""
    from qtx.decode import greedy_decode
    gm, _ = gpu_model(*cfg)
    src, mask = SR.inputs()
    ys, sc = greedy_decode(gm, src, mask, SR.L, 0, return_scores=True)
    tok, rank, ti, tv = score_call(torch, gm, src, mask, ys, pad=-1)
    same(ti[0], sc.top_ids, "top_ids")
    same(tv[0], sc.top_logp, "top_logp")
    same(tok[0], np.ascontiguousarray(sc.top_logp[..., 0]), "tok_logp")
    assert (rank[0] == 0).all()
    np.testing.assert_array_equal(ys, SR.greedy(*cfg))      # (and the decode is the oracle's)


# =====================================================================================
# 5. beam search: rescoring and tgt_per_src
# =====================================================================================
def test_rescore_beam_and_targets_per_source(torch):
    from qtx.decode import beam_decode, rescore_beam, score_targets
    d_ff, wb, V, beam = BR.MODELS[0]
    gm, _ = gpu_model(d_ff, wb, V, boosted=True)
    src, mask = BR.inputs(d_ff, wb, V)
    res = beam_decode(gm, src, mask, BR.MAX_LEN, BR.START, beam_size=beam)
    ref = BR.reference(d_ff, wb, V, beam)
    np.testing.assert_array_equal(res.hyp_ids, ref["hyp_ids"])
    assert np.isfinite(res.hyp_score).all()
    same(rescore_beam(gm, src, mask, res), res.hyp_score, "rescored hyp_score")
    B, K, L = res.hyp_ids.shape
    tgt = res.hyp_ids.reshape(B * K, L)
    a = score_targets(gm, src, mask, tgt, tgt_per_src=K)
    b = score_targets(gm, np.repeat(src, K, axis=0), np.repeat(mask, K, axis=0), tgt)
    for k in ("tok_logp", "rank", "top_ids", "top_logp"):
        same(getattr(a, k), getattr(b, k), k)
    got = score_call(torch, gm, src, mask, tgt, K=K, poison=POISONS[1])
    same(got[0][0], a.tok_logp, "guarded K = 4")


# =====================================================================================
# 6. fault trials in one call
# =====================================================================================
@pytest.mark.parametrize("poison", POISONS)
def test_fault_trials_in_one_call(torch, poison):
    cfg = SR.MODELS[0]
    gm, _ = gpu_model(*cfg)
    src, mask = SR.inputs()
    tgt = SR.targets(*cfg)
    fl = SR.faults()
    got = score_call(torch, gm, src, mask, tgt, faults=fl, poison=poison)
    assert got[0].shape == (len(fl) + 1, 3, SR.L - 1)
    same_ref(got, SR.reference(*cfg), 0, "trial 0")
    plain = score_call(torch, gm, src, mask, tgt, poison=poison)
    rev = score_call(torch, gm, src, mask, tgt, faults=fl[::-1], poison=poison)
    for n, f in enumerate(fl):
        same_ref(got, SR.reference(*cfg, fault=f), n + 1, f"trial {n + 1}")
        alone = score_call(torch, gm, src, mask, tgt, faults=[f], poison=poison)
        for g, a, p, r in zip(got, alone, plain, rev):
            same(g[n + 1], a[1], f"trial {n + 1} == stand-alone")
            same(g[0], a[0], "golden of a stand-alone call")
            same(g[0], p[0], "trial 0 == the call without faults")
            # the reversed list: the golden buffers survive an encoder-fault trial
            same(g[n + 1], r[len(fl) - n], f"trial {n + 1} reversed")


# =====================================================================================
# 7. refusals, nothing written
# =====================================================================================
def test_refusals_write_nothing(torch):
    from qtx import _lib
    from qtx.fault import Fault
    gm, _ = gpu_model(*SR.MODELS[0])
    gm4, _ = gpu_model(512, 4, 97)
    src, mask = SR.inputs()
    tgt = SR.targets(*SR.MODELS[0])
    B, S = src.shape
    L = tgt.shape[1]
    srcd = torch.from_numpy(src).cuda()
    md = torch.from_numpy(np.ascontiguousarray(mask.reshape(B, S)).astype(np.uint8)).cuda()
    tgt2 = torch.from_numpy(np.repeat(tgt, 2, axis=0)).cuda()
    tgtd = torch.from_numpy(tgt).cuda()
    ts, checks = outputs(torch, (3, 2 * B, L - 1), 0x5A)
    ws = torch.empty(4 * _lib.lib().qtx_score_workspace_size(gm.handle, B, S, L, 2, 2),
                     dtype=torch.uint8, device="cuda")
    good = Fault("WEIGHT", 1, 1, "FFN1", row=77, col=300, bit=6)
    arr = lambda *fs: (_lib.Fault * len(fs))(*[f.to_c() for f in fs])

    def run(model=gm, tgt_=tgtd, L_=L, K=1, faults=None, N=0, nbytes=ws.numel(), B_=B, S_=S):
        return status("qtx_score_targets", model.handle, P(srcd), P(md), B_, S_, P(tgt_), L_, K,
                      SR.PAD, faults, N, *[P(t) for t in ts], P(ws), nbytes, S0)
    assert run(L_=1) == E_INVALID
    assert run(K=0) == E_INVALID
    assert run(L_=66) == E_INVALID                          # L - 1 above the 64-row positional table
    assert run(N=-1) == E_INVALID
    assert run(N=1) == E_INVALID                            # no fault array
    assert run(faults=arr(Fault("NONE", 1, 0, "Q")), N=1) == E_INVALID
    assert run(faults=arr(Fault("INPUT", 2, 0, "Q")), N=1) == E_INVALID
    assert run(tgt_=tgt2, K=2, faults=arr(good), N=1) == E_UNSUPPORTED
    assert run(model=gm4, faults=arr(good), N=1) == E_UNSUPPORTED
    past = Fault("INPUT", 1, 1, "FFN1", row=B * (L - 1), col=100, bit=6)
    assert run(faults=arr(good, past), N=2) == E_INVALID
    assert run(faults=arr(Fault("INPUT", 0, 1, "FFN2", row=B * S, col=100, bit=6)), N=1) == E_INVALID
    assert run(faults=arr(Fault("RANDOM", 1, 0, "CK", row=B * S, col=0, value=1.0)), N=1) == E_INVALID
    need = _lib.lib().qtx_score_workspace_size(gm.handle, B, S, L, 1, 1)
    assert run(faults=arr(good), N=1, nbytes=need - 256) == E_WORKSPACE
    torch.cuda.synchronize()
    for c in checks:
        c()
    assert all(bool((t.view(torch.uint8) == 0x5A).all()) for t in ts)
    assert run(faults=arr(good), N=1, nbytes=need) == OK    # and the good call goes through
    gm.check()
    with pytest.raises(ValueError):
        from qtx.decode import score_targets
        bad = tgt.copy()
        bad[1, 3] = 97
        score_targets(gm, src, mask, bad)


def test_workspace_size_is_monotone(torch):
    """More sentences, longer sources or targets, more targets per sentence or fault trials
    never need less workspace."""
    from qtx import _lib
    gm, _ = gpu_model(*SR.MODELS[0])
    size = lambda *a: _lib.lib().qtx_score_workspace_size(gm.handle, *a)
    base = (3, 9, 10, 1, 0)
    assert size(*base) > 0
    for i in range(5):
        prev = size(*base)
        for step in range(1, 4):
            a = list(base)
            a[i] += step
            assert size(*a) >= prev, (i, a)
            prev = size(*a)


# =====================================================================================
# 8. neighbours untouched
# =====================================================================================
def test_neighbours_are_left_alone(torch):
    from qtx import _lib
    from qtx.decode import greedy_decode
    from qtx.fault import Fault
    cfg = SR.MODELS[0]
    gm, _ = gpu_model(*cfg)
    src, mask = SR.inputs()
    tgt = SR.targets(*cfg)
    B, S = src.shape
    L = SR.L
    before = greedy_decode(gm, src, mask, L, 0, return_scores=True)
    score_call(torch, gm, src, mask, tgt, faults=SR.faults()[:1])
    after = greedy_decode(gm, src, mask, L, 0, return_scores=True)
    np.testing.assert_array_equal(after[0], before[0])
    same(after[1].top_logp, before[1].top_logp, "scored decode after a score call")
    # a score call on a decoder-fault decode's workspace drops its header
    lib = _lib.lib()
    need = max(lib.qtx_greedy_dfault_workspace_size(gm.handle, B, S, L),
               lib.qtx_score_workspace_size(gm.handle, B, S, L, 1, 0))
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    srcd = torch.from_numpy(src).cuda()
    md = torch.from_numpy(np.ascontiguousarray(mask.reshape(B, S)).astype(np.uint8)).cuda()
    tgtd = torch.from_numpy(tgt).cuda()
    ids = torch.empty((B, L), dtype=torch.int64, device="cuda")
    ti = torch.empty((B, L - 1, 2), dtype=torch.int64, device="cuda")
    tl = torch.empty((B, L - 1, 2), dtype=torch.float32, device="cuda")
    ri = torch.empty((B, 2, 2), dtype=torch.int64, device="cuda")
    rl = torch.empty((B, 2, 2), dtype=torch.float32, device="cuda")
    f = Fault("INPUT", 1, 1, "FFN1", row=0, col=100, bit=6).to_c()

    def resume(step):
        return lib.qtx_greedy_dfault_resume(gm.handle, B, S, L, P(ids), P(ti), P(tl), P(ri), P(rl),
                                            P(ws), need, C.byref(f), step, None, S0)
    _lib.call("qtx_greedy_decode_dfault", gm.handle, P(srcd), P(md), B, S, L, 0, P(ids), P(ti), P(tl),
              P(ri), P(rl), P(ws), need, C.byref(f), 2, S0)
    assert resume(1) == OK                                   # the header is there ...
    ts, _ = outputs(torch, (1, B, L - 1), 0xA5, top2=False)
    _lib.call("qtx_score_targets", gm.handle, P(srcd), P(md), B, S, P(tgtd), L, 1, SR.PAD, None, 0,
              *[P(t) for t in ts], P(ws), need, S0)
    assert resume(1) == E_INVALID                            # ... and gone after the score call
    gm.check()


# =====================================================================================
# 9. perplexity
# =====================================================================================
def test_perplexity_equals_the_oracle_backed_evaluation(torch):
    from qtx import data
    from qtx.decode import TargetScores
    cfg = SR.MODELS[0]
    gm, om = gpu_model(*cfg)
    words_s, words_t = [f"s{i}" for i in range(60)], [f"t{i}" for i in range(93)]
    vs, vt = data.Vocab(list(data.SPECIALS) + words_s), data.Vocab(list(data.SPECIALS) + words_t)
    rng = np.random.default_rng(3)
    pairs = [(" ".join(rng.choice(words_s, int(rng.integers(2, 7)))),
              " ".join(rng.choice(words_t, int(rng.integers(1, 8))))) for _ in range(5)]

    def oracle_score(s, m, t):
        r = SR.score_ref(om, s, m, t, pad=SR.PAD)
        return TargetScores(r["tok_logp"], r["rank"], None, None, t[:, 1:], pad=SR.PAD)
    exp = data.perplexity(None, pairs, vs, vt, batch_size=3, max_padding=12, score=oracle_score)
    got = data.perplexity(gm, pairs, vs, vt, batch_size=3, max_padding=12)
    np.testing.assert_array_equal(got.sentence_logp, exp.sentence_logp)
    assert (got.nll, got.n_tokens, got.ppl, got.token_accuracy) == \
        (exp.nll, exp.n_tokens, exp.ppl, exp.token_accuracy)
    assert got.n_tokens > 0 and np.isfinite(got.ppl)

"""The fused decode step for vocabularies of 8193 to 65536 words (csrc/qtx_decode_wide.hip:
k_tok_wide, k_top2_wide; include/qtx_wide_vocab.h) against the oracle, bit for bit.

Per-op sizes: 97 (the narrow range through the wide kernels), 8193 (one element past the old
cap and past a 4096-element chunk border), 65521 (prime: a one-column last strip, a ragged last
64-lane round and a ragged last chunk), 65536 (the cap, every chunk full).  Rows: crafted_rows
(ties in different chunks and waves, a logp collision, -inf entries, the non-finite kinds) and
64 random rows, of which at least two per size must tell the canonical denominator from a sum of
per-chunk sums and from a correctly rounded sum (asserted on the CPU: without it random rows
would not see a wrong summation order).  The per-op entries run at the device counter; the
model-level decodes run the host-known positions (default, QTX_NO_GRAPH) and the counter
(QTX_GRAPH_STEPS=4)."""
import os
import sys

import numpy as np
import pytest

from oracle import qtx_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_ref as BR  # noqa: E402
import model_cfgs as MC  # noqa: E402
from guarded import guarded  # noqa: E402
from test_gpu_beam import assert_same, gpu_beam  # noqa: E402
from test_gpu_long_fused import stats  # noqa: E402
from test_gpu_scored import (P, S0, call, crafted_rows, gpu_scored, memo, oracle_scored_decode,  # noqa: E402,F401
                             top2_of, torch)

pytestmark = pytest.mark.gpu
f32 = np.float32
NEG, IMAX, CHUNK = f32(-3.0e38), 2 ** 31 - 1, 4096


def strip_records(lg):
    """[M, V] logits -> [M, ceil(V / 16), 4] f32: launch_generator_mfma's record per 16-column
    strip, {m1, m2, i1 (int32 bits), flags (int32 bits)} (include/qtx.h qtx_decode_generator)."""
    M, V = lg.shape
    n = -(-V // 16)
    x = np.zeros((M, n * 16), f32)
    x[:, :V] = lg
    x, ok = x.reshape(M, n, 16), (np.arange(n * 16) < V).reshape(1, n, 16)
    c = np.where(ok, np.fmax(NEG, x), NEG)
    m1 = c.max(-1)
    eq = ok & (x == m1[..., None])
    i1 = np.where(eq.any(-1), 16 * np.arange(n) + eq.argmax(-1), IMAX).astype(np.int32)
    m2 = np.where(eq & (eq.cumsum(-1) == 1), NEG, c).max(-1)      # without the first holder of m1
    fl = ((ok & ~(x < np.inf)).any(-1) * 1 | (ok & (x > -np.inf)).any(-1) * 2).astype(np.int32)
    return np.stack([m1, m2, i1.view(f32), fl.view(f32)], -1)


def rows_of(V):
    """(logits [n, V], oracle ids, top-2 ids, top-2 logp): crafted rows, then 64 random ones."""
    def make():
        rnd = (np.random.default_rng(V).standard_normal((64, V)) * 2).astype(f32)
        if V > CHUNK:   # the random rows see the summation order (two wrong models)
            e = O.qexp(rnd - rnd.max(-1, keepdims=True))
            lse = np.log(O.row_sum_lanesplit(e))
            chunked = np.zeros(64, f32)
            for c0 in range(0, V, CHUNK):
                chunked = chunked + O.row_sum_lanesplit(e[:, c0:c0 + CHUNK])
            for wrong in (chunked, e.sum(-1, dtype=np.float64).astype(f32)):
                assert (np.log(wrong) != lse).sum() >= 2
        lg = np.concatenate([crafted_rows(V, 100 + V)[0], rnd])
        lp, ids = O.log_softmax_argmax(lg)
        return (lg, ids) + top2_of(lp)
    return memo(("wide_rows", V), make)


@pytest.fixture(scope="module")
def tail_models(torch):
    """One-layer d_ff 512 models by tgt_vocab (the tails read their tables alone), built once."""
    from qtx.model import QtxModel
    from qtx.weights import ModelConfig, synthetic_state_dict
    cache = {}

    def get(V):
        if V not in cache:
            cfg = ModelConfig(src_vocab=16, tgt_vocab=V, n_layers=1, d_ff=512, max_len=64)
            sd = synthetic_state_dict(7, cfg)
            cache[V] = (QtxModel(sd, cfg), np.asarray(sd["tgt_embed.0.lut.weight"], f32))
        return cache[V]
    yield get
    cache.clear()


@pytest.mark.parametrize("kind", ["tok", "top2"])
@pytest.mark.parametrize("V", [97, 8193, 65521, 65536])
def test_wide_tail(torch, tail_models, oracle_model, V, kind):
    """Every row in one launch at the device counter (s = 3): ids, top ids, top logp and x_next
    == the oracle; the other columns, the guard bands and the arrival counter stay; the position
    advances once."""
    gm, lut = tail_models(V)
    lg, want_id, want_i, want_v = rows_of(V)
    M, ids_bs, s = len(lg), 7, 3
    assert np.array_equal(want_i[:, 0], want_id) and np.isnan(want_v[-67:-64]).all()
    lgd = torch.from_numpy(lg).cuda()
    dt = {np.int64: torch.int64, np.int32: torch.int32, f32: torch.float32}
    bufs, checks = {}, []
    for name, shape, k in (("ids", (M, ids_bs), np.int64), ("top_ids", (M, ids_bs - 1, 2), np.int64),
                           ("top_logp", (M, ids_bs - 1, 2), f32), ("x_next", (M, 512), f32),
                           ("step", (2,), np.int32)):
        bufs[name], c = guarded(torch, shape, dt[k], 0xA5, name=name)
        checks.append(c)
    ids0 = np.arange(M * ids_bs, dtype=np.int64).reshape(M, ids_bs) - 50
    bufs["ids"].copy_(torch.from_numpy(ids0))
    bufs["step"].copy_(torch.tensor([s, 0], dtype=torch.int32))
    before = {n: bufs[n].cpu().numpy().copy() for n in ("top_ids", "top_logp")}
    if kind == "tok":
        rec = torch.from_numpy(strip_records(lg)).cuda()
        call("qtx_decode_tok_wide", gm.handle, P(lgd), P(rec), M, P(bufs["ids"]), ids_bs,
             P(bufs["step"]), P(bufs["x_next"]), S0)
    else:
        call("qtx_decode_top2_wide", gm.handle, P(lgd), M, P(bufs["ids"]), ids_bs, P(bufs["top_ids"]),
             P(bufs["top_logp"]), P(bufs["step"]), P(bufs["x_next"]), S0)
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:       # a device fault: nothing more may run on this GPU
        pytest.exit(f"GPU error at synchronize, stopping the session: {e}", returncode=3)
    for c in checks:
        c()
    got = {n: t.cpu().numpy() for n, t in bufs.items()}
    ids1 = ids0.copy()
    ids1[:, s + 1] = want_id
    np.testing.assert_array_equal(got["ids"], ids1)
    np.testing.assert_array_equal(got["step"], [s + 1, 0])
    np.testing.assert_array_equal(got["x_next"], oracle_model.embed(want_id[:, None], lut, pos0=s + 1)[:, 0])
    if kind == "top2":
        before["top_ids"][:, s], before["top_logp"][:, s] = want_i, want_v
    np.testing.assert_array_equal(got["top_ids"], before["top_ids"])
    np.testing.assert_array_equal(got["top_logp"].view(np.uint32), before["top_logp"].view(np.uint32))


# ---- model level: two layers, B = 3, S = 9, 9 tokens (test_config_large_vocab's shapes) --------
WIDE = {8200: 512, 12289: 2048}      # tgt_vocab -> d_ff
L = 9


def wide_case(V):
    """(cfg, state dict, src, mask, the oracle's scored decode) of one model, once."""
    def make():
        from qtx.weights import ModelConfig, synthetic_state_dict
        cfg = ModelConfig(src_vocab=64, tgt_vocab=V, n_layers=2, d_ff=WIDE[V], max_len=64)
        sd = synthetic_state_dict(1, cfg, ln_random=True)
        src, m = MC.small_src(3, 9, 5, full=(0,))
        ref = oracle_scored_decode(O.OracleModel(sd, n_layers=2, n_bits=8), src, m, L)
        assert MC.distinct_tokens(ref[0]) >= 3, ref[0]      # (a stuck cache would repeat a token)
        return cfg, sd, src, m, ref
    return memo(("wide_case", V), make)


def fresh(V):
    from qtx.model import QtxModel
    cfg, sd = wide_case(V)[:2]
    gm = QtxModel(sd, cfg)
    gm.workspace(64 << 20)        # sized once: every call carves the same memory
    return gm


@pytest.mark.parametrize("env", [{}, {"QTX_NO_GRAPH": 1}, {"QTX_GRAPH_STEPS": 4}, {"QTX_UNFUSED": 1}],
                         ids=["default", "no_graph", "graph_steps_4", "unfused"])
@pytest.mark.parametrize("V", sorted(WIDE))
def test_greedy_and_scored(torch, knob_env, V, env):
    from qtx.decode import greedy_decode
    for k, v in env.items():
        knob_env(k, v)
    _, _, src, m, (oy, oi, ov) = wide_case(V)
    gm = fresh(V)
    np.testing.assert_array_equal(greedy_decode(gm, src, m, L, 0), oy)
    gy, gi, gv = gpu_scored(gm, src, m, L)
    np.testing.assert_array_equal(gy, oy)
    np.testing.assert_array_equal(gi, oi)
    np.testing.assert_array_equal(gv, ov)


@pytest.mark.parametrize("scored", [False, True], ids=["plain", "scored"])
@pytest.mark.parametrize("V", sorted(WIDE))
def test_decode_is_captured(torch, V, scored):
    """The decode runs on graphs of the fused step: at least one capture by the first call, none
    by the second, and both calls give the oracle's ids."""
    from qtx.decode import greedy_decode
    _, _, src, m, (oy, _, _) = wide_case(V)
    gm = fresh(V)
    assert stats(gm) == (0, 0)
    seen = []
    for _ in range(2):
        ys = gpu_scored(gm, src, m, L)[0] if scored else greedy_decode(gm, src, m, L, 0)
        np.testing.assert_array_equal(ys, oy)
        seen.append(stats(gm))
    assert seen[0][1] >= 1 and seen[1] == seen[0], seen


def test_beam_is_fused(torch):
    """beam 4 on the beam tests' 8200-word model == beam_ref, on captured graphs."""
    from qtx.model import QtxModel
    cfg, sd, _ = BR.boosted_state(512, 8, 8200)
    gm = QtxModel(sd, cfg)
    gm.workspace(64 << 20)
    src, m = BR.inputs(512, 8, 8200)
    seen = []
    for _ in range(2):
        assert_same(gpu_beam(gm, src, m, 4), BR.reference(512, 8, 8200, 4))
        seen.append(stats(gm))
    assert seen[0][1] >= 1 and seen[1] == seen[0], seen

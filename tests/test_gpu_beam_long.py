"""The beam decode past 128 positions on the fused step (csrc/qtx_decode_beam.hip):
k_dec_attn_beam through qtx_decode_attention_beam against the oracle's cached decoder attention
on caches gathered through the ancestry table in numpy, k_beam_ancestry through
qtx_beam_ancestry against a numpy gather, and qtx_beam_decode at max_len 140 / 137 and S = 132
against tests/beam_ref.py — all bit for bit."""
import os
import sys

import numpy as np
import pytest

from oracle import qtx_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_long as BL  # noqa: E402
import long_target as LT  # noqa: E402
from guarded import guarded  # noqa: E402
from test_gpu_beam import assert_same, gpu_beam  # noqa: E402
from test_gpu_fused import P, S0, call, dev, head_max, torch, vgroup4  # noqa: E402,F401
from test_gpu_long_fused import filled, stats  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
NS = 2      # sentences of the op tests


def table(pattern, K, n):
    """anc [NS * K, n]: the slot that holds position j of row b * K + k."""
    k, j = np.arange(K)[:, None], np.arange(n)[None, :]
    other, cyc = np.broadcast_to((k + 1) % K, (K, n)), (k + j) % K
    t = {"identity": np.broadcast_to(k, (K, n)), "other": other, "cycle": cyc,
         "alternate": np.where((j // 4) % 2 == 0, other, cyc)}[pattern]
    return np.tile(t, (NS, 1)).astype(np.uint8)


@pytest.mark.parametrize("K", [3, 8])
@pytest.mark.parametrize("pattern", ["identity", "other", "cycle", "alternate"])
@pytest.mark.parametrize("step,kv_bs", [(s, 512) for s in (1, 3, 4, 5, 127, 128, 129, 511)] + [(139, 140)])
def test_attention_op(torch, step, kv_bs, pattern, K):
    """Every cache row holds its own random codes and scales, so a position read from the wrong
    slot changes the context.  "cycle" makes every value group mixed (the assemble path),
    "alternate" every other one.  Sentence 0's entry of position 0 lies one above the last slot
    and must be read as that slot; the entries from `step` on hold other slots and must not
    matter.  Only the own slot's row `step` of the caches may change."""
    R, n = NS * K, step + 1
    rng = np.random.default_rng(1000 * K + step)
    y = rng.standard_normal((R, 1536)).astype(f32)
    kc, vc = (rng.integers(-127, 128, (R, kv_bs, 512)).astype(np.int8) for _ in range(2))
    skc, svc = (rng.uniform(0.002, 0.03, (R, kv_bs)).astype(f32) for _ in range(2))
    anc = table(pattern, K, kv_bs)
    anc[:K, 0] = K
    anc[:, step:] = (anc[:, step:] + 1) % K
    rows = (np.arange(R)[:, None] // K) * K + np.minimum(anc, K - 1)     # [R, kv_bs] cache rows
    j = np.arange(kv_bs)[None, :]
    gk, gv, gsk, gsv = kc[rows, j], vc[rows, j], skc[rows, j], svc[rows, j]
    qq, sq = O.quant_rows(y[:, :512])
    kc[:, step], skc[:, step] = gk[:, step], gsk[:, step] = O.quant_rows(y[:, 512:1024])
    vc[:, step], svc[:, step] = gv[:, step], gsv[:, step] = O.quant_rows(y[:, 1024:])
    ctx, _ = O.attention(qq[:, None], sq[:, None], gk[:, :n], gsk[:, :n], gv[:, :n], gsv[:, :n],
                         np.ones((R, 1, n), np.uint8), dec=True)
    stale = rng.integers(-127, 128, (4, R, 512)).astype(np.int8)         # row `step` before the call
    bufs = []
    for a, nm in ((kc, "kc"), (vgroup4(vc), "vc"), (skc, "skc"), (svc, "svc")):
        t, chk = filled(torch, a, nm)
        bufs.append((t, chk))
    (kcd, vcd, skd, svd), checks = zip(*bufs)
    kcd[:, step] = dev(torch, stale[0])
    vcd[:, step >> 2, :, step & 3] = dev(torch, stale[1])
    skd[:, step], svd[:, step] = 7.0, 9.0
    ctxd, c0 = guarded(torch, (R, 512), torch.float32, 0x5A, name="ctx")
    pm, c1 = guarded(torch, (8, R), torch.float32, 0x5A, name="pmax")
    call("qtx_decode_attention_beam", P(dev(torch, y)), 1536, P(kcd), P(vcd), P(skd), P(svd), kv_bs,
         P(dev(torch, np.array([step], np.int32))), P(dev(torch, anc)), K, R, P(ctxd), P(pm), S0)
    torch.cuda.synchronize()
    for chk in checks + (c0, c1):
        chk()
    for got, want in ((ctxd, ctx[:, 0]), (pm, head_max(ctx[:, 0])), (kcd, kc), (vcd, vgroup4(vc)),
                      (skd, skc), (svd, svc)):
        np.testing.assert_array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("n,ML", [(1, 512), (130, 512), (512, 512), (138, 140)])
@pytest.mark.parametrize("parents", [(2, 0, 0), (7, 0, 0, 3, 5, 6, 1, 2), (0, 1, 2)],
                         ids=["beam3", "beam8", "identity"])
def test_ancestry_op(torch, parents, n, ML):
    """The prefix of the table == a numpy gather by parent (sentence 1: the vector rolled by
    one, except the identity); the bytes past it, the guards and the step words stay."""
    K = len(parents)
    par = np.array([parents, np.roll(parents, parents != tuple(range(K)))], np.int32).reshape(-1)
    anc = np.random.default_rng(n + K).integers(0, K, (NS * K, ML)).astype(np.uint8)
    ancd, chk = filled(torch, anc, "anc")
    step = dev(torch, np.array([n, 0, 0, 0], np.int32))
    call("qtx_beam_ancestry", P(ancd), NS, K, ML, P(step), P(dev(torch, par)), S0)
    torch.cuda.synchronize()
    chk()
    want = anc.copy()
    want[:, :n] = anc[(np.arange(NS)[:, None] * K + par.reshape(NS, K)).reshape(-1), :n]
    np.testing.assert_array_equal(ancd.cpu().numpy(), want)
    np.testing.assert_array_equal(step.cpu().numpy(), [n, 0, 0, 0])


# ---- model level ---------------------------------------------------------------------------
def fresh():
    from qtx.model import QtxModel
    cfg, sd, _ = BL.state()
    return QtxModel(sd, cfg)


@pytest.mark.parametrize("env,L,rows,early", [
    ({}, LT.L, None, False), ({}, LT.L, None, True), ({"QTX_NO_GRAPH": 1}, LT.L, None, False),
    ({"QTX_GRAPH_STEPS": 8}, 137, (0,), False), ({"QTX_UNFUSED": 1}, LT.L, None, False)],
    ids=["default", "early_exit", "no_graph", "graph_steps_8", "unfused"])
def test_beam_decode(torch, knob_env, env, L, rows, early):
    """beam 3 at max_len 140 (139 steps: 17 graphs of 8 and 3 replays of the one-step graph)
    and 137 (QTX_GRAPH_STEPS=8: 17 graphs, the last ones past 128) == beam_ref: ids, lengths,
    score bits, steps_run.  The final hypotheses descend through moves at step 129
    (tests/test_beam_long_ref.py)."""
    for k, v in env.items():
        knob_env(k, v)
    src, m = BL.inputs(rows=rows)
    assert_same(gpu_beam(fresh(), src, m, BL.BEAM, early_exit=early, max_len=L),
                BL.reference(L, rows=rows), early=early)


def test_long_source_short_target(torch):
    """S = 132, max_len 12: the fused step with the reorder, its cross side past 128 keys."""
    src, m = BL.inputs(long_src=True)
    assert_same(gpu_beam(fresh(), src, m, BL.BEAM, early_exit=False, max_len=12),
                BL.reference(12, long_src=True), early=False)


def test_route_is_captured(torch):
    """The long beam decode runs on graphs of the fused step: at least one capture by the first
    call, none by the second."""
    gm = fresh()
    gm.workspace(64 << 20)        # sized once: every call carves the same memory
    src, m = BL.inputs()
    assert stats(gm) == (0, 0)
    seen = []
    for _ in range(2):
        assert_same(gpu_beam(gm, src, m, BL.BEAM, early_exit=False, max_len=LT.L), BL.reference(),
                    early=False)
        seen.append(stats(gm))
    assert seen[0][1] >= 1 and seen[1] == seen[0], seen

"""The beam decode past 128 positions for models with 4 and 16 heads
(csrc/qtx_decode_beam_heads.hip): k_dec_attn_beam_hd through qtx_decode_attention_beam_heads
against the oracle's cached decoder attention at that head count, on caches gathered through the
ancestry table in numpy, and qtx_beam_decode at max_len 140 / 137 against tests/beam_ref.py — all
bit for bit.

The model is test_gpu_heads_model.model(H).  Picked on the CPU: beam 4 on the two sentences of
model_cfgs.small_src(2, 9, 5, full=(0,)), test_gpu_heads_model.test_beam's — for both head counts
every final hypothesis of sentence 0 then descends through slots whose parents at steps 132 to
137 are other slots (long_target.beam_late_moves), so an attention that ignored the table past
128 keys would fail.  (Beam 3 on the same sentences meets the condition too.)"""
import os
import sys

import numpy as np
import pytest

from oracle import qtx_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_ref as R  # noqa: E402
import long_target as LT  # noqa: E402
import model_cfgs as MC  # noqa: E402
from guarded import guarded  # noqa: E402
from test_gpu_beam import assert_same, gpu_beam  # noqa: E402
from test_gpu_beam_long import NS, table  # noqa: E402
from test_gpu_fused import P, S0, call, dev, head_max, torch, vgroup4  # noqa: E402,F401
from test_gpu_heads_model import graph_captures, model  # noqa: E402
from test_gpu_long_fused import filled  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
HEADS = (4, 16)
BEAM, SRC_SEED = 4, 5
STEPS = [(s, 512) for s in (1, 3, 4, 5, 127, 128, 129, 255, 256, 511)] + [(139, 140)]


def op_case(torch, step, kv_bs, pattern, K, H):
    """test_gpu_beam_long.test_attention_op's buffers: (args of the entry up to pmax, device
    buffers, guard checks, expected (ctx, pmax, kc, vc, skc, svc))."""
    R_, n = NS * K, step + 1
    rng = np.random.default_rng(1000 * K + step + H)
    y = rng.standard_normal((R_, 1536)).astype(f32)
    kc, vc = (rng.integers(-127, 128, (R_, kv_bs, 512)).astype(np.int8) for _ in range(2))
    skc, svc = (rng.uniform(0.002, 0.03, (R_, kv_bs)).astype(f32) for _ in range(2))
    anc = table(pattern, K, kv_bs)
    anc[:K, 0] = K
    anc[:, step:] = (anc[:, step:] + 1) % K
    rows = (np.arange(R_)[:, None] // K) * K + np.minimum(anc, K - 1)    # [R, kv_bs] cache rows
    j = np.arange(kv_bs)[None, :]
    gk, gv, gsk, gsv = kc[rows, j], vc[rows, j], skc[rows, j], svc[rows, j]
    qq, sq = O.quant_rows(y[:, :512])
    kc[:, step], skc[:, step] = gk[:, step], gsk[:, step] = O.quant_rows(y[:, 512:1024])
    vc[:, step], svc[:, step] = gv[:, step], gsv[:, step] = O.quant_rows(y[:, 1024:])
    ctx, _ = O.attention(qq[:, None], sq[:, None], gk[:, :n], gsk[:, :n], gv[:, :n], gsv[:, :n],
                         np.ones((R_, 1, n), np.uint8), H, dec=True)
    stale = rng.integers(-127, 128, (2, R_, 512)).astype(np.int8)        # row `step` before the call
    (kcd, vcd, skd, svd), checks = zip(*(filled(torch, a, nm) for a, nm in (
        (kc, "kc"), (vgroup4(vc), "vc"), (skc, "skc"), (svc, "svc"))))
    kcd[:, step] = dev(torch, stale[0])
    vcd[:, step >> 2, :, step & 3] = dev(torch, stale[1])
    skd[:, step], svd[:, step] = 7.0, 9.0
    ctxd, c0 = guarded(torch, (R_, 512), torch.float32, 0x5A, name="ctx")
    pm, c1 = guarded(torch, (8, R_), torch.float32, 0x5A, name="pmax")
    args = (P(dev(torch, y)), 1536, P(kcd), P(vcd), P(skd), P(svd), kv_bs,
            P(dev(torch, np.array([step], np.int32))), P(dev(torch, anc)), K, R_, P(ctxd), P(pm))
    want = (ctx[:, 0], head_max(ctx[:, 0]), kc, vgroup4(vc), skc, svc)
    return args, (ctxd, pm, kcd, vcd, skd, svd), checks + (c0, c1), want


@pytest.mark.parametrize("K", [3, 8])
@pytest.mark.parametrize("pattern", ["identity", "cycle", "alternate"])
@pytest.mark.parametrize("step,kv_bs", STEPS)
@pytest.mark.parametrize("H", HEADS)
def test_attention_op(torch, H, step, kv_bs, pattern, K):
    """Every cache row holds its own random codes and scales, so a position read from the wrong
    slot, head half or k-step changes the context.  "cycle" makes every value group mixed,
    "alternate" every other one; steps 255 / 256 / 511 reach waves 2 and 3.  Sentence 0's entry
    of position 0 lies one above the last slot and must be read as that slot; the entries from
    `step` on hold other slots and must not matter.  Only the own slot's row `step` of the
    caches may change."""
    args, bufs, checks, want = op_case(torch, step, kv_bs, pattern, K, H)
    call("qtx_decode_attention_beam_heads", *args, H, S0)
    torch.cuda.synchronize()
    for chk in checks:
        chk()
    for got, exp in zip(bufs, want):
        np.testing.assert_array_equal(got.cpu().numpy(), exp)


def test_eight_heads_is_the_64_wide_entry(torch):
    outs = []
    for name, tail in (("qtx_decode_attention_beam_heads", (8, S0)), ("qtx_decode_attention_beam", (S0,))):
        args, bufs, checks, _ = op_case(torch, 129, 512, "alternate", 3, 8)
        call(name, *args, *tail)
        torch.cuda.synchronize()
        outs.append([b.cpu().numpy() for b in bufs])
    for a, b in zip(*outs):
        np.testing.assert_array_equal(a, b)


def test_six_heads_refused(torch):
    from qtx import _lib
    args, bufs, checks, _ = op_case(torch, 5, 512, "cycle", 3, 4)
    before = [b.cpu().numpy() for b in bufs]
    with pytest.raises(_lib.QtxError) as e:
        call("qtx_decode_attention_beam_heads", *args, 6, S0)
    assert e.value.code == 1
    torch.cuda.synchronize()
    for chk in checks:
        chk()
    for b, was in zip(bufs, before):
        np.testing.assert_array_equal(b.cpu().numpy(), was)


# ---- model level ---------------------------------------------------------------------------
def case(H, L=LT.L, rows=(0, 1)):
    """(src, mask, beam_ref) of the picked sentences, the reference once per (H, L, rows)."""
    src, m = MC.small_src(2, 9, SRC_SEED, full=(0,))
    src, m = src[list(rows)], m[list(rows)]
    return src, m, LT.memo(("beam_heads", H, L, rows), lambda: R.beam_ref(model(H)[1], src, m, L, BEAM))


@pytest.mark.parametrize("env,L,rows,early", [
    ({}, LT.L, (0, 1), False), ({}, LT.L, (0, 1), True), ({"QTX_NO_GRAPH": 1}, LT.L, (0, 1), False),
    ({"QTX_GRAPH_STEPS": 8}, 137, (0,), False)],
    ids=["default", "early_exit", "no_graph", "graph_steps_8"])
@pytest.mark.parametrize("H", HEADS)
def test_beam_decode(torch, knob_env, H, env, L, rows, early):
    src, m, ref = case(H, L, rows)
    if L == LT.L:
        assert LT.beam_late_moves(ref) and min(s for _, _, s in LT.beam_late_moves(ref)) >= 129
    for k, v in env.items():
        knob_env(k, v)
    assert_same(gpu_beam(model(H)[0], src, m, BEAM, early_exit=early, max_len=L), ref, early=early)


@pytest.mark.parametrize("H", HEADS)
def test_route_is_captured(torch, H):
    """The long beam decode of a 4- / 16-head model runs on graphs of the fused step: the first
    call captures at least one, the second adds none."""
    import dataclasses
    from qtx.model import QtxModel
    from qtx.weights import synthetic_state_dict
    cfg = dataclasses.replace(MC.small_cfg(512), n_heads=H, max_len=160)
    gm = QtxModel(synthetic_state_dict(1, cfg, ln_random=True), cfg)     # a fresh graph cache
    gm.workspace(64 << 20)        # sized once: every call carves the same memory
    src, m, ref = case(H)
    seen = [graph_captures(gm)]
    for _ in range(2):
        assert_same(gpu_beam(gm, src, m, BEAM, early_exit=False, max_len=LT.L), ref, early=False)
        seen.append(graph_captures(gm))
    assert seen[0] == 0 and seen[1] >= 1 and seen[2] == seen[1], seen

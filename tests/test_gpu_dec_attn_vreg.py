"""k_dec_attn's value rows loaded straight into the PV chains' registers (csrc/qtx_decode.hip:
vg4[g][q] = the dword of 4-key group 4 g + q, dim = lane; self-attention patches this step's
value byte in registers), against the oracle, bit for bit.

Through qtx_decode_attention (the position from the device counter: the patch selects over
all fragments): self-attention at every step 0 .. 127, cross-attention at every row count at
which the fragment count, the group clamp or the last group's fill change, each with random
values, +-127 values and one-hot value rows (a wrong group, dim or byte then shows in the
context).  The position from the host (the patch in the last fragment) is reachable only
through a decode: a scored greedy decode of the smallest fused config to max_len 36 — every
(step & 3, (step >> 2) & 3) and one to three fragments — against the oracle and under
QTX_GRAPH_STEPS=5 and QTX_NO_GRAPH=1."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import model_cfgs as MC  # noqa: E402
from test_gpu_dec_attn_mfma import _release, caches, run_cross, run_self, torch  # noqa: E402,F401
from test_gpu_scored import gpu_scored, oracle_scored_decode  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
KINDS = ("random", "pm127", "onehot")


def values(rng, kind, B, n, skip=-1):
    """[B, n, 512] value codes.  pm127: every byte +-127.  onehot: one key row per sentence
    (not `skip`, the row a self-attention step overwrites) holds values, every other is 0."""
    v = rng.integers(-127, 128, (B, n, 512)).astype(np.int8)
    if kind == "pm127":
        v = np.where(v < 0, -127, 127).astype(np.int8)
    elif kind == "onehot":
        keep = np.zeros((B, n, 1), bool)
        for b in range(B):
            rows = [j for j in range(n) if j != skip] or [0]
            keep[b, rows[rng.integers(0, len(rows))]] = True
        v = np.where(keep, v, 0).astype(np.int8)
    return v


@pytest.mark.parametrize("step,kv_bs", [(s, 128) for s in range(128)] + [(16, 17), (71, 72)])
def test_self_every_step(torch, step, kv_bs):
    rng = np.random.default_rng(3000 + 7 * step + kv_bs)
    B = 2
    y = rng.standard_normal((B, 1536)).astype(f32)
    for kind in KINDS:
        kc, _, skc, svc = caches(rng, B, kv_bs, 0.0015, 0.003)
        if kind == "pm127":                     # this step's value row at +-127 as well
            y[:, 1024:] = np.where(rng.integers(0, 2, (B, 512)) > 0, 1.0, -1.0)
        run_self(torch, y, kc, values(rng, kind, B, kv_bs, skip=step), skc, svc, step)


@pytest.mark.parametrize("mask_kind", ["suffix", "holes"])
@pytest.mark.parametrize("S", [1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 72, 127, 128])
def test_cross_rows_and_masks(torch, S, mask_kind):
    B = 3
    rng = np.random.default_rng(4000 + S)
    y = rng.standard_normal((B, 512)).astype(f32)
    mask = np.ones((B, S), np.uint8)
    for b in range(B):
        mask[b, rng.integers(1, S + 1):] = 0
    if mask_kind == "holes":
        mask[0, 3:9:2] = 0
        mask[0, S // 2] = 0
        mask[0, 0] = 1
        mask[1, :] = 0                          # fully masked: all S keys, uniform
        mask[2, :] = rng.integers(0, 2, S)
        mask[2, S - 1] = 1
    for kind in KINDS:
        kc, _, skc, svc = caches(rng, B, S, 0.0015, 0.003)
        run_cross(torch, y, kc, values(rng, kind, B, S), skc, svc, mask)


def test_host_position_decode(torch, knob_env):
    """max_len 36: steps 0 .. 34 with the position from the host, the attention inside the
    captured graph; the same under 5-step graphs and launched eagerly."""
    from qtx.model import QtxModel
    cfg, sd, om = MC.small_state(512)
    gm = QtxModel(sd, cfg)
    src, m = MC.small_src(2, 9, 5, full=(1,))
    L = 36
    ys, ti, tv = oracle_scored_decode(om, src, m, L)
    for env in ({}, {"QTX_GRAPH_STEPS": 5}, {"QTX_NO_GRAPH": 1}):
        for k, v in env.items():
            knob_env(k, v)
        gy, gi, gv = gpu_scored(gm, src, m, L)
        np.testing.assert_array_equal(gy, ys, err_msg=str(env))
        np.testing.assert_array_equal(gi, ti, err_msg=str(env))
        np.testing.assert_array_equal(gv, tv, err_msg=str(env))

"""k_dec_attn's scores on the int8 MFMA, the key rows loaded straight into fragment layout
(csrc/qtx_decode.hip; the mapping alone: tests/test_dec_attn_frag_ref.py): through
qtx_decode_attention against the oracle's decoder attention and the expected caches,
bit-exact.  The new key of a self-attention step is patched into the fragment that holds its
row, so every fragment index and column is visited; cross-attention runs every row count at
which the fragment count, the clamped rows or the second key slot change."""
import os
import sys

import numpy as np
import pytest

from oracle import qtx_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_fused import _KEEP, P, S0, _release, call, dev, head_max, torch, vgroup4, vungroup4  # noqa: E402,F401
from test_gpu_model import make_batch  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32

STEPS = [0, 1, 15, 16, 31, 47, 48, 63, 64, 65, 79, 80, 127]


def run_self(torch, y, kc, vc, skc, svc, step):
    """Two calls at the device-counter position `step` (the second re-appends the same
    row); checks the caches, the context and the head maxima against the oracle."""
    B, kv_bs = kc.shape[:2]
    kc, vc, skc, svc = kc.copy(), vc.copy(), skc.copy(), svc.copy()
    kcd, vcd, skd, svd = dev(torch, kc), dev(torch, vgroup4(vc)), dev(torch, skc), dev(torch, svc)
    stepd = dev(torch, np.array([step], np.int32))
    yd = dev(torch, y)
    ctxd = torch.empty((B, 512), dtype=torch.float32, device="cuda")
    pm = torch.empty((8, B), dtype=torch.float32, device="cuda")
    qq, sq = O.quant_rows(y[:, :512])
    qk, sk = O.quant_rows(y[:, 512:1024])
    qv, sv = O.quant_rows(y[:, 1024:])
    kc[:, step], vc[:, step], skc[:, step], svc[:, step] = qk, qv, sk, sv
    n = step + 1
    ctx, _ = O.attention(qq[:, None], sq[:, None], kc[:, :n], skc[:, :n], vc[:, :n],
                         svc[:, :n], np.ones((B, 1, n), np.uint8), dec=True)
    for _ in range(2):
        call("qtx_decode_attention", 1, P(yd), 1536, P(kcd), P(vcd), P(skd), P(svd), kv_bs,
             P(stepd), 0, S0, B, P(ctxd), P(pm), S0)
        np.testing.assert_array_equal(kcd.cpu().numpy(), kc)       # cache append
        np.testing.assert_array_equal(vungroup4(vcd.cpu().numpy(), kv_bs), vc)
        np.testing.assert_array_equal(skd.cpu().numpy(), skc)
        np.testing.assert_array_equal(svd.cpu().numpy(), svc)
        np.testing.assert_array_equal(ctxd.cpu().numpy(), ctx[:, 0])
        np.testing.assert_array_equal(pm.cpu().numpy(), head_max(ctx[:, 0]))


def run_cross(torch, y, kc, vc, skc, svc, mask):
    B, S = kc.shape[:2]
    ctxd = torch.empty((B, 512), dtype=torch.float32, device="cuda")
    pm = torch.empty((8, B), dtype=torch.float32, device="cuda")
    call("qtx_decode_attention", 0, P(dev(torch, y)), 512, P(dev(torch, kc)), P(dev(torch, vgroup4(vc))),
         P(dev(torch, skc)), P(dev(torch, svc)), S, S0, S, P(dev(torch, mask)), B, P(ctxd),
         P(pm), S0)
    qq, sq = O.quant_rows(y)
    ctx, _ = O.attention(qq[:, None], sq[:, None], kc, skc, vc, svc, mask[:, None], dec=True)
    np.testing.assert_array_equal(ctxd.cpu().numpy(), ctx[:, 0])
    np.testing.assert_array_equal(pm.cpu().numpy(), head_max(ctx[:, 0]))


def caches(rng, B, n, lo=0.002, hi=0.03):
    return (rng.integers(-127, 128, (B, n, 512)).astype(np.int8),
            rng.integers(-127, 128, (B, n, 512)).astype(np.int8),
            rng.uniform(lo, hi, (B, n)).astype(f32), rng.uniform(lo, hi, (B, n)).astype(f32))


@pytest.mark.parametrize("step,kv_bs", [(s, 128) for s in STEPS] + [(16, 17), (71, 72)])
def test_self_new_key_in_every_fragment(torch, step, kv_bs):
    rng = np.random.default_rng(7000 + 131 * step + kv_bs)
    y = rng.standard_normal((2, 1536)).astype(f32)
    run_self(torch, y, *caches(rng, 2, kv_bs), step)


@pytest.mark.parametrize("kind", ["suffix", "holes"])
@pytest.mark.parametrize("S", [1, 15, 16, 17, 63, 64, 65, 72, 128])
def test_cross_rows_and_masks(torch, S, kind):
    """suffix: padding masks.  holes: masked keys inside the sentence (row 0), a fully masked
    row (row 1), and a row with holes whose last unmasked key is the last one (row 2: at
    S >= 65 the second key slot is live while key 64 itself may be masked)."""
    B = 3
    rng = np.random.default_rng(9000 + S)
    y = rng.standard_normal((B, 512)).astype(f32)
    mask = np.ones((B, S), np.uint8)
    for b in range(B):
        mask[b, rng.integers(1, S + 1):] = 0
    if kind == "holes":
        mask[0, 3:9:2] = 0
        mask[0, S // 2] = 0
        mask[1, :] = 0
        mask[2, :] = rng.integers(0, 2, S)
        mask[2, S - 1] = 1
        if S > 66:
            mask[2, 64:66] = 0
    run_cross(torch, y, *caches(rng, B, S), mask)


def test_cross_second_slot_after_masked_tail(torch):
    """S = 72, the last unmasked keys 64, 65 and 70: the key loops stop inside the second
    slot's fragment."""
    B, S = 3, 72
    rng = np.random.default_rng(72)
    y = rng.standard_normal((B, 512)).astype(f32)
    mask = np.ones((B, S), np.uint8)
    for b, last in enumerate([64, 65, 70]):
        mask[b, last + 1:] = 0
        mask[b, 60:64] = 0
    run_cross(torch, y, *caches(rng, B, S), mask)


def test_cross_one_hot_rows(torch):
    """Every key row zero except row j, +-127 times the sign of the q code on each head's 64
    bytes, q codes all +-127: |acc| = 64 * 127^2 in key j's lane alone.  The values are
    random, so a permuted key <-> lane map changes the context."""
    B, S = 3, 72
    rng = np.random.default_rng(5)
    y = rng.choice(np.array([-1.0, 1.0], f32), (B, 512))
    qq, sq = O.quant_rows(y)
    assert np.all(np.abs(qq) == 127)
    _, vc, skc, svc = caches(rng, B, S, 0.0015, 0.003)   # scores of +-1.5 .. 3: P spread over keys
    mask = np.ones((B, S), np.uint8)
    mask[2, 70:] = 0
    for j in range(S):
        sign = rng.choice(np.array([-1, 1]), (B, 8)).repeat(64, axis=1)
        kc = np.zeros((B, S, 512), np.int8)
        kc[:, j] = (sign * qq).astype(np.int8)
        acc = np.einsum("bd,bd->b", kc[:, j, :64].astype(np.int64), qq[:, :64].astype(np.int64))
        assert np.all(np.abs(acc) == 64 * 127 * 127)
        run_cross(torch, y, kc, vc, skc, svc, mask)
        _KEEP.clear()      # the device copies of this j


def alternating(B, n, rng):
    """[B, n, 512] codes +-127: row j alternates with period 1, 2 or 4 dims and a phase, so the
    dot products with an alternating q run from -64 * 127^2 over 0 to +64 * 127^2."""
    d = np.arange(512)
    k = np.zeros((B, n, 512), np.int8)
    for b in range(B):
        for j in range(n):
            per, ph = (1, 2, 4)[rng.integers(0, 3)], rng.integers(0, 8)
            k[b, j] = np.where(((d + ph) // per) & 1, -127, 127)
    return k


def test_mixed_sign_extremes_cross(torch):
    B, S = 3, 72
    rng = np.random.default_rng(11)
    y = np.tile(np.array([1.0, -1.0], f32), (B, 256))
    y[1] = -y[1]
    _, vc, skc, svc = caches(rng, B, S, 0.0015, 0.003)
    kc = alternating(B, S, rng)
    qq, _ = O.quant_rows(y)
    acc = np.einsum("bjd,bd->bj", kc[:, :, :64].astype(np.int64), qq[:, :64].astype(np.int64))
    assert acc.min() == -64 * 127 * 127 and acc.max() == 64 * 127 * 127
    run_cross(torch, y, kc, vc, skc, svc, np.ones((B, S), np.uint8))


def test_mixed_sign_extremes_self(torch):
    """The new key alternates too: the patched fragment carries -127 / +127 codes."""
    B, kv_bs, step = 2, 128, 79
    rng = np.random.default_rng(12)
    y = rng.standard_normal((B, 1536)).astype(f32)
    y[:, :1024] = np.tile(np.array([1.0, -1.0], f32), (B, 512))
    y[1, 512:1024] *= -1
    _, vc, skc, svc = caches(rng, B, kv_bs, 0.0015, 0.003)
    run_self(torch, y, alternating(B, kv_bs, rng), vc, skc, svc, step)


def test_greedy_two_sentences_max_len_20(torch, gpu_model, oracle_model):
    """The whole path: the position from the host, the attention inside the captured graph,
    one fragment (steps 0 .. 15) and two (16 ..)."""
    from qtx.decode import greedy_decode
    src, m = make_batch(np.random.default_rng(20), 2, 11)
    ys = greedy_decode(gpu_model, src, m, 20, 0)
    np.testing.assert_array_equal(ys, oracle_model.greedy_decode(src, m, 20))

"""k_attn_mfma_long (csrc/qtx_attn_long.hip): the attention of 129 to 512 keys on the matrix
cores, through qtx_attention_i8, bit for bit against the numpy oracle (no tolerance anywhere).

The kernel and k_attention compute the same bits, so a result alone cannot say which of them
ran: test_route asks the launcher's own selecting function (qtx_debug_attention_kernel).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from oracle import qtx_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import softmax_edges as E  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
S0 = C.c_void_p(0)
VALU, MFMA, MFMA_LONG = "k_attention", "k_attn_mfma", "k_attn_mfma_long"


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def attention_i8(torch, q, sq, k, sk, v, sv, mdev, m_bs, m_is, dec):
    """qtx_attention_i8 of numpy operands (H = 8) -> the context [B, Sq, 512]."""
    from qtx import _lib
    B, Sq, Sk = q.shape[0], q.shape[1], k.shape[1]
    assert _lib.attention_kernel(B, 8, Sq, Sk, dec) == MFMA_LONG
    t = [torch.from_numpy(np.array(a)).cuda() for a in (q, sq, k, sk, v, sv, mdev)]
    ctx = torch.empty((B, Sq, 512), dtype=torch.float32, device="cuda")
    _lib.call("qtx_attention_i8", *(C.c_void_p(x.data_ptr()) for x in t), m_bs, m_is, B, 8, Sq, Sk,
              C.c_void_p(ctx.data_ptr()), dec, S0)
    return ctx.cpu().numpy()


@pytest.mark.parametrize("dec", [0, 1])
@pytest.mark.parametrize("B,Sq,Sk,form", [
    (2, 65, 129, "key"),       # one key in the second block, a second query block of one row
    (1, 130, 257, "causal"),   # three query blocks, NB = 3 with one key
    (2, 16, 385, "full"),      # a mask row per query, one query fully masked; NB = 4, ragged
    (1, 70, 511, "key"), (1, 64, 512, "none"),   # the ragged and the full last tile
    (3, 1, 300, "key")])       # one live row in the workgroup
def test_shapes(torch, B, Sq, Sk, form, dec):
    """Both PV orders and both mask forms, as tests/test_gpu_ops.py test_attention builds them."""
    rng = np.random.default_rng(Sq * 7 + Sk)
    q = rng.integers(-127, 128, (B, Sq, 512)).astype(np.int8)
    k = rng.integers(-127, 128, (B, Sk, 512)).astype(np.int8)
    v = rng.integers(-127, 128, (B, Sk, 512)).astype(np.int8)
    sq, sk, sv = (rng.uniform(0.002, 0.03, (B, n)).astype(f32) for n in (Sq, Sk, Sk))
    mask = np.ones((B, Sq, Sk), np.uint8)
    m_bs, m_is, mdev = Sq * Sk, Sk, mask
    if form == "key":                 # one key mask per sentence (m_is = 0)
        km = np.ones((B, Sk), np.uint8)
        km[0, Sk - Sk // 3:] = 0
        km[-1, 1::7] = 0
        mask[:] = km[:, None, :]
        m_bs, m_is, mdev = Sk, 0, km
    elif form == "causal":
        mask[0] = np.tril(np.ones((Sq, Sk), np.uint8), k=Sk - Sq)
    elif form == "full":
        mask[-1, :, Sk // 2:] = 0
        mask[0] = rng.integers(0, 2, (Sq, Sk))
        mask[0, 5] = 0
    got = attention_i8(torch, q, sq, k, sk, v, sv, mdev, m_bs, m_is, dec)
    np.testing.assert_array_equal(got, O.attention(q, sq, k, sk, v, sv, mask, 8, dec=bool(dec))[0])


@pytest.mark.parametrize("dec", [0, 1])
@pytest.mark.parametrize("S", [129, 511, 512])
def test_every_key_slot(torch, S, dec):
    """Query i keeps key i alone (the identity as the per-query mask): P is 127 / 127 in every
    slot in turn, so context row i is the single product RN(s_v[i] * v[i][d]) in both PV orders
    — a slot that the permutation, a block border or a short PV chain drops or moves shows."""
    rng = np.random.default_rng(8100 + S)
    q, k = (rng.integers(-127, 128, (1, S, 512)).astype(np.int8) for _ in range(2))
    v = rng.integers(1, 128, (1, S, 512)).astype(np.int8) * rng.choice(np.array([-1, 1], np.int8), (1, S, 512))
    sq, sk, sv = (rng.uniform(0.002, 0.03, (1, S)).astype(f32) for _ in range(3))
    got = attention_i8(torch, q, sq, k, sk, v, sv, np.eye(S, dtype=np.uint8)[None], S * S, S, dec)
    np.testing.assert_array_equal(got, (sv[..., None] * v.astype(f32)).astype(f32))


@pytest.mark.parametrize("name", ["cross129", "cross257", "cross511", "cross512", "cross254x", "cross512x",
                                  "cross257_order", "cross512_order"])
def test_ties_and_sum_order(torch, name):
    """tests/softmax_edges.py's decode cross-attention cases past 128 keys as one-query
    attentions (Sq = 1, key mask, dec = 1): the rounding ties of the 1/127 grid, the exact ties,
    and the rows whose denominator feels the order of its sum."""
    raw = E.case(name)["raw"]
    B, S = raw["mask"].shape
    qq, sq = O.quant_rows(raw["y"])
    got = attention_i8(torch, qq[:, None], sq[:, None], raw["kc"], raw["skc"], raw["vc"], raw["svc"],
                       raw["mask"], S, 0, 1)
    np.testing.assert_array_equal(got, E.expected(name, True)[0])


def test_route():
    """The kernel each shape reaches, from the launcher's selecting function."""
    from qtx import _lib
    for Sq in (1, 512):
        for dec in (0, 1):
            assert _lib.attention_kernel(32, 8, Sq, 129, dec) == MFMA_LONG
            assert _lib.attention_kernel(32, 8, Sq, 512, dec) == MFMA_LONG
            assert _lib.attention_kernel(32, 8, Sq, 128, dec) == MFMA
            assert _lib.attention_kernel(32, 8, Sq, 512, dec, device_counts=1) == VALU
            assert _lib.attention_kernel(32, 8, Sq, 128, dec, device_counts=1) == VALU

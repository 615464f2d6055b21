"""The closed forms of tests/long_attn.py on the CPU: what tests/test_gpu_long_fused.py expects
of k_dec_attn_long at every key slot and every step is what O.attention gives."""
import os
import sys

import numpy as np
import pytest

from oracle import qtx_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import long_attn as LA  # noqa: E402

f32 = np.float32
# the edges of the lane rounds, fragments, value groups and wave blocks, and 25 steps between
STEPS = sorted({0, 1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 127, 128, 129, 191, 192, 255, 256, 257,
                383, 384, 510, 511} | set(range(7, 512, 21)))


@pytest.fixture(scope="module")
def es():
    return LA.EveryStep()


def test_one_hot_closed_form():
    """S = 129 (the cheapest of the GPU test's three; the construction is the same for all):
    the codes are one-hot 127 and the context the single product."""
    c = LA.one_hot(129)
    qq, sq = O.quant_rows(c["y"])
    ctx, qp = LA.attention_chunked(qq, sq, c["kc"], c["skc"], c["vc"], c["svc"], c["mask"])
    np.testing.assert_array_equal(qp, np.repeat((127 * np.eye(129, dtype=np.int8))[:, None], 8, 1))
    np.testing.assert_array_equal(ctx, c["ctx"])
    assert np.all(c["ctx"] != 0)


def test_every_step_layout(es):
    assert len(STEPS) >= 40 and {0, 1, 3, 4, 127, 128, 255, 256, 511} <= set(STEPS)
    j = es.j[1:]
    assert np.all(j >= 0) and np.all(j < np.arange(1, 512))
    # the live cached key walks the slots: every wave's block, lane slot, fragment and byte
    assert {(a >> 7, (a >> 6) & 1) for a in j} == {(w, u) for w in range(4) for u in range(2)}
    assert {a & 15 for a in j} == set(range(16)) and {(a >> 4) & 7 for a in j} == set(range(8))
    assert {(a >> 2) & 3 for a in j} == set(range(4)) and len(set(j >> 2)) >= 64   # of 128 value groups
    assert np.all(es.stale_v != 0) and np.all(np.abs(es.stale_k) == 127)


@pytest.mark.parametrize("step", STEPS)
def test_every_step_closed_form(es, step):
    """One live key with P == 127: the context is its value row times its scale, sentence 0's
    the row appended by this step, sentence 1's the one appended at step j(step)."""
    qq, sq, k, sk, v, sv, mask = es.view(step)
    ctx, qp = LA.attention_chunked(qq, sq, k, sk, v, sv, mask)
    live = np.array([step, es.j[step] if step else 0])
    assert (qp.astype(int).sum(-1) == 127).all() and (qp[np.arange(2), :, live] == 127).all()
    np.testing.assert_array_equal(ctx, es.ctx[step])
    assert np.abs(es.ctx[step]).max(-1).min() > 0
    # the rows the test writes ahead of the call give this view's caches below `step`
    kc = np.repeat(es.dead[:, None], step + 1, 1)
    if step:
        kc[0, step - 1] = es.live[0]
        kc[1, es.j[step - 1] if step > 1 else 0] = es.live[1]
    for b, r, codes, _ in es.before(step):
        kc[b, r] = codes
    np.testing.assert_array_equal(kc[:, :step], k[:, :step])
    np.testing.assert_array_equal(kc[:, step], es.stale_k[step])

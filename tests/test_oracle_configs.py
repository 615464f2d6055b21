"""The oracle on the non-default model configs (CPU): the KV-cached decode equals the
reference-shaped full-prefix recompute, and every seed of tests/model_cfgs.py gives a decode
with enough distinct tokens to tell a working KV cache from a stuck one."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import model_cfgs as MC  # noqa: E402


@pytest.mark.parametrize("d_ff", [256, 1536])
def test_oracle_kv_cache_equals_recompute(d_ff):
    _, _, om = MC.small_state(d_ff)
    src, m = MC.small_src(3, 9, 5, full=(0,))
    ys = om.greedy_decode(src, m, 9, kv_cache=True)
    np.testing.assert_array_equal(ys, om.greedy_decode(src, m, 9, kv_cache=False))
    assert MC.distinct_tokens(ys) >= 3, ys


@pytest.mark.parametrize("key", sorted(MC.SEEDS), ids=lambda k: "-".join(map(str, k)))
def test_seed_gives_distinct_tokens(key):
    cfg, sd, om = MC.small_state(*key)
    assert sd["encoder.layers.0.feed_forward.w_1.weight"].shape == (key[0], 512)
    assert om.gen_w.shape[0] == key[2] and om.N == cfg.n_layers
    src, m = MC.small_src(3, 9, 5, full=(0,))
    ys = om.greedy_decode(src, m, 9)
    assert ys.shape == (3, 9) and MC.distinct_tokens(ys) >= 3, ys

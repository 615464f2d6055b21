"""The decode tail folded into layer 0's LN+QKV launch (csrc/qtx_decode.hip
k_skinny_wide_tok, k_generator_mfma's per-strip records; csrc/qtx_api.hip greedy_step_fused):
the decoded ids equal the oracle's and those of the same library with QTX_NO_TAIL_FOLD=1,
exactly, over the shapes and the decisions at which the folded reduction can go wrong.

Models are tiny (one or two layers, d_ff 512, a 64-row positional table, S = 7, max_len
6 - 9); the oracle's decodes are memoized per case.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import model_cfgs as MC  # noqa: E402
import tail_fold_ref as R  # noqa: E402
from test_gpu_scored import oracle_scored_decode  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
S, L = 7, 6
_MEMO = {}


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def memo(key, fn):
    if key not in _MEMO:
        _MEMO[key] = fn()
    return _MEMO[key]


def tiny_state(V, n_layers=1):
    """(cfg, state dict) of a d_ff 512 model with a V-word target vocabulary."""
    def make():
        from qtx.weights import ModelConfig, synthetic_state_dict
        cfg = ModelConfig(src_vocab=64, tgt_vocab=V, n_layers=n_layers, d_ff=512, max_len=64)
        return cfg, synthetic_state_dict(3, cfg, ln_random=True)
    return memo(("sd", V, n_layers), make)


def build(torch, cfg, sd):
    from oracle.qtx_oracle import OracleModel
    from qtx.model import QtxModel
    return QtxModel(sd, cfg), OracleModel(sd, n_layers=cfg.n_layers, n_bits=8)


def gpu_greedy(gm, src, m, max_len):
    from qtx.decode import greedy_decode
    return greedy_decode(gm, src, m, max_len, 0)


def check_fold(gm, knob_env, src, m, max_len, ref):
    """folded == oracle == unfolded, exactly."""
    np.testing.assert_array_equal(gpu_greedy(gm, src, m, max_len), ref)
    knob_env("QTX_NO_TAIL_FOLD", 1)
    np.testing.assert_array_equal(gpu_greedy(gm, src, m, max_len), ref)


# =====================================================================================
# 1. shapes
# =====================================================================================
@pytest.fixture(scope="module")
def model97(torch):
    """Vocabulary 97: 7 strips, the last one ragged (one valid column); two layers."""
    cfg, sd = tiny_state(97, 2)
    yield build(torch, cfg, sd)


@pytest.mark.parametrize("B", [1, 3, 5, 33, 97])
def test_fold_batch_sizes(torch, model97, knob_env, B):
    """B = 1, 3, 5: a ragged 4-row block; 33: two 16-row generator blocks and a ragged third;
    97: the 8-row instances (two rows per wave), the last block ragged.  This model has two
    layers, d_ff 512 and 97 words; tests/test_gpu_wide_batch.py decodes 97 and 193 rows on the
    default model (4444 words, the d_ff 2048 FFN2)."""
    gm, om = model97
    src, m = MC.small_src(B, S, 11 + B, full=(0,))
    ref = memo(("b", B), lambda: om.greedy_decode(src, m, L))
    assert MC.distinct_tokens(ref) >= 2, ref      # (a stuck tail would repeat one token)
    check_fold(gm, knob_env, src, m, L, ref)


def test_fold_vocab_4444(torch, gpu_model, oracle_model, knob_env):
    """The default model (6 layers, d_ff 2048, 278 strips: five records per lane, the last
    strip ragged), two steps: step 1 starts with the folded launch."""
    rng = np.random.default_rng(41)
    src = np.full((3, 8), 2, np.int64)
    for b, n in enumerate((8, 6, 5)):
        src[b, 0], src[b, n - 1] = 0, 1
        src[b, 1:n - 1] = rng.integers(4, 5337, n - 2)
    m = (src != 2)[:, None, :]
    ref = memo("v4444", lambda: oracle_model.greedy_decode(src, m, 3))
    check_fold(gpu_model, knob_env, src, m, 3, ref)


def test_fold_vocab_8192(torch, knob_env):
    """The cap of the fused tail: 512 strips, eight records per lane."""
    cfg, sd = tiny_state(8192)
    gm, om = build(torch, cfg, sd)
    src, m = MC.small_src(3, S, 5, full=(0,))
    ref = om.greedy_decode(src, m, L)
    assert MC.distinct_tokens(ref) >= 2, ref
    check_fold(gm, knob_env, src, m, L, ref)


def test_vocab_8200_decodes_unfused(torch, knob_env):
    """Above the cap the decode takes the unfused step, with or without the switch."""
    cfg, sd, om = MC.small_state(512, 8, 8200)
    from qtx.model import QtxModel
    gm = QtxModel(sd, cfg)
    src, m = MC.small_src(3, S, 5, full=(0,))
    check_fold(gm, knob_env, src, m, L, om.greedy_decode(src, m, L))


# =====================================================================================
# 2. decisions, through the real generator (crafted weight and bias)
# =====================================================================================
J1, J2 = 5, 70     # two vocabulary rows in different strips


def craft(kind):
    cfg, sd = tiny_state(97)
    sd = dict(sd)
    W = sd["generator.proj.weight"].copy()
    b = sd["generator.proj.bias"].copy()
    if kind == "tie":                  # two identical rows hold the maximum
        W[J2] = W[J1]
        b[J1] = b[J2] = 8.0
    elif kind == "near_tie":           # the later row leads by 2 ulp of the bias
        W[J2] = W[J1]
        b[J1] = 8.0
        b[J2] = np.nextafter(np.nextafter(f32(8.0), f32(9)), f32(9))
    elif kind == "nonfinite":
        b[J1] = np.inf
        b[J2] = np.nan
    elif kind == "all_equal":
        W[:] = 0
        b[:] = 0
    elif kind == "last_column":        # the one valid column of the ragged strip
        b[96] = 8.0
    sd["generator.proj.weight"], sd["generator.proj.bias"] = W, b
    return cfg, sd


@pytest.mark.parametrize("kind", ["tie", "near_tie", "nonfinite", "all_equal", "last_column"])
def test_fold_decisions(torch, knob_env, kind):
    cfg, sd = craft(kind)
    gm, om = build(torch, cfg, sd)
    src, m = MC.small_src(3, S, 9, full=(0,))
    ref, ti, tv = oracle_scored_decode(om, src, m, L)
    np.testing.assert_array_equal(ref, om.greedy_decode(src, m, L))
    # the oracle on the CPU first: the case is what it claims to be
    if kind in ("tie", "near_tie"):    # the exact path ran: the top-2 gap is below 4e-6
        gap = tv[..., 0] - tv[..., 1]
        assert (gap < 4e-6).any(), gap
        assert set(np.unique(ref[:, 1:])) <= {J1, J2}
        if kind == "tie":
            assert (gap == 0).all() and (ref[:, 1:] == J1).all()      # the first index wins
    elif kind in ("nonfinite", "all_equal"):
        assert (ref[:, 1:] == 0).all()
    else:
        assert (ref[:, 1:] == 96).all()
    check_fold(gm, knob_env, src, m, L, ref)


# =====================================================================================
# 3. the generator launch: logits do not depend on the records; the records themselves
# =====================================================================================
def run_generator(torch, gm, x, V, with_rec):
    from qtx import _lib
    M = x.shape[0]
    nstrip = (V + 15) // 16
    P = lambda t: C.c_void_p(t.data_ptr())
    xd = torch.from_numpy(x).cuda()
    logits = torch.full((M + 1, V), -7.0, dtype=torch.float32, device="cuda")
    rec = torch.full((M + 1, nstrip, 4), -7.0, dtype=torch.float32, device="cuda")
    _lib.call("qtx_decode_generator", gm.handle, P(xd), M, P(logits), P(rec) if with_rec else None,
              C.c_void_p(0))
    torch.cuda.synchronize()
    lg, rc = logits.cpu().numpy(), rec.cpu().numpy()
    assert (lg[M] == -7.0).all() and (rc[M] == -7.0).all()             # nothing past row M - 1
    if not with_rec:
        assert (rc == -7.0).all()
    return lg[:M], rc[:M]


@pytest.mark.parametrize("M", [1, 5, 16, 17, 33])
@pytest.mark.parametrize("V", [97, 4444])
def test_generator_records(torch, request, V, M):
    if V == 97:
        gm = request.getfixturevalue("model97")[0]
    else:
        gm = request.getfixturevalue("gpu_model")
    x = (np.random.default_rng(100 * V + M).standard_normal((M, 512)) * 3).astype(f32)
    off, _ = run_generator(torch, gm, x, V, False)
    on, rec = run_generator(torch, gm, x, V, True)
    assert off.tobytes() == on.tobytes()
    ri = rec.view(np.int32)
    for r in range(M):
        want = R.strip_records(on[r])
        got = [(rec[r, s, 0], rec[r, s, 1], int(ri[r, s, 2]), int(ri[r, s, 3]))
               for s in range(len(want))]
        assert got == want, r

"""tools/enctrials_ab.py draws its 32 trials with fault.random_fault(.., rows=S) and
fault.random_attn_fault(.., B=1, Sq=S, Sk=S): every draw must lie in the coordinates
qtx_greedy_decode_enctrials accepts for one sentence (include/qtx_enctrials.h), and the set must
hold encoder linears, encoder attention targets and both memory K/V projections (CPU)."""
import importlib.util
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("enctrials_ab",
                                                  os.path.join(REPO, "tools", "enctrials_ab.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_draws_are_one_sentence_trials():
    from qtx.fault import linear_shape
    S, H = 72, 8
    faults = _tool().draw_faults(np.random.default_rng(20241223), 32, S)
    assert len(faults) == 32
    lins = {f.linear for f in faults}
    assert {"CK", "CV", "QK", "PV"} <= lins and lins & {"Q", "K", "V", "O", "FFN1", "FFN2"}
    assert {f.kind for f in faults} >= {"INPUT", "WEIGHT", "INPUT16", "WEIGHT16", "RANDOM"}
    for f in faults:
        assert 0 <= f.layer < 6 and 0 <= f.bit <= 7
        assert f.module == (1 if f.linear in ("CK", "CV") else 0)
        inp, wgt = f.kind in ("INPUT", "INPUT16"), f.kind in ("WEIGHT", "WEIGHT16")
        if f.linear in ("QK", "PV"):
            qk = f.linear == "QK"
            rows = S                                      # B = 1: Sq = Sk = S rows either way
            cols = H * 64 if (wgt or (inp and qk)) else H * S
            wmax = S if wgt else (S if qk else 64)
        else:
            N, K = linear_shape(f.linear)
            rows = N if wgt else S
            cols = N if f.kind == "RANDOM" else K
            wmax = S if wgt else N
        assert 0 <= f.row < rows and 0 <= f.col < cols, f
        if f.kind in ("INPUT16", "WEIGHT16"):
            assert 1 <= f.win_len <= 16 and 0 <= f.win_start and f.win_start + f.win_len <= wmax, f
        if f.kind == "RANDOM":
            assert np.isfinite(f.value)

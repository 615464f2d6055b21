"""The model and references of the beam decode past 128 positions on the fused step
(tests/test_beam_long_ref.py on the CPU, tests/test_gpu_beam_long.py on the GPU): a helper
module, not a conftest.

The model is long_target's (2 layers, 64 / 97 words, 192-row positional table) with d_ff 2048
and seed 1, picked on the CPU: with beam 3 and max_len 140 sentence 0's final hypotheses 1 and 2
descend through a slot whose parent at step 129 is another slot (long_target.beam_late_moves),
which the d_ff 512 model of the regime never does.  A reference decode takes about half a
minute, so each is computed once per process and never changed."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_ref as BR  # noqa: E402
import long_target as LT  # noqa: E402

CFG, SEED, BEAM = (2048, 8), 1, 3


def state():
    """(cfg, state dict, OracleModel), built once."""
    def run():
        from oracle.qtx_oracle import OracleModel
        from qtx.weights import ModelConfig, synthetic_state_dict
        cfg = ModelConfig(src_vocab=64, tgt_vocab=97, n_layers=2, d_ff=CFG[0], max_len=LT.PE_ROWS,
                          weight_bits=CFG[1])
        sd = synthetic_state_dict(SEED, cfg, ln_random=True)
        return cfg, sd, OracleModel(sd, n_layers=cfg.n_layers, n_bits=CFG[1])
    return LT.memo(("beam_long_state",), run)


def inputs(long_src=False, rows=None):
    src, m = LT.long_inputs() if long_src else LT.inputs()
    return (src, m) if rows is None else (src[list(rows)], m[list(rows)])


def reference(max_len=LT.L, long_src=False, rows=None):
    """beam_ref at beam 3 of the sources (rows: a subset of the sentences)."""
    def run():
        src, m = inputs(long_src, rows)
        return BR.beam_ref(state()[2], src, m, max_len, BEAM)
    return LT.memo(("beam_long", max_len, long_src, rows), run)

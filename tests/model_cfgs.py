"""Small models of every config qtx_model_create accepts, shared by
tests/test_gpu_model_configs.py (GPU) and tests/test_oracle_configs.py (CPU).

Two layers, a 64 / 97-word vocabulary (97: no multiple of 16 or 64, the generator's and the
argmax tail's tile widths) and a 64-row positional table keep a model at a few MB and an
oracle decode under a second.  The seeds were picked on the CPU so that the oracle's greedy
decode of small_src(B = 3, S = 9) holds at least three distinct tokens after the start
symbol in some sentence (a decode that repeats one token would pass with a stuck KV cache):
tests/test_oracle_configs.py asserts it for every entry.
"""
import numpy as np

D_FFS = (256, 512, 768, 1024, 1280, 1536, 1792, 2048)
# (d_ff, weight_bits, tgt_vocab) -> synthetic_state_dict seed
SEEDS = {(256, 8, 97): 1, (512, 8, 97): 1, (768, 8, 97): 1, (1024, 8, 97): 1,
         (1280, 8, 97): 1, (1536, 8, 97): 1, (1792, 8, 97): 1, (2048, 8, 97): 1,
         (256, 4, 97): 1, (512, 4, 97): 1, (1024, 4, 97): 1, (512, 8, 8200): 1}
_CACHE = {}


def small_cfg(d_ff, weight_bits=8, tgt_vocab=97):
    from qtx.weights import ModelConfig
    return ModelConfig(src_vocab=64, tgt_vocab=tgt_vocab, n_layers=1 if tgt_vocab > 97 else 2,
                       d_ff=d_ff, max_len=64, weight_bits=weight_bits)


def small_state(d_ff, weight_bits=8, tgt_vocab=97):
    """(cfg, state dict, OracleModel) of one config, built once per process."""
    key = (d_ff, weight_bits, tgt_vocab)
    if key not in _CACHE:
        from oracle.qtx_oracle import OracleModel
        from qtx.weights import synthetic_state_dict
        cfg = small_cfg(*key)
        sd = synthetic_state_dict(SEEDS[key], cfg, ln_random=True)
        _CACHE[key] = (cfg, sd, OracleModel(sd, n_layers=cfg.n_layers, n_bits=weight_bits))
    return _CACHE[key]


def small_src(B, S, seed, vocab=64, full=()):
    """Source ids below `vocab` with ragged padding (BOS .. EOS PAD*); the sentences in
    `full` span all S tokens.  Returns (src int64 [B,S], src_mask bool [B,1,S])."""
    rng = np.random.default_rng(seed)
    src = np.full((B, S), 2, np.int64)
    for b in range(B):
        n = S if b in full else int(rng.integers(4, S))
        src[b, 0], src[b, n - 1] = 0, 1
        src[b, 1:n - 1] = rng.integers(4, vocab, n - 2)
    return src, (src != 2)[:, None, :]


def distinct_tokens(ys):
    """The largest number of distinct tokens after the start symbol in one sentence."""
    return max(len(set(row[1:].tolist())) for row in np.asarray(ys))

"""Models, inputs and memoised oracle results of the long-target regime: 129 to 512 decoder
positions.  Shared by tests/test_long_target_ref.py (CPU: the guards) and
tests/test_gpu_long_target.py (GPU == the oracle, bit for bit); a helper module, not a conftest.

Above 128 target positions the library leaves the code every other test runs: the decode takes
the unfused step whose self-attention reads its key count from the device counter (the generic
k_attention), the full-prefix passes run k_attention under a [T, T] mask over more than one
128-row tile, the beam reorder moves ungrouped V caches, and the attention fault kernels run past
128 keys.

The models are built like those of tests/model_cfgs.py (2 layers, 64 / 97 words; for d_ff 512
and 1024 the same seed, so the same weights) with a 192-row positional table, and one d_ff = 512
model with a 512-row table for the cap T = 512.  The decodes run to L = 140, so the self-attention's keys run to 139: past the 128
switch, two full 64-lane rounds plus a ragged 11.  SEEDS were picked on the CPU so that the
oracle's decode holds at least three distinct tokens at the positions 129 and up in some
sentence (tests/test_long_target_ref.py asserts it, and what every fault, upset and beam case
below must change).

An oracle decode of L = 140 takes about five seconds and a T = 139 full pass about two, so every
result is computed once per process (memo) and never changed by its users.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_ref as BR  # noqa: E402
import kvfault_ref as KR  # noqa: E402
import model_cfgs as MC  # noqa: E402
import score_ref as SR  # noqa: E402

L = 140                      # max_len of every decode: keys 0 .. 139
B, S = 2, 9
T_FULL = L - 1               # the teacher-forced pass over a decode's prefix: 139 positions
PE_ROWS, CAP_ROWS = 192, 512
LONG_S, LONG_LENS, LONG_T = 132, (132, 70), 130
# (d_ff, weight_bits): fused-capable but unfused by length; the row chain; the generic k_gemm
# chain; int4
CONFIGS = [(512, 8), (1024, 8), (256, 8), (512, 4)]
SEEDS = {(512, 8): 1, (1024, 8): 1, (256, 8): 4, (512, 4): 2}
# The model of the dfault / kvfault cases.  Its seed was picked so that sentence 1's two best
# tokens lie 0.006 apart at step 133: one flipped bit of one key's code (the QK WEIGHT fault on
# key 130) moves a score by a fraction of a unit, which changes a token only at a near-tie.
FAULT_CFG = (256, 8)
_STATE, _MEMO = {}, {}


def memo(key, fn):
    if key not in _MEMO:
        _MEMO[key] = fn()
    return _MEMO[key]


def cfg_id(c):
    return "dff%d_w%d" % c


def state(d_ff, weight_bits=8, pe_rows=PE_ROWS):
    """(cfg, state dict, OracleModel) with a pe_rows-row positional table, built once.  The
    weights are model_cfgs.small_state's for the same seed (the table draws no random number)."""
    key = (d_ff, weight_bits, pe_rows)
    if key not in _STATE:
        from oracle.qtx_oracle import OracleModel
        from qtx.weights import ModelConfig, synthetic_state_dict
        cfg = ModelConfig(src_vocab=64, tgt_vocab=97, n_layers=2, d_ff=d_ff, max_len=pe_rows,
                          weight_bits=weight_bits)
        sd = synthetic_state_dict(SEEDS[(d_ff, weight_bits)], cfg, ln_random=True)
        _STATE[key] = (cfg, sd, OracleModel(sd, n_layers=cfg.n_layers, n_bits=weight_bits))
    return _STATE[key]


def inputs():
    """(src [2, 9], mask): sentence 0 spans all 9 tokens, sentence 1 is padded."""
    return MC.small_src(B, S, 5, full=(0,))


def long_inputs():
    """(src [2, 132], mask), lengths 132 and 70: cross-attention past 128 keys."""
    from dfault_cases import make_src
    return make_src(seed=77, vocab=64, b=2, s=LONG_S, lens=LONG_LENS)


# ---- the cached decode ---------------------------------------------------------------------
def scored(c):
    """The oracle's scored KV-cached decode of inputs() to L: (ys [2, 140], top_ids, top_logp
    [2, 139, 2])."""
    def run():
        from test_gpu_scored import oracle_scored_decode
        src, m = inputs()
        return oracle_scored_decode(state(*c)[2], src, m, L)
    return memo(("scored", c), run)


def tail_distinct(ys, first=129):
    """The largest number of distinct tokens one sentence holds at the positions first .. ."""
    return max(len(set(row[first:].tolist())) for row in np.asarray(ys))


# ---- full-prefix passes --------------------------------------------------------------------
def memory_of(c, long_src=False, pe_rows=PE_ROWS):
    def run():
        om = state(*c, pe_rows)[2]
        src, m = long_inputs() if long_src else inputs()
        return om.encode(om.embed(src, om.src_lut), m)
    return memo(("memory", c, long_src, pe_rows), run)


def pad_mask(T=T_FULL):
    """A batched [2, T, T] target mask: causal AND a key pattern with holes below and above
    position 128 (sentence 0: keys 5, 64, 127, 130 .. 132 dropped; sentence 1: every seventh key
    from 3 and key 128), and query row 133 of sentence 1 fully masked."""
    keep = np.ones((B, T), bool)
    keep[0, [5, 64, 127, 130, 131, 132]] = False
    keep[1, 3::7] = False
    keep[1, 128] = False
    tm = (keep[:, None, :] & (np.tril(np.ones((T, T), np.int64)) != 0)[None]).astype(np.uint8)
    tm[1, 133, :] = 0
    return tm


def full_pass(c, kind="causal"):
    """One teacher-forced decoder pass: dict(y, memory, src_mask, tgt_mask, out).
      causal  (2, 139, 9): the embedded prefix ys[:, :139] of scored(c), the shared causal mask
      padded  the same input under pad_mask()
      long    (2, 130, 132): seeded target ids on the long source's memory, causal mask
      cap     (1, 512, 9): the 512-row-table model, sentence 0, seeded target ids"""
    def run():
        rows = CAP_ROWS if kind == "cap" else PE_ROWS
        om = state(*c, rows)[2]
        _, m = long_inputs() if kind == "long" else inputs()
        memory = memory_of(c, kind == "long", rows)
        if kind in ("causal", "padded"):
            ys = scored(c)[0][:, :T_FULL]
        else:
            T = CAP_ROWS if kind == "cap" else LONG_T
            ys = np.random.default_rng(T).integers(4, 97, (B, T))
            ys[:, 0] = 0
        if kind == "cap":
            ys, m, memory = ys[:1], m[:1], memory[:1]
        T = ys.shape[1]
        tm = pad_mask(T) if kind == "padded" else np.tril(np.ones((1, T, T), np.uint8))
        y = om.embed(ys, om.tgt_lut)
        return dict(y=y, memory=memory, src_mask=m, tgt_mask=tm, out=om.decode(y, memory, m, tm))
    return memo(("full", c, kind), run)


def full_pass_tokens(c):
    """The first-index argmax of the generator on every position of full_pass(c): [2, 139]."""
    def run():
        om = state(*c)[2]
        out = full_pass(c)["out"]
        return om.generator(out.reshape(-1, out.shape[-1]))[1].reshape(out.shape[:2])
    return memo(("full_tokens", c), run)


# ---- target scoring ------------------------------------------------------------------------
def score_golden(c):
    """score_ref of the decode's own ids (the causal mask alone)."""
    def run():
        src, m = inputs()
        return SR.score_ref(state(*c)[2], src, m, scored(c)[0], pad=-1)
    return memo(("score", c), run)


PAD_AT = (131, 137)          # where score_padded() plants the pad token: labels past 128


def score_padded(c):
    """(tgt, score_ref with pad = 2): the decode's ids with the pad token at PAD_AT of sentence
    1, so the pad-aware mask drops keys above position 128 for every later query."""
    def run():
        src, m = inputs()
        tgt = scored(c)[0].copy()
        tgt[1, list(PAD_AT)] = SR.PAD
        return tgt, SR.score_ref(state(*c)[2], src, m, tgt, pad=SR.PAD)
    return memo(("score_pad", c), run)


# ---- decoder faults at fault_step 133 (the faulty full-prefix pass runs at T = 134) -----------
DF_STEP = 133
DF_T = DF_STEP + 1


def dfault_trials():
    """name -> Fault; rows index the faulty pass's [B * 134] tokens, all on sentence 1.  A
    linear target on the last position; a QK WEIGHT fault on key j = 130 (every query row that
    sees it); a PV INPUT fault on the last query at column h * Sk + 131."""
    from qtx.fault import Fault
    T = DF_T
    return {
        "output_ffn2": Fault("OUTPUT", 1, 1, "FFN2", row=1 * T + T - 1, col=7, value=3.0e4),
        "weight_qk_j130": Fault("WEIGHT", 1, 1, "QK", row=1 * T + 130, col=2 * 64 + 28, bit=7),
        "input_pv_j131": Fault("INPUT", 1, 1, "PV", row=1 * T + T - 1, col=1 * T + 131, bit=6),
    }


def kv_golden(c=FAULT_CFG):
    """kvfault_ref.golden of inputs() to L: the cached decode with the state before each step."""
    src, m = inputs()
    return KR.golden(state(*c)[2], src, m, L, "long" + cfg_id(c))


def dfault_trial(name, c=FAULT_CFG):
    """(ys, top_ids, top_logp, record) of one dfault trial, as dfault_cases.oracle_trial gives
    it, from a cached golden decode plus ONE faulty full-prefix pass: the golden steps are the
    cached decode's (by causal invariance the full-prefix loop's, which test_long_target_ref.py
    checks at T = 139), the faulty step is oracle decode(fault=) on the golden prefix, and the
    steps after a changed token run KV-cached from the golden state before step 134 (the faulty
    pass leaves the caches alone)."""
    def run():
        from dfault_cases import _step
        om = state(*c)[2]
        src, m = inputs()
        g = kv_golden(c)
        gy, gi, gv = g["ys"], g["top_ids"], g["top_logp"]
        i2, v2, nxt = _step(om, gy[:, :DF_T], g["memory"], m, fault=dfault_trials()[name].as_dict())
        rec = (gi[:, DF_STEP], gv[:, DF_STEP], i2, v2)
        ti, tv, ys = gi.copy(), gv.copy(), gy.copy()
        ti[:, DF_STEP], tv[:, DF_STEP] = i2, v2
        if not np.array_equal(nxt, gy[:, DF_T]):
            ys0 = np.concatenate([gy[:, :DF_T], nxt[:, None]], axis=1)
            ys, i3, v3 = KR._run(om, KR.clone(g["snaps"][DF_T]), ys0, DF_T, L - 1)
            ti[:, DF_T:], tv[:, DF_T:] = np.stack(i3, 1), np.stack(v3, 1)
        return ys, ti, tv, rec
    return memo(("dfault", c, name), run)


# ---- faults of the cached decode itself ------------------------------------------------------
def kvfault_cases():
    """name -> (Fault or None, CacheUpset or None, step).  Step faults index the step's [B]
    rows and its step + 1 self keys."""
    from qtx.fault import CacheUpset as U
    from qtx.fault import Fault as F
    return {
        # the K row of position 131 in the lowest layer, sentence 1: every later step reads it
        "out_k_s131": (F("OUTPUT", 1, 0, "K", row=1, col=7, value=50.0), None, 131),
        # a stored K code of position 129, sentence 1, flipped before step 133
        "up_sk_j129": (None, U("self_k", 0, row=1 * L + 129, col=2 * 64 + 33, bit=7), 133),
        # the sign of a stored V scale at position 129, sentence 0
        "up_sv_scale_j129": (None, U("self_v", 0, row=0 * L + 129, bit=31, field="scale"), 137),
        # the step's own attention at Sk = 134: the probability code of key 131, head 0,
        # sentence 1
        "in_pv_j131": (F("INPUT", 1, 0, "PV", row=1, col=0 * 134 + 131, bit=6), None, 133),
        # and the score of key 128, head 1
        "rand_qk_j128": (F("RANDOM", 1, 0, "QK", row=1, col=1 * 134 + 128, value=1.0e4), None, 133),
    }


def kvfault_trial(name, c=FAULT_CFG):
    f, u, step = kvfault_cases()[name]
    src, m = inputs()
    return KR.trial(state(*c)[2], src, m, L, "long" + cfg_id(c), f, u, step)


def kvfault_effect(name, c=FAULT_CFG):
    src, m = inputs()
    return KR.effect(state(*c)[2], src, m, L, "long" + cfg_id(c), kvfault_trial(name, c))


# ---- beam ------------------------------------------------------------------------------------
BEAM = 3
# beam_ref's EOS boost is dropped: with it every hypothesis ends long before position 128;
# without it the search runs all 139 steps and still reorders at most of them
BEAM_CONFIGS = [(512, 8), (1024, 8)]


def beam_reference(c):
    def run():
        src, m = inputs()
        return BR.beam_ref(state(*c)[2], src, m, L, BEAM)
    return memo(("beam", c), run)


def beam_late_moves(ref, first=129):
    """(sentence, final slot, step) of every cache move that a final hypothesis descends
    through at a step >= first and that a later step still reads: the slot's parent at that
    step is another slot, so k_beam_reorder gave it that slot's K/V rows, and its next step
    attended over them."""
    par = np.stack(ref["parents"])
    n, out = len(par), []
    for b in range(par.shape[1]):
        for k in range(par.shape[2]):
            slot = k
            for s in range(n - 1, -1, -1):
                p = int(par[s, b, slot])
                if p != slot and first <= s <= n - 2:
                    out.append((b, k, s))
                slot = p
    return out

"""Inputs, trials and oracle expectations shared by tests/test_gpu_dfault_cached.py (a helper
module, not a conftest).

Expected values never come from the code under test.  oracle_trial() follows the campaign
loop (parallelized_inject_onnx_transformer.py:536-740) on the oracle: every step is a
full-prefix oracle_model.decode + generator, the step target_inference_number - 1 with the
fault, and the top 2 of a step are the two best entries of its oracle logp row under a stable
descending sort (the first-index rule).  The ids are checked against
oracle_model.greedy_decode(fault=, fault_step=).  Golden steps are computed once per input and
shared; once a faulty step leaves every token as the golden decode's, the remaining steps are
the golden ones (same inputs, same deterministic oracle).
"""
import numpy as np

f32 = np.float32
B, S, L = 3, 14, 8
LENS = (14, 9, 12)
_MEMO = {}


def memo(key, fn):
    if key not in _MEMO:
        _MEMO[key] = fn()
    return _MEMO[key]


def top2_of(logp):
    logp = np.asarray(logp, f32)
    order = np.argsort(-logp, axis=-1, kind="stable")[:, :2].astype(np.int64)
    return order, np.take_along_axis(logp, order, axis=-1)


def make_src(seed=141, vocab=5337, b=B, s=S, lens=LENS):
    rng = np.random.default_rng(seed)
    src = np.full((b, s), 2, np.int64)          # PAD
    for i, n in enumerate(lens):
        src[i, 0] = 0
        src[i, 1:n - 1] = rng.integers(4, vocab, n - 2)
        src[i, n - 1] = 1
    return src, (src != 2)[:, None, :]


def _step(om, ys, memory, m, fault=None):
    T = ys.shape[1]
    out = om.decode(om.embed(ys, om.tgt_lut), memory, m, np.tril(np.ones((1, T, T), np.int64)),
                    fault=fault)
    logp, nxt = om.generator(out[:, -1])
    i2, v2 = top2_of(logp)
    assert np.array_equal(i2[:, 0], nxt)
    return i2, v2, nxt


def oracle_golden(om, src, m, max_len, tag):
    """The golden decode, every step a full-prefix pass: (memory, ys, top_ids, top_logp)."""
    def run():
        memory = om.encode(om.embed(src, om.src_lut), m)
        ys = np.zeros((src.shape[0], 1), np.int64)
        ti, tv = [], []
        for _ in range(max_len - 1):
            i2, v2, nxt = _step(om, ys, memory, m)
            ti.append(i2)
            tv.append(v2)
            ys = np.concatenate([ys, nxt[:, None]], axis=1)
        return memory, ys, np.stack(ti, 1), np.stack(tv, 1)
    return memo(("gold", tag, max_len), run)


def oracle_trial(om, src, m, max_len, fault, tin, tag):
    """(ys, top_ids, top_logp, record) of one campaign trial; record = (golden ids, golden
    logp, faulty ids, faulty logp) [B, 2] each, or None when the loop never reaches tin."""
    def run():
        memory, gy, gi, gv = oracle_golden(om, src, m, max_len, tag)
        step = tin - 1
        if not 0 <= step < max_len - 1:
            return gy, gi, gv, None
        fd = fault.as_dict()
        i2, v2, nxt = _step(om, gy[:, :step + 1], memory, m, fault=fd)
        rec = (gi[:, step], gv[:, step], i2, v2)
        ti, tv = gi.copy(), gv.copy()
        ti[:, step], tv[:, step] = i2, v2
        ys = gy.copy()
        if not np.array_equal(nxt, gy[:, step + 1]):
            ys = np.concatenate([gy[:, :step + 1], nxt[:, None]], axis=1)
            for t in range(step + 1, max_len - 1):
                i2, v2, nxt = _step(om, ys, memory, m)
                ti[:, t], tv[:, t] = i2, v2
                ys = np.concatenate([ys, nxt[:, None]], axis=1)
        np.testing.assert_array_equal(
            ys, om.greedy_decode(src, m, max_len=max_len, fault=fd, fault_step=step))
        return ys, ti, tv, rec
    return memo(("trial", tag, max_len, repr(fault), tin), run)


def changed(exp):
    """Whether the trial's fault changed a token (in the oracle's result)."""
    return exp[3] is not None and bool((exp[3][0][:, 0] != exp[3][2][:, 0]).any())


def trials():
    """name -> (Fault, target_inference_number) for B = 3 sentences, max_len = 8.  Rows index
    the faulty step's [B * T] tokens, T = target_inference_number (memory K/V: [B * S])."""
    from qtx.fault import Fault
    return {
        # INPUT on FFN1: sentence 1's last position at T = 3
        "input_ffn1": (Fault("INPUT", 1, 2, "FFN1", row=1 * 3 + 2, col=100, bit=6), 3),
        # the same element, bit 0: masked
        "input_ffn1_bit0": (Fault("INPUT", 1, 2, "FFN1", row=1 * 3 + 2, col=100, bit=0), 3),
        "input_bit0_t2": (Fault("INPUT", 1, 2, "FFN1", row=1 * 2 + 1, col=100, bit=0), 2),
        # WEIGHT on O: every row
        "weight_o": (Fault("WEIGHT", 1, 3, "O", row=77, col=300, bit=6), 2),
        # WEIGHT on FFN2 of the last layer (every row) at step 2, where sentence 2's two best
        # tokens lie 7e-5 apart in the golden decode: a single weight bit changes the token
        "weight_ffn2": (Fault("WEIGHT", 1, 5, "FFN2", row=404, col=207, bit=6), 3),
        # WEIGHT16 on the memory V projection: memory rows 16 .. 25 of [B * S]
        "weight16_cv": (Fault("WEIGHT16", 1, 1, "CV", row=40, col=200, bit=6, win_start=16,
                              win_len=10), 4),
        # RANDOM on QK^T: sentence 2, query 4, head 3, key 2 at T = 5
        "random_qk": (Fault("RANDOM", 1, 0, "QK", row=2 * 5 + 4, col=3 * 5 + 2, value=1.0e4), 5),
        # INPUT on self-attention PV: sentence 0, query 5, head 1, key 3 at T = 6
        "input_pv": (Fault("INPUT", 1, 4, "PV", row=0 * 6 + 5, col=1 * 6 + 3, bit=5), 6),
        # OUTPUT on the last layer's FFN2 at sentence 0's last position: the token changes
        "output_ffn2": (Fault("OUTPUT", 1, 5, "FFN2", row=0 * 3 + 2, col=100, value=3.0e4), 3),
        "output_ffn2_t2": (Fault("OUTPUT", 1, 5, "FFN2", row=0 * 2 + 1, col=100, value=3.0e4), 2),
        "output_ffn2_late": (Fault("OUTPUT", 1, 5, "FFN2", row=2 * 6 + 5, col=100, value=3.0e4), 6),
        # INPUT at position 0 of sentence 2 while fault_step = 3: an earlier row of the prefix
        "input_v_pos0": (Fault("INPUT", 1, 0, "V", row=2 * 4 + 0, col=50, bit=6), 4),
        # the first step (T = 1) and the last one (no continuation)
        "first_step": (Fault("WEIGHT", 1, 0, "FFN1", row=10, col=20, bit=6), 1),
        "last_step": (Fault("INPUT", 1, 5, "FFN2", row=2 * 7 + 6, col=1000, bit=6), L - 1),
        # never applied: the loop ends before this inference number
        "never_8": (Fault("INPUT", 1, 2, "FFN1", row=0, col=100, bit=6), L),
        "never_11": (Fault("WEIGHT", 1, 3, "O", row=77, col=300, bit=6), L + 3),
    }


# target_inference_numbers 1, 2, 2, 4, 6, 7 and two never applied: a masked one (bit 0) and
# token changers at an earlier and a later step
SWEEP = ("first_step", "output_ffn2_t2", "input_bit0_t2", "weight16_cv", "output_ffn2_late",
         "last_step", "never_8", "never_11")

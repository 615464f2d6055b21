"""The reference of teacher-forced target scoring (include/qtx.h, target scoring): the contract
restated over the oracle — OracleModel.encode / decode(fault=...) / logits, the canonical
log-softmax, the pad-aware target mask of batch.py:25-30, the rank rule, and tgt_per_src by
np.repeat of the memory and the source mask.  Shared by tests/test_score_ref.py (CPU) and
tests/test_gpu_score.py (GPU == this, bit for bit), like tests/beam_ref.py.

The models: tests/model_cfgs.small_state for MODELS; the sources small_src(3, 9, 5); targets
of L = 10 tokens, so M = R * T = 27 rows: more than one 16-row generator block and no multiple
of 16; V = 97 and 8200 are no multiples of the generator's 64-column tile.  targets() builds
them from the oracle's greedy ids so that the ranks 0 and 1 occur by construction:
per sentence the first three labels are the greedy ones, the fourth is the greedy step's
runner-up, then seeded random tokens; sentences 0 and 1 end ``EOS PAD*``, sentence 2 runs to
the full length.
"""
import numpy as np

from oracle import qtx_oracle as O

f32 = np.float32
BOS, EOS, PAD = 0, 1, 2
MODELS = [(512, 8, 97), (2048, 8, 97), (512, 4, 97), (512, 8, 8200)]
SRC_ARGS = (3, 9, 5)
L = 10
# sentence -> position of its EOS (PAD after it); sentence 2 has none
ENDS = {0: 7, 1: 5}
_MEMO = {}


def memo(key, fn):
    if key not in _MEMO:
        _MEMO[key] = fn()
    return _MEMO[key]


def top2_of(logp):
    """The two best entries of each row under "larger value, then smaller index"."""
    logp = np.asarray(logp, f32)
    order = np.argsort(-logp, axis=-1, kind="stable")[:, :2].astype(np.int64)
    return order, np.take_along_axis(logp, order, axis=-1)


def score_logp(logp, y):
    """The rule on log-probability rows: logp f32 [M, V] (a non-finite row is all NaN, as
    O.log_softmax_argmax leaves it), y int64 [M] -> (tok_logp f32 [M], rank int32 [M], top_ids
    int64 [M, 2], top_logp f32 [M, 2])."""
    logp = np.asarray(logp, f32)
    y = np.asarray(y, np.int64)
    M, V = logp.shape
    bad = np.isnan(logp).any(-1)
    inside = (y >= 0) & (y < V)
    yc = np.where(inside, y, 0)
    ly = logp[np.arange(M), yc]
    idx = np.arange(V)[None, :]
    with np.errstate(invalid="ignore"):
        before = (logp > ly[:, None]) | ((logp == ly[:, None]) & (idx < yc[:, None]))
    ok = inside & ~bad
    tok = np.where(ok, ly, f32(np.nan)).astype(f32)
    rank = np.where(ok, before.sum(-1), -1).astype(np.int32)
    ti, tv = top2_of(np.where(bad[:, None], f32(0), logp))
    ti[bad] = (0, 1)
    tv[bad] = np.nan
    return tok, rank, ti, tv.astype(f32)


def score_logits(x, y):
    """score_logp on the canonical log-softmax of logits rows x [M, V]."""
    return score_logp(O.log_softmax_argmax(np.asarray(x, f32))[0], y)


def std_mask(tgt, pad):
    """make_std_mask (batch.py:25-30) of the decoder input tgt[:, :-1]: int64 [R, T, T];
    pad < 0: the causal mask alone [1, T, T]."""
    tin = np.asarray(tgt)[:, :-1]
    T = tin.shape[1]
    causal = np.tril(np.ones((1, T, T), np.int64))
    if pad < 0:
        return causal
    return ((tin != pad)[:, None, :] & (causal != 0)).astype(np.int64)


def score_ref(om, src, src_mask, tgt, pad=PAD, tgt_per_src=1, fault=None):
    """The contract on OracleModel `om`: a dict of tok_logp f32, rank int32 [R, T], top_ids
    int64, top_logp f32 [R, T, 2] and logp f32 [R, T, V].  fault: a Fault.as_dict() (module 0:
    the encoder pass, module 1: the decoder pass), tgt_per_src 1 only."""
    src, tgt = np.asarray(src), np.asarray(tgt)
    K = tgt_per_src
    R, T = tgt.shape[0], tgt.shape[1] - 1
    assert R == src.shape[0] * K and (fault is None or K == 1)
    enc_f = fault if fault is not None and fault["module"] == 0 else None
    dec_f = fault if fault is not None and fault["module"] == 1 else None
    memory = om.encode(om.embed(src, om.src_lut), src_mask, fault=enc_f)
    out = om.decode(om.embed(tgt[:, :T], om.tgt_lut), np.repeat(memory, K, axis=0),
                    np.repeat(np.asarray(src_mask), K, axis=0), std_mask(tgt, pad), fault=dec_f)
    logp = O.log_softmax_argmax(om.logits(out.reshape(R * T, -1)))[0]
    tok, rank, ti, tv = score_logp(logp, tgt[:, 1:].reshape(-1))
    return dict(tok_logp=tok.reshape(R, T), rank=rank.reshape(R, T), top_ids=ti.reshape(R, T, 2),
                top_logp=tv.reshape(R, T, 2), logp=logp.reshape(R, T, -1))


def model(d_ff, weight_bits=8, tgt_vocab=97):
    from model_cfgs import small_state
    return small_state(d_ff, weight_bits, tgt_vocab)


def inputs():
    from model_cfgs import small_src
    return small_src(*SRC_ARGS)


def greedy(d_ff, weight_bits=8, tgt_vocab=97):
    """The oracle's KV-cached greedy ids [3, L] of the shared sources."""
    def run():
        src, mask = inputs()
        return model(d_ff, weight_bits, tgt_vocab)[2].greedy_decode(src, mask, max_len=L)
    return memo(("greedy", d_ff, weight_bits, tgt_vocab), run)


def greedy_scores(d_ff, weight_bits=8, tgt_vocab=97):
    """score_ref of the oracle's own greedy ids (causal mask alone)."""
    def run():
        src, mask = inputs()
        return score_ref(model(d_ff, weight_bits, tgt_vocab)[2], src, mask,
                         greedy(d_ff, weight_bits, tgt_vocab), pad=-1)
    return memo(("greedy_scores", d_ff, weight_bits, tgt_vocab), run)


def targets(d_ff, weight_bits=8, tgt_vocab=97):
    """tgt int64 [3, L] (see the module docstring)."""
    def run():
        g = greedy(d_ff, weight_bits, tgt_vocab)
        gs = greedy_scores(d_ff, weight_bits, tgt_vocab)
        rng = np.random.default_rng(11)
        tgt = rng.integers(4, tgt_vocab, g.shape).astype(np.int64)
        tgt[:, :4] = g[:, :4]                     # start + three greedy labels
        tgt[:, 4] = gs["top_ids"][:, 3, 1]        # the runner-up of the greedy step 3
        for b, e in ENDS.items():
            tgt[b, e] = EOS
            tgt[b, e + 1:] = PAD
        return tgt
    return memo(("targets", d_ff, weight_bits, tgt_vocab), run)


def reference(d_ff, weight_bits=8, tgt_vocab=97, pad=PAD, rows=None, fault=None):
    """score_ref of targets() on the shared sources (rows: a subset of the sentences), once."""
    key = ("ref", d_ff, weight_bits, tgt_vocab, pad, tuple(rows) if rows is not None else None,
           repr(fault))
    def run():
        src, mask = inputs()
        tgt = targets(d_ff, weight_bits, tgt_vocab)
        if rows is not None:
            src, mask, tgt = src[list(rows)], mask[list(rows)], tgt[list(rows)]
        return score_ref(model(d_ff, weight_bits, tgt_vocab)[2], src, mask, tgt, pad=pad,
                         fault=None if fault is None else fault.as_dict())
    return memo(key, run)


def faults():
    """The fault trials of the (512, 8, 97) model on B = 3, S = 9, T = 9 (picked on the CPU:
    tests/test_score_ref.py asserts what each must change): an encoder linear INPUT, a decoder
    FFN1 WEIGHT, a decoder memory-K RANDOM and a decoder self-attention QK INPUT16.  Decoder
    rows index the [R * T] = 27 target tokens, the CK row the [B * S] = 27 memory tokens."""
    from qtx.fault import Fault
    return [
        Fault("INPUT", 0, 1, "FFN2", row=1 * 9 + 2, col=100, bit=6),
        Fault("WEIGHT", 1, 1, "FFN1", row=77, col=300, bit=6),
        Fault("RANDOM", 1, 0, "CK", row=2 * 9 + 1, col=130, value=3.0e3),
        Fault("INPUT16", 1, 0, "QK", row=2 * 9 + 6, col=3 * 64 + 5, bit=6, win_start=0, win_len=7),
    ]


def crafted_rows(V):
    """Logits rows [12, V] and labels [12] that exercise the rule: all-equal
    logits, two equal maxima, a 1-ulp pair, a NaN, a +inf, an all -inf row, the label at index
    0 and at V - 1, a label out of range on either side, a -inf label on a finite row."""
    rng = np.random.default_rng(1000 + V)
    base = lambda: rng.normal(0, 2, V).astype(f32)
    rows, ys = [], []
    add = lambda r, y: (rows.append(np.asarray(r, f32)), ys.append(int(y)))
    add(np.full(V, 0.5, f32), V - 1)                       # all equal: rank = the label's index
    r = base(); r[0] = r[V - 1] = r.max() + f32(1); add(r, V - 1)   # two equal maxima: rank 1
    r = base(); m = f32(r.max() + 1); r[V - 1] = m; r[0] = np.nextafter(m, f32(0)); add(r, 0)
    r = base(); r[V // 2] = np.nan; add(r, 1)
    r = base(); r[V - 1] = np.inf; add(r, 0)
    add(np.full(V, -np.inf, f32), 0)
    r = base(); add(r, 0)
    r = base(); add(r, V - 1)
    r = base(); add(r, V)
    r = base(); add(r, -1)
    r = base(); r[1] = -np.inf; add(r, 1)
    r = base(); add(r, int(np.argmax(r)))
    return np.stack(rows), np.asarray(ys, np.int64)

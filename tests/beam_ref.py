"""The reference of the beam-search decode (include/qtx.h, beam search): a beam search over
the oracle's KV-cached DecodeState, whose caches are numpy arrays indexed by a parent vector.
Shared by tests/test_beam_ref.py (CPU) and tests/test_gpu_beam.py (GPU == this, bit for bit).

The models: tests/model_cfgs.small_state with EOS_BOOST added to generator.proj.bias[EOS] in
a copy of the state dict (random weights otherwise almost never emit EOS), the sources
small_src(4, 9, 5), max_len 14, start 0 (PARAMS: the models that need another boost or seed to
meet the conditions below).  MODELS lists every (d_ff, weight_bits, tgt_vocab,
beam) the GPU tests decode; tests/test_beam_ref.py asserts for each that the search exercises
what it is meant to (finished sentences, reorders, shared parents, an early stop).
"""
import numpy as np

from oracle import qtx_oracle as O

f32 = np.float32
EOS, PAD, START = 1, 2, 0
EOS_BOOST = 2.0
MAX_LEN = 14
SRC_ARGS = (4, 9, 5)
# (d_ff, weight_bits, tgt_vocab, beam): the end-to-end cases of tests/test_gpu_beam.py
MODELS = [(512, 8, 97, 4), (512, 8, 97, 3), (512, 8, 97, 1), (2048, 8, 97, 4),
          (1024, 8, 97, 4), (512, 4, 97, 4), (512, 8, 8200, 2)]
# (d_ff, weight_bits, tgt_vocab) -> (EOS boost, small_src seed) where boost 2.0 / seed 5 misses
# a condition of tests/test_beam_ref.py (picked on the CPU): d_ff 2048 finishes every hypothesis
# at 2.0; d_ff 1024 has no sentence finished early at seed 5 for any boost tried (1.0 .. 3.5);
# the 8200-word model reorders at fewer than half of its steps at 2.0
PARAMS = {(2048, 8, 97): (1.5, 5), (1024, 8, 97): (3.5, 9), (512, 8, 8200): (1.5, 5)}
_CACHE = {}


def params(d_ff, weight_bits=8, tgt_vocab=97):
    return PARAMS.get((d_ff, weight_bits, tgt_vocab), (EOS_BOOST, SRC_ARGS[2]))


def boosted_state(d_ff, weight_bits=8, tgt_vocab=97, boost=None):
    """(cfg, state dict copy with the EOS bias raised, its OracleModel), built once."""
    boost = params(d_ff, weight_bits, tgt_vocab)[0] if boost is None else boost
    key = (d_ff, weight_bits, tgt_vocab, boost)
    if key not in _CACHE:
        from model_cfgs import small_state
        cfg, sd, _ = small_state(d_ff, weight_bits, tgt_vocab)
        sd = dict(sd)
        b = np.array(sd["generator.proj.bias"], f32, copy=True)
        b[EOS] += f32(boost)
        sd["generator.proj.bias"] = b
        _CACHE[key] = (cfg, sd, O.OracleModel(sd, n_layers=cfg.n_layers, n_bits=weight_bits))
    return _CACHE[key]


def select_ref(score, fin, logp, pad):
    """Rules 3-4 for one sentence: score f32 [K], fin bool [K], logp f32 [K, V] ->
    (parent [K], token [K], value f32 [K]), the K best candidates under "larger value, then
    smaller flat"."""
    score = np.asarray(score, f32)
    logp = np.asarray(logp, f32)
    K, V = logp.shape
    with np.errstate(invalid="ignore", over="ignore"):
        cand = (score[:, None] + logp).astype(f32)
    cand = np.where(np.isfinite(cand), cand, f32(-np.inf)).astype(f32)
    vals, flats = [], []
    for k in range(K):
        if fin[k]:
            vals.append(np.array([score[k]], f32))
            flats.append(np.array([k * V + pad], np.int64))
        else:
            vals.append(cand[k])
            flats.append(k * V + np.arange(V, dtype=np.int64))
    vals, flats = np.concatenate(vals), np.concatenate(flats)
    order = np.lexsort((flats, -vals.astype(np.float64)))[:K]
    return flats[order] // V, flats[order] % V, vals[order]


def beam_ref(om, src, src_mask, max_len, beam, start=START, eos=EOS, pad=PAD):
    """The beam search of include/qtx.h on OracleModel `om`.  Returns a dict: hyp_ids int64
    [B, K, max_len], hyp_score f32 [B, K], hyp_len int32 [B, K], fin bool [B, K], steps_run
    (steps executed until every row was finished, at most max_len - 1), and the trace:
    parents [steps][B, K], fins [steps][B, K] (the flags after each step)."""
    src = np.asarray(src)
    B, K = src.shape[0], beam
    R = B * K
    memory = om.encode(om.embed(src, om.src_lut), src_mask)
    st = O.DecodeState(om, np.repeat(memory, K, axis=0),
                       np.repeat(np.asarray(src_mask), K, axis=0), max_len)
    score = np.full((B, K), -np.inf, f32)
    score[:, 0] = 0
    fin = np.zeros((B, K), bool)
    length = np.zeros((B, K), np.int32)
    hist = np.full((B, K, max_len), pad, np.int64)
    hist[:, :, 0] = start
    tok_in = np.full((R, 1), start, np.int64)
    parents, fins = [], []
    steps = 0
    for t in range(max_len - 1):
        out = st.step(om.embed(tok_in, om.tgt_lut, pos0=t))
        logp = O.log_softmax_argmax(om.logits(out))[0].reshape(B, K, -1)
        par = np.zeros((B, K), np.int64)
        tok = np.zeros((B, K), np.int64)
        for b in range(B):
            par[b], tok[b], score[b] = select_ref(score[b], fin[b], logp[b], pad)
        rows = (np.arange(B)[:, None] * K + par).reshape(-1)
        for L in range(om.N):
            st.kcache[L] = tuple(a[rows] for a in st.kcache[L])
            st.vcache[L] = tuple(a[rows] for a in st.vcache[L])
        pfin = np.take_along_axis(fin, par, 1)
        hist = np.take_along_axis(hist, par[:, :, None], 1)
        hist[:, :, t + 1] = tok
        length = np.where(pfin, np.take_along_axis(length, par, 1), t + 1).astype(np.int32)
        fin = pfin | (tok == eos)
        tok_in = tok.reshape(R, 1)
        parents.append(par)
        fins.append(fin.copy())
        steps = t + 1
        if fin.all():
            break
    return dict(hyp_ids=hist, hyp_score=score, hyp_len=length, fin=fin, steps_run=steps,
                parents=parents, fins=fins)


def rank(hyp_score, hyp_len, length_penalty=0.0):
    """The Python layer's ranking: per sentence the stable descending order of
    score / max(len, 1) ** length_penalty in float64.  Returns the order [B, K]."""
    s = np.asarray(hyp_score, np.float64) / np.maximum(np.asarray(hyp_len), 1) ** float(length_penalty)
    return np.argsort(-s, axis=-1, kind="stable")


def inputs(d_ff=512, weight_bits=8, tgt_vocab=97):
    from model_cfgs import small_src
    return small_src(SRC_ARGS[0], SRC_ARGS[1], params(d_ff, weight_bits, tgt_vocab)[1])


def early_rows(ref):
    """Up to two sentences whose hypotheses are all finished before the last step: decoded
    alone they stop early (for the d_ff 512 model: sentences 0 and 2)."""
    fins = np.stack(ref["fins"])
    return tuple(b for b in range(fins.shape[1]) if fins[:-1, b].all(-1).any())[:2]


_REF = {}


def reference(d_ff, weight_bits, tgt_vocab, beam, rows=None, max_len=MAX_LEN):
    """beam_ref of one model on the shared sources (rows: a subset of the sentences), once."""
    key = (d_ff, weight_bits, tgt_vocab, beam, tuple(rows) if rows is not None else None, max_len)
    if key not in _REF:
        src, mask = inputs(d_ff, weight_bits, tgt_vocab)
        if rows is not None:
            src, mask = src[list(rows)], mask[list(rows)]
        om = boosted_state(d_ff, weight_bits, tgt_vocab)[2]
        _REF[key] = beam_ref(om, src, mask, max_len, beam)
    return _REF[key]

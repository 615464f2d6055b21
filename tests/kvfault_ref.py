"""The contract of qtx_greedy_decode_kvfault (include/qtx.h): faults of the KV-cached decode
itself, on the oracle (a helper module, not a conftest).

The reference has no KV cache, so nothing in it says what a fault in a cached step does.  This
module says it, the way tests/beam_ref.py does for the beam search: step() restates
oracle.qtx_oracle.DecodeState.step, operation for operation, with one optional fault handed to
the oracle's own QLinear(fault=) and attention(fault=); apply_upset() flips one stored bit of
DecodeState.kcache / vcache / cross; apply_cross_fault() redoes the one-time memory K/V
projection with a CK / CV fault.  It imports oracle/ and changes nothing in it.

trial() is the decode: steps 0 .. i-1 golden, step i's cached run with the fault (or on the
upset caches), steps i+1 .. KV-cached from whatever step i left in the caches and in ys.  The
top 2 of a step are the two best entries of its oracle logp row under a stable descending sort
(the first-index rule, as tests/dfault_cases.py).  The golden decode and the state before each
of its steps are computed once per input and shared.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dfault_cases import memo, top2_of  # noqa: E402
from oracle.qtx_oracle import DecodeState, attention, layer_norm  # noqa: E402

f32 = np.float32


def step(st, y, fault=None):
    """DecodeState.step with one fault (a qtx.fault.Fault.as_dict() with module 1, or None):
    y [B,1,512] -> decoder output [B,512]; appends this step's K/V rows — computed with the
    fault — to st.  Linear targets see the step's [B] token rows; attention targets Sq = 1 and
    Sk = the keys of this step (self: the position + 1; cross: S)."""
    m = st.m
    x = np.asarray(y, f32)
    B = x.shape[0]
    for L, lp in enumerate(m.dec):
        lf = lambda lin, n=512: m._lin_fault(fault, 1, L, lin, B, n)   # noqa: E731
        h = layer_norm(x, *lp["ln"][0])
        lin = lp["self_attn"]
        qq, sq = lin[0](h, quantize_output=True, fault=lf("Q"))
        k = lin[1](h, quantize_output=True, fault=lf("K"))
        v = lin[2](h, quantize_output=True, fault=lf("V"))
        if st.kcache[L] is None:
            st.kcache[L], st.vcache[L] = k, v
        else:
            st.kcache[L] = tuple(np.concatenate([a, b], 1) for a, b in zip(st.kcache[L], k))
            st.vcache[L] = tuple(np.concatenate([a, b], 1) for a, b in zip(st.vcache[L], v))
        (qk, sk), (qv, sv) = st.kcache[L], st.vcache[L]
        Sk = qk.shape[1]
        ones = np.ones((B, 1, Sk), np.int64)
        ctx, _ = attention(qq, sq, qk, sk, qv, sv, ones, m.H, dec=True,
                           fault=m._attn_fault(fault, 1, L, "QK", "PV", 1, Sk))
        x = x + lin[3](ctx, fault=lf("O"))
        h = layer_norm(x, *lp["ln"][1])
        lin = lp["src_attn"]
        qq, sq = lin[0](h, quantize_output=True, fault=lf("CQ"))
        (qk, sk), (qv, sv) = st.cross[L]
        ctx, _ = attention(qq, sq, qk, sk, qv, sv, st.sm, m.H, dec=True,
                           fault=m._attn_fault(fault, 1, L, "CQK", "CPV", 1, qk.shape[1]))
        x = x + lin[3](ctx, fault=lf("CO"))
        x = x + m.ffn(lp, layer_norm(x, *lp["ln"][2]),
                      [lf("FFN1", lp["w1"].q.shape[0]), lf("FFN2")])
    return layer_norm(x, *m.dec_norm)[:, 0]


def clone(st):
    """A DecodeState that shares st's arrays (step() replaces, never mutates, a cache entry;
    apply_upset copies what it changes)."""
    n = object.__new__(DecodeState)
    n.m, n.sm = st.m, st.sm
    n.cross, n.kcache, n.vcache = list(st.cross), list(st.kcache), list(st.vcache)
    return n


def apply_cross_fault(st, memory, fault):
    """The one-time memory K/V projection of the fault's layer again, with the CK / CV fault
    (rows index the [B * S] memory tokens)."""
    m = st.m
    mrows = memory.shape[0] * memory.shape[1]
    L = fault["layer"]
    lin = m.dec[L]["src_attn"]
    st.cross[L] = (lin[1](memory, quantize_output=True, fault=m._lin_fault(fault, 1, L, "CK", mrows, 512)),
                   lin[2](memory, quantize_output=True, fault=m._lin_fault(fault, 1, L, "CV", mrows, 512)))


def apply_upset(st, upset, max_len):
    """One stored bit flipped (a qtx.fault.CacheUpset.as_dict()): row = b * max_len + j for
    the self caches (j a position already cached), b * S + j for the cross caches; field
    "code": bit 0..7 of the int8 code at col; "scale": bit 0..22 or 31 of the row's float32
    scale."""
    L, cache = upset["layer"], upset["cache"]
    is_v = cache.endswith("_v")
    if cache.startswith("self"):
        q, s = (st.vcache if is_v else st.kcache)[L]
        b, j = divmod(int(upset["row"]), max_len)
        assert j < q.shape[1], "self-cache position not written yet"
    else:
        q, s = st.cross[L][1 if is_v else 0]
        b, j = divmod(int(upset["row"]), q.shape[1])
    q, s = q.copy(), s.copy()
    bit = int(upset["bit"])
    if upset["field"] == "code":
        assert 0 <= bit <= 7
        q.view(np.uint8)[b, j, int(upset["col"])] ^= np.uint8(1 << bit)
    else:
        assert 0 <= bit <= 22 or bit == 31
        s.view(np.uint32)[b, j] ^= np.uint32(1 << bit)
    if cache.startswith("self"):
        (st.vcache if is_v else st.kcache)[L] = (q, s)
    else:
        pair = list(st.cross[L])
        pair[1 if is_v else 0] = (q, s)
        st.cross[L] = tuple(pair)


def _run(om, st, ys, t0, last, fault=None):
    """Steps t0 .. last-1 from ys [B, t0+1] on st, the first with `fault`: (ys, ids, logp)."""
    ti, tv = [], []
    for t in range(t0, last):
        out = step(st, om.embed(ys[:, -1:], om.tgt_lut, pos0=t), fault if t == t0 else None)
        logp, nxt = om.generator(out)
        i2, v2 = top2_of(logp)
        assert np.array_equal(i2[:, 0], nxt)
        ti.append(i2)
        tv.append(v2)
        ys = np.concatenate([ys, nxt[:, None]], axis=1)
    return ys, ti, tv


def golden(om, src, m, max_len, tag, start=0):
    """The golden KV-cached decode: dict(memory, ys, top_ids, top_logp, snaps), snaps[t] the
    state before step t."""
    def run():
        src_ = np.asarray(src)
        memory = om.encode(om.embed(src_, om.src_lut), m)
        st = DecodeState(om, memory, m, max_len)
        ys = np.full((src_.shape[0], 1), start, np.int64)
        snaps, ti, tv = [], [], []
        for t in range(max_len - 1):
            snaps.append(clone(st))
            ys, i2, v2 = _run(om, st, ys, t, t + 1)
            ti += i2
            tv += v2
        return dict(memory=memory, ys=ys, top_ids=np.stack(ti, 1), top_logp=np.stack(tv, 1),
                    snaps=snaps)
    return memo(("kvgold", tag, max_len, start), run)


def trial(om, src, m, max_len, tag, fault=None, upset=None, step_i=0):
    """(ys, top_ids, top_logp, record) of one decode with a step fault (qtx.fault.Fault) or a
    cache upset (qtx.fault.CacheUpset) effective at step_i; record = (golden ids, golden logp,
    faulty ids, faulty logp) [B, 2] each, or None when step_i >= max_len - 1 (golden decode)."""
    assert (fault is None) != (upset is None)

    def run():
        g = golden(om, src, m, max_len, tag)
        last = max_len - 1
        if step_i >= last:
            return g["ys"], g["top_ids"], g["top_logp"], None
        st = clone(g["snaps"][step_i])
        fd = fault.as_dict() if fault is not None else None
        if upset is not None:
            apply_upset(st, upset.as_dict(), max_len)
        elif fd["linear"] in ("CK", "CV"):
            assert step_i == 0
            apply_cross_fault(st, g["memory"], fd)
            fd = None
        ys, ti, tv = _run(om, st, g["ys"][:, :step_i + 1], step_i, last, fd)
        top_ids, top_logp = g["top_ids"].copy(), g["top_logp"].copy()
        top_ids[:, step_i:], top_logp[:, step_i:] = np.stack(ti, 1), np.stack(tv, 1)
        rec = (g["top_ids"][:, step_i], g["top_logp"][:, step_i], ti[0], tv[0])
        return ys, top_ids, top_logp, rec
    return memo(("kvtrial", tag, max_len, repr(fault), repr(upset), step_i), run)


def effect(om, src, m, max_len, tag, exp):
    """'tokens' / 'scores' / 'none': what a trial's result changes against the golden decode."""
    g = golden(om, src, m, max_len, tag)
    if not np.array_equal(exp[0], g["ys"]):
        return "tokens"
    same = np.array_equal(exp[2].view(np.uint32), g["top_logp"].view(np.uint32))
    return "none" if same and np.array_equal(exp[1], g["top_ids"]) else "scores"

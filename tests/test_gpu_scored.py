"""The scored decode (include/qtx.h: per-step top-2 tokens and log-probabilities) against
the oracle, bit for bit.

Expected values never come from the code under test: oracle_scored_decode() drives
O.DecodeState step by step (embed, step, oracle_model.generator) and top2_of() takes the two
best entries of each oracle logp row with a stable descending sort — the first-index rule.
Floats are compared with assert_array_equal.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from oracle import qtx_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from guarded import POISONS, guarded  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
S0 = C.c_void_p(0)
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


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else S0


def call(name, *args):
    from qtx import _lib
    _lib.call(name, *args)


def top2_of(logp):
    """[M, V] log-probs -> (ids int64 [M, 2], values f32 [M, 2]): stable descending sort, so
    equal values keep index order; an all-NaN row gives ids (0, 1)."""
    logp = np.asarray(logp, f32)
    order = np.argsort(-logp, axis=-1, kind="stable")[:, :2].astype(np.int64)
    return order, np.take_along_axis(logp, order, axis=-1)


def make_src(rng, B, S, lens):
    src = np.full((B, S), 2, np.int64)          # PAD
    for b, n in enumerate(lens):
        src[b, 0] = 0
        src[b, 1:n - 1] = rng.integers(4, 5337, n - 2)
        src[b, n - 1] = 1
    return src, (src != 2)[:, None, :]


def oracle_scored_decode(om, src, mask, max_len, start=0, fault=None):
    """(ys [B, max_len], top_ids [B, max_len-1, 2], top_logp [B, max_len-1, 2]) of the
    KV-cached oracle decode; fault: an encoder fault dict or None."""
    B = src.shape[0]
    memory = om.encode(om.embed(src, om.src_lut), mask, fault=fault)
    st = O.DecodeState(om, memory, mask, max_len)
    ys = np.full((B, 1), start, np.int64)
    ti, tv = [], []
    for t in range(max_len - 1):
        out = st.step(om.embed(ys[:, -1:], om.tgt_lut, pos0=t))
        logp, nxt = om.generator(out)
        i2, v2 = top2_of(logp)
        assert np.array_equal(i2[:, 0], nxt)     # the oracle's own argmax is its top 1
        ti.append(i2)
        tv.append(v2)
        ys = np.concatenate([ys, nxt[:, None]], axis=1)
    return ys, np.stack(ti, 1), np.stack(tv, 1)


def gpu_scored(gpu_model, src, mask, max_len):
    from qtx.decode import greedy_decode
    ys, sc = greedy_decode(gpu_model, src, mask, max_len, 0, return_scores=True)
    assert sc.top_ids.shape == (src.shape[0], max_len - 1, 2) and sc.top_ids.dtype == np.int64
    assert sc.top_logp.shape == (src.shape[0], max_len - 1, 2) and sc.top_logp.dtype == f32
    np.testing.assert_array_equal(sc.top_ids[..., 0], ys[:, 1:])
    return ys, sc.top_ids, sc.top_logp


# =====================================================================================
# 1. the per-op tail on crafted logits
# =====================================================================================
def crafted_rows(V, seed):
    """Random rows plus ties, a logp collision, -inf entries and the non-finite kinds.
    Returns (logits [M, V], the row index of the collision case)."""
    rng = np.random.default_rng(seed)
    rows = [(rng.standard_normal(V) * 2).astype(f32) for _ in range(5)]
    base = lambda: (rng.standard_normal(V) * 2).astype(f32)
    hi = min(V - 1, 4000)

    r = base()                                   # the maximum twice
    r[[hi, 0] if V == 2 else [hi, 1]] = r.max() + f32(1)
    rows.append(r)
    if V >= 3:
        r = base()                               # three times
        r[[V - 1, V // 2, 1]] = r.max() + f32(1)
        rows.append(r)
        r = base()                               # the runner-up twice
        top = r.max() + f32(2)
        r[V // 2] = top
        r[[V - 1, 0]] = top - f32(1)
        rows.append(r)
    # two distinct logits whose logp collide: the second one stepped down 1..16 ulps.  The
    # logits are small (fine ulps) and close together (a denominator near V: coarse logp ulps)
    found = None
    a, b = V - 1, (0 if V == 2 else V // 3)      # the larger logit at the HIGHER index
    for mx in (f32(0.2), f32(0.1), f32(0.05), f32(0.01)):
        r = (rng.uniform(-1, 1, V) * 0.005).astype(f32)
        r[a] = mx
        x = mx
        for k in range(1, 17):
            x = np.nextafter(x, f32(-np.inf))
            r[b] = x
            lp = O.log_softmax_argmax(r[None])[0][0]
            if lp[a] == lp[b]:
                found = r.copy()
                break
        if found is not None:
            break
    assert found is not None, f"no logp collision of distinct logits found at V={V}"
    assert found[a] != found[b]
    collide = len(rows)
    rows.append(found)
    r = base()                                   # -inf among finite values: a normal row
    r[::3] = -np.inf
    r[V - 1] = f32(1)
    rows.append(r)
    if V == 2:
        rows.append(np.array([0, -np.inf], f32))
    r = base(); r[V // 2] = np.nan; rows.append(r)          # the three non-finite kinds
    r = base(); r[V - 1] = np.inf; rows.append(r)
    rows.append(np.full(V, -np.inf, f32))
    return np.stack(rows), collide


@pytest.fixture(scope="module")
def vocab_models(torch, gpu_model):
    """One-layer models that differ in tgt_vocab (the tail kernels see nothing else of them)."""
    from qtx.model import QtxModel
    from qtx.weights import ModelConfig, synthetic_state_dict
    cache = {4444: gpu_model}

    def get(V):
        if V not in cache:
            cfg = ModelConfig(src_vocab=16, tgt_vocab=V, n_layers=1, max_len=64)
            cache[V] = QtxModel(synthetic_state_dict(7, cfg), cfg)
        return cache[V]
    return get


@pytest.mark.parametrize("poison", POISONS, ids=lambda p: f"poison{p:02X}")
@pytest.mark.parametrize("V", [2, 63, 1024, 1025, 4444, 8192])
def test_decode_top2_embed(torch, vocab_models, oracle_model, V, poison):
    """qtx_decode_top2_embed: ids and values == the oracle's two best of logp (ties, a
    collision of distinct logits, -inf entries, non-finite rows); the ids column and x_next
    == qtx_decode_argmax_embed on the same input; nothing outside the stated extents is
    written (M = 5 rows per launch, every crafted row in one of them)."""
    model = vocab_models(V)
    lg_all, collide = memo(("rows", V), lambda: crafted_rows(V, 100 + V))
    want_lp = memo(("lp", V), lambda: O.log_softmax_argmax(lg_all)[0])
    want_i, want_v = top2_of(want_lp)
    # the setup is what it claims: the collision row's two logits share one logp, and the
    # lower index wins although its logit is smaller
    a, b = V - 1, (0 if V == 2 else V // 3)
    assert lg_all[collide, b] < lg_all[collide, a] and want_i[collide].tolist() == [b, a]
    assert np.isnan(want_v[-3:]).all() and (want_i[-3:] == [0, 1]).all()
    M, ids_bs, s = 5, 7, 3
    dt = {np.int64: torch.int64, np.int32: torch.int32, f32: torch.float32}
    n = len(lg_all)
    for r0 in range(0, n, M):
        rows = np.arange(r0, r0 + M) % n         # (the last launch wraps round to the first rows)
        lg = lg_all[rows]
        lgd = torch.from_numpy(np.ascontiguousarray(lg)).cuda()
        checks, bufs = [], {}
        for name, shape, kind in (("ids", (M, ids_bs), np.int64), ("top_ids", (M, ids_bs - 1, 2), np.int64),
                                  ("top_logp", (M, ids_bs - 1, 2), f32), ("x_next", (M, 512), f32),
                                  ("step", (2,), np.int32)):
            t, c = guarded(torch, shape, dt[kind], poison, name=name)
            bufs[name] = t
            checks.append(c)
        ids0 = np.arange(M * ids_bs, dtype=np.int64).reshape(M, ids_bs) - 50
        bufs["ids"].copy_(torch.from_numpy(ids0))
        bufs["step"].copy_(torch.tensor([s, 0], dtype=torch.int32))
        ti0, tl0 = bufs["top_ids"].cpu().numpy(), bufs["top_logp"].cpu().numpy().view(np.uint32)
        call("qtx_decode_top2_embed", model.handle, P(lgd), M, P(bufs["ids"]), ids_bs,
             P(bufs["top_ids"]), P(bufs["top_logp"]), P(bufs["step"]), P(bufs["x_next"]), S0)
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:       # a device fault: nothing more may run on this GPU
            pytest.exit(f"GPU error at synchronize, stopping the session: {e}", returncode=3)
        for c in checks:
            c()
        # the plain tail on the same input
        ids_p = torch.from_numpy(ids0).cuda()
        step_p = torch.tensor([s, 0], dtype=torch.int32, device="cuda")
        xn_p = torch.empty((M, 512), dtype=torch.float32, device="cuda")
        call("qtx_decode_argmax_embed", model.handle, P(lgd), M, P(ids_p), ids_bs, P(step_p),
             P(xn_p), S0)
        ti, tl = bufs["top_ids"].cpu().numpy(), bufs["top_logp"].cpu().numpy()
        msg = f"V={V} rows {rows.tolist()}"
        np.testing.assert_array_equal(ti[:, s], want_i[rows], err_msg=msg)
        np.testing.assert_array_equal(tl[:, s], want_v[rows], err_msg=msg)
        # only entry s of top_ids / top_logp changed
        keep = np.arange(ids_bs - 1) != s
        np.testing.assert_array_equal(ti[:, keep], ti0[:, keep])
        np.testing.assert_array_equal(tl.view(np.uint32)[:, keep], tl0[:, keep])
        ids1 = ids0.copy()
        ids1[:, s + 1] = want_i[rows, 0]
        np.testing.assert_array_equal(bufs["ids"].cpu().numpy(), ids1, err_msg=msg)
        np.testing.assert_array_equal(bufs["step"].cpu().numpy(), [s + 1, 0])
        np.testing.assert_array_equal(bufs["ids"].cpu().numpy(), ids_p.cpu().numpy(), err_msg=msg)
        np.testing.assert_array_equal(bufs["x_next"].cpu().numpy().view(np.uint32),
                                      xn_p.cpu().numpy().view(np.uint32), err_msg=msg)


def test_generator_top2(torch, gpu_model, oracle_model):
    """qtx_generator_top2 (the one-wave-per-row kernel; no model-independent route to it):
    random x [37, 512] against oracle_model.generator."""
    rng = np.random.default_rng(37)
    x = (rng.standard_normal((37, 512)) * np.linspace(0.2, 3, 37)[:, None]).astype(f32)
    want_i, want_v = top2_of(oracle_model.generator(x)[0])
    ti, tl = gpu_model.generator_top2(torch.from_numpy(x).cuda())
    np.testing.assert_array_equal(ti.cpu().numpy(), want_i)
    np.testing.assert_array_equal(tl.cpu().numpy(), want_v)
    # the C entry point between guards: exactly [M, 2] ids and values, M * tgt_vocab floats of ws
    M, V = 37, 4444
    gi, ci = guarded(torch, (M, 2), torch.int64, 0xA5, name="top_ids")
    gl, cl = guarded(torch, (M, 2), torch.float32, 0xA5, name="top_logp")
    ws, cw = guarded(torch, (M * V,), torch.float32, 0xA5, name="ws", pitch_bytes=4 * V)
    xd = torch.from_numpy(x).cuda()
    call("qtx_generator_top2", gpu_model.handle, P(xd), M, P(gi), P(gl), P(ws), M * V * 4, S0)
    torch.cuda.synchronize()
    for c in (ci, cl, cw):
        c()
    np.testing.assert_array_equal(gi.cpu().numpy(), want_i)
    np.testing.assert_array_equal(gl.cpu().numpy(), want_v)
    np.testing.assert_array_equal(ws.cpu().numpy().reshape(M, V), oracle_model.logits(x))
    from qtx import _lib
    rc = _lib.lib().qtx_generator_top2(gpu_model.handle, P(xd), M, P(gi), P(gl), P(ws), M * V * 4 - 1, S0)
    assert rc == 3                                   # QTX_E_WORKSPACE


# =====================================================================================
# 2 - 7. the scored decode
# =====================================================================================
def test_scored_decode_matches_oracle(torch, gpu_model, oracle_model):
    from qtx.decode import greedy_decode
    rng = np.random.default_rng(21)
    B, S, L = 3, 13, 12
    src, m = make_src(rng, B, S, [13, 7, 10])
    ys, ti, tl = gpu_scored(gpu_model, src, m, L)
    np.testing.assert_array_equal(ys, greedy_decode(gpu_model, src, m, L, 0))
    oy, oi, ov = oracle_scored_decode(oracle_model, src, m, L)
    np.testing.assert_array_equal(ys, oy)
    np.testing.assert_array_equal(ti, oi)
    np.testing.assert_array_equal(tl, ov)
    # torch in, torch out
    ys_t, sc = greedy_decode(gpu_model, torch.from_numpy(src), torch.from_numpy(m), L, 0,
                             return_scores=True)
    assert isinstance(sc.top_logp, torch.Tensor) and sc.margin.shape == (B, L - 1)
    np.testing.assert_array_equal(sc.top_logp.numpy(), tl)


def _paths_inputs():
    rng = np.random.default_rng(55)
    return make_src(rng, 5, 24, [24, 9, 17, 24, 12])


@pytest.fixture(scope="module")
def paths_default(torch, gpu_model):
    src, m = _paths_inputs()
    return gpu_scored(gpu_model, src, m, 40)


@pytest.mark.parametrize("env", [{"QTX_NO_GRAPH": 1}, {"QTX_UNFUSED": 1}, {"QTX_GRAPH_STEPS": 13},
                                 {"QTX_DECODE_GROUPS": 3},
                                 {"QTX_DECODE_GROUPS": 2, "QTX_NO_GRAPH": 1}],
                         ids=lambda e: "-".join(f"{k[4:].lower()}{v}" for k, v in e.items()))
def test_scored_paths_agree(torch, gpu_model, paths_default, knob_env, env):
    """Eager launches, the unfused step, graphs of 13 steps (the device step counter) and
    sub-batch groups give the default path's ids and scores."""
    src, m = _paths_inputs()
    for k, v in env.items():
        knob_env(k, v)
    ys, ti, tl = gpu_scored(gpu_model, src, m, 40)
    np.testing.assert_array_equal(ys, paths_default[0])
    np.testing.assert_array_equal(ti, paths_default[1])
    np.testing.assert_array_equal(tl, paths_default[2])


def test_scored_long_source_matches_oracle(torch, gpu_model, oracle_model):
    """S = 160 > 128: the unfused step (k_lsm_top2)."""
    rng = np.random.default_rng(160)
    src, m = make_src(rng, 2, 160, [160, 131])
    ys, ti, tl = gpu_scored(gpu_model, src, m, 10)
    oy, oi, ov = oracle_scored_decode(oracle_model, src, m, 10)
    np.testing.assert_array_equal(ys, oy)
    np.testing.assert_array_equal(ti, oi)
    np.testing.assert_array_equal(tl, ov)


def test_plain_and_scored_graphs_do_not_mix(torch, gpu_model):
    """Plain, scored, plain, scored at one shape: each replays its own captured step."""
    from qtx.decode import greedy_decode
    rng = np.random.default_rng(77)
    src, m = make_src(rng, 4, 11, [11, 6, 9, 11])
    p0 = greedy_decode(gpu_model, src, m, 9, 0)
    s0 = gpu_scored(gpu_model, src, m, 9)
    p1 = greedy_decode(gpu_model, src, m, 9, 0)
    s1 = gpu_scored(gpu_model, src, m, 9)
    np.testing.assert_array_equal(p1, p0)
    np.testing.assert_array_equal(s0[0], p0)
    for a, b in zip(s0, s1):
        np.testing.assert_array_equal(b, a)


def test_scored_workspace_and_extents(torch, gpu_model):
    """The scores lie behind the plain workspace layout; a plain-sized workspace is
    QTX_E_WORKSPACE before anything is written; ids / top_ids / top_logp are written at
    exactly [B, max_len], [B, max_len-1, 2], [B, max_len-1, 2]."""
    from qtx import _lib
    L_ = _lib.lib()
    B, S, L = 3, 10, 6
    plain = L_.qtx_greedy_workspace_size(gpu_model.handle, B, S, L)
    scored = L_.qtx_greedy_scored_workspace_size(gpu_model.handle, B, S, L)
    assert scored >= plain + B * (L - 1) * 2 * (8 + 4) and scored < plain + 4096
    rng = np.random.default_rng(6)
    src, m = make_src(rng, B, S, [10, 5, 8])
    srcd = torch.from_numpy(src).cuda()
    md = torch.from_numpy(m.reshape(B, S).astype(np.uint8)).cuda()
    ids, c0 = guarded(torch, (B, L), torch.int64, 0x5A, name="ids")
    ti, c1 = guarded(torch, (B, L - 1, 2), torch.int64, 0x5A, name="top_ids")
    tl, c2 = guarded(torch, (B, L - 1, 2), torch.float32, 0x5A, name="top_logp")
    ws = torch.empty(scored, dtype=torch.uint8, device="cuda")
    args = (gpu_model.handle, P(srcd), P(md), B, S, L, 0, P(ids), P(ti), P(tl), P(ws))
    assert L_.qtx_greedy_decode_scored(*args, plain, None, S0) == 3      # QTX_E_WORKSPACE
    torch.cuda.synchronize()
    assert bool((ids.view(torch.uint8) == 0x5A).all()) and bool((tl.view(torch.uint8) == 0x5A).all())
    call("qtx_greedy_decode_scored", *args, scored, None, S0)
    torch.cuda.synchronize()
    for c in (c0, c1, c2):
        c()
    ys, i2, l2 = gpu_scored(gpu_model, src, m, L)
    np.testing.assert_array_equal(ids.cpu().numpy(), ys)
    np.testing.assert_array_equal(ti.cpu().numpy(), i2)
    np.testing.assert_array_equal(tl.cpu().numpy(), l2)


def test_scored_batch_invariance(torch, gpu_model):
    rng = np.random.default_rng(32)
    lens = rng.integers(5, 25, 32)
    lens[0], lens[31] = 24, 8
    src, m = make_src(rng, 32, 24, lens)
    ys, ti, tl = gpu_scored(gpu_model, src, m, 24)
    for b in (0, 31):
        y1, i1, l1 = gpu_scored(gpu_model, src[b:b + 1], m[b:b + 1], 24)
        np.testing.assert_array_equal(y1[0], ys[b])
        np.testing.assert_array_equal(i1[0], ti[b])
        np.testing.assert_array_equal(l1[0], tl[b])


def test_scored_int4_model(torch, state_dict):
    from qtx.model import QtxModel
    from qtx.weights import ModelConfig
    model = QtxModel(state_dict, ModelConfig(weight_bits=4))
    om = O.OracleModel(state_dict, n_bits=4)
    rng = np.random.default_rng(4)
    src, m = make_src(rng, 2, 9, [9, 6])
    ys, ti, tl = gpu_scored(model, src, m, 8)
    oy, oi, ov = oracle_scored_decode(om, src, m, 8)
    np.testing.assert_array_equal(ys, oy)
    np.testing.assert_array_equal(ti, oi)
    np.testing.assert_array_equal(tl, ov)


# =====================================================================================
# 8. the campaign's record
# =====================================================================================
@pytest.mark.parametrize("kind", ["OUTPUT", "WEIGHT"])
def test_decoder_fault_record(torch, gpu_model, oracle_model, kind):
    """greedy_decode_fault(return_scores=True) with a decoder fault at step 2: every step's
    top 2 of the faulty decode, and the corrupted step's golden / faulty top 2 and
    token_changed, all derived from oracle_model.decode(..., fault=...) + generator."""
    from qtx import fault as F
    from qtx.decode import greedy_decode_fault
    rng = np.random.default_rng(8)
    B, S, L, step = 1, 9, 6, 2
    src, m = make_src(rng, B, S, [9])
    T = step                                     # the faulty step's prefix length
    if kind == "OUTPUT":     # the last position's FFN2 output in the last layer, a large value
        f = F.Fault("OUTPUT", 1, 5, "FFN2", row=T - 1, col=100, value=3.0e4)
    else:
        f = F.Fault("WEIGHT", 1, 3, "O", row=77, col=300, bit=0)
    ys, sc = greedy_decode_fault(gpu_model, src, m, L, 0, fault=f, target_inference_number=step,
                                 return_scores=True)
    om = oracle_model
    memory = om.encode(om.embed(src, om.src_lut), m)
    oy = np.full((B, 1), 0, np.int64)
    oi, ov, rec = [], [], None
    for i in range(L - 1):
        Tn = oy.shape[1]
        y = om.embed(oy, om.tgt_lut)
        tm = np.tril(np.ones((1, Tn, Tn), np.int64))
        out = om.decode(y, memory, m, tm, fault=f.as_dict() if i == step - 1 else None)
        logp, nxt = om.generator(out[:, -1])
        i2, v2 = top2_of(logp)
        if i == step - 1:
            gi, gv = top2_of(om.generator(om.decode(y, memory, m, tm)[:, -1])[0])
            rec = (gi, gv, i2, v2)
        oi.append(i2)
        ov.append(v2)
        oy = np.concatenate([oy, nxt[:, None]], axis=1)
    np.testing.assert_array_equal(oy, om.greedy_decode(src, m, max_len=L, fault=f.as_dict(),
                                                       fault_step=step - 1))
    np.testing.assert_array_equal(ys, oy)
    np.testing.assert_array_equal(sc.top_ids, np.stack(oi, 1))
    np.testing.assert_array_equal(sc.top_logp, np.stack(ov, 1))
    r = sc.fault_step
    assert r is not None and r.step == step - 1
    np.testing.assert_array_equal(r.golden_ids, rec[0])
    np.testing.assert_array_equal(r.golden_logp, rec[1])
    np.testing.assert_array_equal(r.faulty_ids, rec[2])
    np.testing.assert_array_equal(r.faulty_logp, rec[3])
    np.testing.assert_array_equal(r.token_changed, rec[0][:, 0] != rec[2][:, 0])
    # the plain form is unchanged
    np.testing.assert_array_equal(
        greedy_decode_fault(gpu_model, src, m, L, 0, fault=f, target_inference_number=step), oy)


def test_encoder_fault_scored_decode(torch, gpu_model, oracle_model):
    from qtx import fault as F
    from qtx.decode import greedy_decode_fault
    rng = np.random.default_rng(13)
    B, S, L = 2, 16, 12
    src, m = make_src(rng, B, S, [16, 11])
    f = F.Fault("WEIGHT", 0, 2, "FFN2", row=17, col=100, bit=7)
    ys, sc = greedy_decode_fault(gpu_model, src, m, L, 0, fault=f, return_scores=True)
    assert sc.fault_step is None
    np.testing.assert_array_equal(ys, oracle_model.greedy_decode(src, m, max_len=L, fault=f.as_dict()))
    oy, oi, ov = oracle_scored_decode(oracle_model, src, m, L, fault=f.as_dict())
    np.testing.assert_array_equal(ys, oy)
    np.testing.assert_array_equal(sc.top_ids, oi)
    np.testing.assert_array_equal(sc.top_logp, ov)

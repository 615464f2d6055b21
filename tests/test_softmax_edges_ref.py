"""The rounding-edge rows of the attention softmax (tests/softmax_edges.py) on the oracle alone:
the construction holds, every tie k + 1/2 of the 1/127 grid is met from both sides, each wrong
model of the quotient, the exponential and the denominator changes the OUTPUT of the entry point
the rows are sent to (so tests/test_gpu_softmax_edges.py would fail a kernel that computes like
it), and the oracle's results equal a restatement of the two-key row written out below."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

from oracle import qtx_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import softmax_edges as E  # noqa: E402

f32 = np.float32
ALL = list(E.CASES)
EXACT = ("trace254", "i8_254x")
PAIRS = [n for n in ALL if n not in EXACT]
OP_DEC = {"trace": (False, True), "i8": (False, True), "i8_quant": (False,), "cross": (True,),
          "self": (True,)}
MIN_ROWS = 16


def grids(c):
    B, Sq = c["jA"].shape
    return np.arange(B)[:, None] + np.zeros((1, Sq), int), np.zeros((B, 1), int) + np.arange(Sq)[None, :]


# ------------------------------------------------------------------ the pools
@pytest.mark.parametrize("kind", ["op", "dec"])
def test_pool_meets_every_tie_from_both_sides(kind):
    p = E.pool(kind)
    code = np.where(p["key"] == 0, p["code_b"], p["code_a"])
    np.testing.assert_array_equal(code, p["tie"] + p["side"])
    assert set(p["code_a"] + p["code_b"]) <= {126, 127, 128}
    for tie in range(127):
        m = p["tie"] == tie
        for side in (0, 1):
            assert (m & (p["side"] == side) & p["near"]).sum() == 1, (tie, side)
            # (four floats are kept on each side of the flip; next to it the oracle's code
            # need not be monotone in the scale, so one of them may show the other side's code)
            assert (m & (p["side"] == side)).sum() >= 3, (tie, side)
    # the rows around a flip are neighbouring floats
    for tie in (0, 31, 62, 64, 100, 126):
        b = np.sort(p["t"][(p["tie"] == tie) & p["near"]].view(np.int32))
        assert b[1] - b[0] == 1


@pytest.mark.parametrize("kind", ["op", "dec"])
def test_pool_models(kind):
    """Every listed model gets rows of the pool wrong; exp+ / exp- together at every tie but
    EXP_BLIND."""
    p = E.pool(kind)
    assert (p["bad"].sum(0) >= 28).all(), dict(zip(E.MODELS, p["bad"].sum(0)))
    caught = set(p["tie"][p["bad"][:, 1] | p["bad"][:, 2]])
    assert set(range(127)) - caught == set(E.EXP_BLIND)


def test_exp_blind_ties_have_no_float():
    """P of a two-key row is a function of the float x = fl(score_B - score_A) alone.  At the
    ties EXP_BLIND, EVERY float x within WINDOW floats of the flip gives the oracle's code of the
    tie's key with the exponential one ulp up or down as well: no choice of scales can catch
    exp+- there (x steps over the tie by more than the models' reach).  (The other key's code
    does change near some of them: that is its own tie 126 - k, counted there.)"""
    for tie in E.EXP_BLIND:
        key = 0 if tie <= 63 else 1
        pred = (lambda c: c <= tie) if key == 0 else (lambda c: c > tie)
        # x < 0: the bit pattern grows with |x|, and so does A's code while B's falls
        flip = E._bisect(lambda x: bool(pred(E.pair_codes(x)[key])), E._bits(-1e-6), E._bits(-20.0))
        x = E._floats(np.arange(flip - E.WINDOW, flip + E.WINDOW))
        ref = E.pair_codes(x)
        assert len(set(ref[key])) == 2
        for m in ("exp+", "exp-"):
            got = E.pair_codes(x, m)
            np.testing.assert_array_equal(got[key], ref[key])


@pytest.mark.parametrize("kind", ["op", "dec"])
def test_div_cr_with_reciprocal_one_ulp_off_is_unobservable(kind):
    """Markstein's correction absorbs a reciprocal one ulp off: on every pool row div_cr gives
    the oracle's codes with RN(1 / den) and with either neighbour (so it is no listed model)."""
    p = E.pool(kind)
    x = E.pair_x(kind, p["t"], p["bsign"])
    e = np.stack([O.qexp(x), np.ones_like(x)], -1)
    den = (e[:, 0] + e[:, 1])[:, None]
    for step in (0, 1, -1):
        y = (f32(1.0) / den).astype(f32)
        if step:
            y = np.nextafter(y, f32(np.inf) if step > 0 else f32(0))
        q = (e * y).astype(f32)
        quot = O.fma32(O.fma32(-q, den, e), y, q)
        np.testing.assert_array_equal(np.rint(quot * f32(127.0))[:, 0], p["code_b"])
        np.testing.assert_array_equal(np.rint(quot * f32(127.0))[:, 1], p["code_a"])


def test_guard_rows():
    for kind in ("op", "dec"):
        e = O.qexp(E.pair_x(kind, E.guard_t(kind)))
        assert (e[:2] >= f32(2.0 ** -60)).all() and (e[2:4] < f32(2.0 ** -60)).all()
        assert (e[2:6] > 0).all() and (e[6:] == 0).all()
        cb, ca = E.pair_codes(E.pair_x(kind, E.guard_t(kind)))
        assert (cb == 0).all() and (ca == 127).all()


# ------------------------------------------------------------------ (a) the construction
@pytest.mark.parametrize("name", PAIRS)
def test_construction(name):
    c = E.case(name)
    v = c["view"]
    e = E.case_exps(name)
    B, H, Sq, Sk = e.shape
    b, i = grids(c)
    assert np.all(c["jA"] != c["jB"])
    ea, eb = e[b, :, i, c["jA"]], e[b, :, i, c["jB"]]           # [B, Sq, 8]
    assert np.all(ea == 1)
    dead = np.ones((B, Sq, Sk), bool)
    dead[b, i, c["jA"]] = dead[b, i, c["jB"]] = False
    assert np.all(e.transpose(0, 2, 3, 1)[dead] == 0)
    den = O.row_sum_lanesplit(e).transpose(0, 2, 1)
    np.testing.assert_array_equal(den, f32(1.0) + eb)
    assert np.all(np.abs(v["q"]) == 127)
    # the rows are the pool's: the codes of the live pair are the ones the sweep recorded
    p = E.pool(c["kind"])
    _, qp = E.expected(name, bool(c.get("dec", False)))
    s = c["src"]
    ok = s >= 0
    for h in range(8):
        np.testing.assert_array_equal(qp[b, h, i, c["jB"]][ok], p["code_b"][s[ok]])
        np.testing.assert_array_equal(qp[b, h, i, c["jA"]][ok], p["code_a"][s[ok]])
    assert (qp[b, 0, i, c["jB"]][~ok] == 0).all() and (qp[b, 0, i, c["jA"]][~ok] == 127).all()
    assert (~ok).sum() >= 8                                      # the guard rows
    if c["by_obs"]:       # the observed key's values are nonzero, the other live key's zero
        jo = np.where(c["obs"] == 1, c["jA"], c["jB"])
        jn = np.where(c["obs"] == 1, c["jB"], c["jA"])
        assert np.all(v["v"][b, jo] != 0) and np.all(v["v"][b, jn] == 0)
        assert np.all(v["sv"] > 0)
    if E.CASES[name][0] in ("cross", "self"):
        np.testing.assert_array_equal(v["sq"], E.SQ_DEC)         # y quantizes as intended
        qq, _ = O.quant_rows(c["raw"]["y"][:, :512])
        assert np.all(np.abs(qq) == 127)
    if E.CASES[name][0] == "self":
        n, it = c["step"], c["intended"]
        np.testing.assert_array_equal(c["after"]["kc"][:, n], it["kc"])
        np.testing.assert_array_equal(c["after"]["skc"][:, n], it["skc"])
        np.testing.assert_array_equal(c["after"]["vc"][:, n], it["vc"])
        assert np.all(np.abs(it["kc"]) == 127)
        new_a = c["jA"][:, 0] == n
        np.testing.assert_array_equal(new_a, it["new_a"])
        assert new_a.any() and (n < 2 or (~new_a).any())
        assert (c["jB"] < n).all()


# ------------------------------------------------------------------ (b) every tie, both sides
@pytest.mark.parametrize("name", PAIRS)
def test_every_tie_on_both_sides(name):
    c = E.case(name)
    p = E.pool(c["kind"])
    s = np.unique(c["src"][c["src"] >= 0])
    have = set(zip(p["tie"][s], p["side"][s]))
    assert have == {(t, sd) for t in range(127) for sd in (0, 1)}
    near = set(zip(p["tie"][s[p["near"][s]]], p["side"][s[p["near"][s]]]))
    assert near == have                                          # the floats next to the flip


# ------------------------------------------------------------------ (c) discrimination
@pytest.mark.parametrize("name", PAIRS)
def test_wrong_models_change_the_output(name):
    entry = E.CASES[name][0]
    c = E.case(name)
    p = E.pool(c["kind"])
    src = c["src"]
    for dec in OP_DEC[entry]:
        counts, exp_ties = {}, set()
        for m in E.MODELS:
            ch = E.changed_rows(name, m, dec, E.OUTPUT[entry])
            rows = np.unique(src[ch & (src >= 0)])
            counts[m] = len(rows)
            if m in ("exp+", "exp-"):
                exp_ties |= set(p["tie"][rows])
            # what changes is what the sweep predicted for the observed key (the trace sees
            # both keys' codes)
            if c["by_obs"]:
                want = np.unique(src[(src >= 0)])
                want = want[p["bad"][want, E.MODELS.index(m)]]
                np.testing.assert_array_equal(rows, want)
        print(name, "dec", int(dec), "rows", len(np.unique(src[src >= 0])), counts)
        for m in E.COUNTED:
            assert counts[m] >= MIN_ROWS, (name, m, counts)
        assert counts["fused"] >= MIN_ROWS, (name, counts)
        if c["by_obs"]:
            assert exp_ties == set(range(127)) - set(E.EXP_BLIND), name
        else:             # both keys' codes are seen: a row also catches its other key's tie
            assert exp_ties >= set(range(127)) - set(E.EXP_BLIND), name


@pytest.mark.parametrize("name", ["i8_20", "encq16", "self1"])
def test_changed_rows_equal_the_patched_oracle(name):
    """changed_rows puts only the rows with changed codes through the PV chain again; on the
    cheap cases the same answer comes from the whole oracle with O.softmax_quant replaced."""
    entry = E.CASES[name][0]
    v = E.case(name)["view"]
    dec = OP_DEC[entry][-1]
    ctx = E.expected(name, dec)[0]
    for m in E.MODELS:
        with E.patched(m):
            got, _ = O.attention(v["q"], v["sq"], v["k"], v["sk"], v["v"], v["sv"], v["mask"], 8,
                                 dec=dec)
        assert O.softmax_quant.__module__ == O.__name__
        if E.OUTPUT[entry] == "quant":
            (qa, sa), (qb, sb) = O.quant_rows(got), O.quant_rows(ctx)
            ch = (qa != qb).any(-1) | (sa != sb)
        else:
            ch = (got != ctx).any(-1)
        np.testing.assert_array_equal(ch, E.changed_rows(name, m, dec, E.OUTPUT[entry]))


def test_exact_ties():
    """n = 2: p * 127 == 63.5, both codes 64 (rounding half away gives 64 too: 127 / n is a tie
    only for n = 2 and n = 254, and only the latter tells the two roundings apart).  n = 254 and
    the fully masked row: RN(1 / 254) * 127 is 0.5 in fp32, code 0; rounding half away or a
    quotient one ulp high gives 1 on all 254 keys."""
    assert [n for n in range(1, 600) if (Fraction(127, n) * 2).denominator == 1
            and (Fraction(127, n) * 2).numerator % 2 == 1] == [2, 254]
    assert (f32(1.0) / f32(254.0)) * f32(127.0) == f32(0.5)
    assert np.nextafter(f32(1.0) / f32(254.0), f32(1)) * f32(127.0) > f32(0.5)
    for name in EXACT:
        c = E.case(name)
        n = c["n"][0]
        for dec in (False, True):
            _, qp = E.expected(name, dec)
            e = E.case_exps(name)
            assert set(np.unique(e)) == {0.0, 1.0}
            np.testing.assert_array_equal(e.sum(-1), np.broadcast_to(n[None, None], e.shape[:3]))
            for i, ni in enumerate(n):
                live = qp[0, :, i][e[0, :, i] == 1]
                assert np.all(live == (64 if ni == 2 else 0)) and live.size == 8 * ni
            out = E.OUTPUT[E.CASES[name][0]]
            for m in E.EXACT_MODELS:
                ch = E.changed_rows(name, m, dec, out)[0]
                np.testing.assert_array_equal(ch, n == 254)
                assert ch.sum() >= 4


# ------------------------------------------------------------------ (d) the restatement
@pytest.mark.parametrize("name", PAIRS)
def test_oracle_equals_two_key_restatement(name):
    """qexp, the two-term sum, IEEE division and np.rint, spelled out for the two-key row: the
    expectations the GPU test uses do not rest on the general oracle path alone."""
    entry = E.CASES[name][0]
    c = E.case(name)
    v = c["view"]
    b, i = grids(c)
    B, Sq = b.shape
    Sk = v["k"].shape[1]

    def score(j):
        q0, k0 = v["q"][:, :, :64].astype(np.int64), v["k"][:, :, :64].astype(np.int64)   # head 0
        acc = (q0[b, i] * k0[b, j]).sum(-1)
        assert np.all(np.abs(acc) == E.ACC)
        return ((acc.astype(f32) * v["sq"]) * v["sk"][b, j]) / f32(8.0)

    sa, sb = score(c["jA"]), score(c["jB"])
    assert np.all(sb <= sa)
    eb = O.qexp((sb - sa).astype(f32))
    den = f32(1.0) + eb
    cb = np.rint((eb / den) * f32(127.0))
    ca = np.rint((f32(1.0) / den) * f32(127.0))
    codes = np.zeros((B, 8, Sq, Sk), np.int8)
    for h in range(8):
        codes[b, h, i, c["jA"]] = ca
        codes[b, h, i, c["jB"]] = cb
    for dec in OP_DEC[entry]:
        ctx, qp = E.expected(name, dec)
        np.testing.assert_array_equal(qp, codes)
        if not c["by_obs"]:
            continue
        jo = np.where(c["obs"] == 1, c["jA"], c["jB"])
        pr = (np.where(c["obs"] == 1, ca, cb).astype(f32) / f32(127.0))[..., None]
        vo, svo = v["v"][b, jo].astype(f32), v["sv"][b, jo][..., None]
        want = ((pr * svo).astype(f32) * vo if dec else pr * (vo * svo).astype(f32)) + f32(0.0)
        np.testing.assert_array_equal(ctx, want.astype(f32))


# ------------------------------------------------------------------ slot coverage
def _slots(names, key):
    js = np.concatenate([E.case(n)[key].reshape(-1) for n in names])
    return {(j // 16, (j % 16) // 4, j % 4) for j in js}


@pytest.mark.parametrize("names", [("i8_128",), ("i8_guard",), ("encq128",)])
def test_mfma_slots(names):
    """k_attn_mfma / k_attn_encq hold key 16 kt + 4 e + fg in register (kt, e) of lane group
    fg: every kt, e and fg holds key A somewhere and key B somewhere."""
    for key in ("jA", "jB"):
        s = _slots(names, key)
        assert {a for a, _, _ in s} == set(range(8))
        assert {e for _, e, _ in s} == set(range(4)) and {g for _, _, g in s} == set(range(4))


def test_partial_tile_and_small_slots():
    for key in ("jA", "jB"):
        assert len({j for j in E.case("i8_20")[key].reshape(-1)}) >= 8
        assert {j for j in E.case("i8_20")[key].reshape(-1)} & {16, 17, 18, 19}
        assert len({j for j in E.case("encq16")[key].reshape(-1)}) == 16


@pytest.mark.parametrize("name", E.names("cross") + E.names("self"))
def test_decode_slots(name):
    """k_dec_attn: a lane's first and second key slot, the last key and the last 16-group."""
    c = E.case(name)
    S = c["view"]["k"].shape[1]
    for key in ("jA", "jB"):
        js = set(c[key].reshape(-1))
        if name.startswith("self") and key == "jB":
            S_ = S - 1                    # key B is a cached key
        else:
            S_ = S
        assert S_ - 1 in js
        assert any(j >= 16 * ((S_ - 1) // 16) for j in js)
        assert any(j < 64 for j in js) and (S_ <= 64 or any(j >= 64 for j in js))


def test_guard_rows_as_wave_neighbours():
    """k_attn_mfma votes its division per wave of 16 queries: an e outside (2^-60, 2^60) sends the
    whole wave to the true division.  In "i8_guard" every wave holds such a row next to its tie
    rows; in "i8_128" only the waves with the appended guard rows do."""
    for name, every in (("i8_guard", True), ("i8_128", False)):
        e = E.case_exps(name)[:, 0]
        slow = ((e > 0) & (e < f32(2.0 ** -60))).any(-1)
        ties = E.case(name)["src"] >= 0
        B, Sq = slow.shape
        waves = [(slow[b, w:w + 16].any(), ties[b, w:w + 16].sum()) for b in range(B)
                 for w in range(0, Sq, 16)]
        assert all(n >= 8 for s, n in waves if s)
        assert all(s for s, _ in waves) if every else 0 < sum(s for s, _ in waves) < len(waves)

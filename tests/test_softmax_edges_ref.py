"""The rounding-edge rows of the attention softmax (tests/softmax_edges.py) on the oracle alone:
the construction holds, every tie k + 1/2 of the 1/127 grid is met from both sides, each wrong
model of the quotient, the exponential and the denominator changes the OUTPUT of the entry point
the rows are sent to (so tests/test_gpu_softmax_edges.py would fail a kernel that computes like
it), and the oracle's results equal a restatement of the two-key row written out below.  Past
128 keys: where the pair lies among k_dec_attn_long's four waves, the exact ties at 254 and 512
keys, and the order cases, on which every wrong order of the denominator's sum changes the
output of at least 16 rows."""
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
PAIRS = [n for n in ALL if n not in EXACT + E.EXACT_DEC + E.ORDER]
LONG_PAIRS = [n for n in PAIRS if E.CASES[n][0] in ("cross", "self") and n not in E.OLD_18]
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


@pytest.mark.parametrize("name", [n for n in PAIRS if E.CASES[n][0] in ("cross", "self")])
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


# ------------------------------------------------------------------ k_dec_attn_long: the pairs
def test_short_pairs_are_what_they_were():
    """Up to 128 keys _dec_slots / _dec_pair return what they returned before the long cases
    existed (restated here), so the k_dec_attn cases and their expectations did not move."""
    def slots(S):
        c = {0, 1, 5, 15, 16, 31, 47, 48, 63, 64, 65, 69, 100, 127, S - 1, S - 2, 16 * ((S - 1) // 16)}
        return np.array(sorted(j for j in c if 0 <= j < S))

    def pair(B, S):
        c, b = slots(S), np.arange(B)
        if len(c) == 1:
            return c[b * 0], c[b * 0]
        return c[b % len(c)], c[(b + 1 + (b // len(c)) % (len(c) - 1)) % len(c)]

    for S in range(1, 129):
        np.testing.assert_array_equal(E._dec_slots(S), slots(S))
        for B in (1, 17, 288, 512):
            for got, want in zip(E._dec_pair(B, S), pair(B, S)):
                np.testing.assert_array_equal(got, want)
    for name in ("cross17", "cross64", "cross65", "cross128"):
        c = E.case(name)
        B, S = c["raw"]["mask"].shape
        np.testing.assert_array_equal(c["jA"][:, 0], pair(B, S)[0])
        np.testing.assert_array_equal(c["jB"][:, 0], pair(B, S)[1])
    assert len(E.OLD_18) == 18 and E.OLD_18[-1] == "self127" and not set(E.OLD_18) & set(LONG_PAIRS)


def _long_slots(S):
    """What the pair of a long case must visit: in every wave's block the first and last key of
    both lane slots and a fragment border, the last two keys and the last 16-group's first."""
    c = {S - 1, S - 2, 16 * ((S - 1) // 16)}
    for w in range((S + 127) // 128):
        c |= {128 * w + j for j in (0, 63, 64, 127, 15, 16)}
    return {j for j in c if j < S}


@pytest.mark.parametrize("name", LONG_PAIRS)
def test_long_pairs(name):
    """The rows to load are past 128 (k_dec_attn_long serves the case); each of key A and key B
    visits every slot of every wave's block; in at least a third of the sentences the two lie in
    different waves' blocks (the maximum and both exponentials cross LDS), in at least a sixth
    in the same one."""
    c = E.case(name)
    jA, jB = c["jA"][:, 0], c["jB"][:, 0]
    if E.CASES[name][0] == "self":
        n = c["step"] + 1
        assert c["kv_bs"] == 512 and c["step"] >= 128
        want_b = _long_slots(c["step"]) if c["step"] > 128 else set(E._dec_slots(128))
        want_a = want_b | {c["step"]}                    # the cached slots and the new key
        if name == "self128":
            assert (jA[::2] == 128).all() and (jA[::2] >> 7 == 1).all()   # the second wave's first key
    else:
        n = c["raw"]["mask"].shape[1]
        want_a = want_b = _long_slots(n)
    assert 128 < n <= 512
    assert set(jA) >= want_a, sorted(want_a - set(jA))
    assert set(jB) >= want_b, sorted(want_b - set(jB))
    far = (jA >> 7) != (jB >> 7)
    print(name, "different waves %.3f, the same wave %.3f" % (far.mean(), 1 - far.mean()))
    assert far.mean() >= 1 / 3 and (~far).mean() >= 1 / 6


# ------------------------------------------------------------------ the exact ties, decode
@pytest.mark.parametrize("name", E.EXACT_DEC)
def test_exact_ties_decode(name):
    """The rule of test_exact_ties at qtx_decode_attention: the fully masked sentence and the
    one of S equal live keys have p = 1 / S on every key (S = 254: p * 127 == 0.5, code 0, context
    0; half away or a quotient one ulp high gives 1 everywhere), two equal keys in different
    waves' blocks 64 / 64.  S = 512: den == 512, the largest denominator the kernel can meet."""
    c = E.case(name)
    n = c["n"][:, 0]
    S = c["raw"]["mask"].shape[1]
    ctx, qp = E.expected(name, True)
    e = E.case_exps(name)
    assert set(np.unique(e)) == {0.0, 1.0}
    np.testing.assert_array_equal(O.row_sum_lanesplit(e)[:, :, 0], np.repeat(n[:, None], 8, 1))
    for b, nb in enumerate(n):
        live = qp[b, :, 0][e[b, :, 0] == 1]
        assert live.size == 8 * nb and np.all(live == (64 if nb == 2 else 0))
        if nb == 2:
            j = np.flatnonzero(c["raw"]["mask"][b])
            assert j[0] >> 7 != j[1] >> 7
        else:
            assert not ctx[b].any()
    assert (n == S).sum() >= 2 and (n == 2).any()
    assert (c["raw"]["mask"].sum(-1) == 0).any() and (c["raw"]["mask"].sum(-1) == S).any()
    for m in E.EXACT_MODELS:
        ch = E.changed_rows(name, m, True, "ctx")[:, 0]
        np.testing.assert_array_equal(ch, n == 254)
        assert ch.sum() >= (4 if S == 254 else 0)


# ------------------------------------------------------------------ the denominator's order
def test_random_rows_are_blind_to_the_order():
    """Why the order cases exist: on random rows the wrong orders move the denominator by an ulp
    in a third to nine tenths of the rows and a code in next to none."""
    rng = np.random.default_rng(5)
    e = E.exps(rng.standard_normal((4000, 512)).astype(f32))
    ref = E.codes_from(e)
    for m, lo in (("wave_sums", 0.25), ("sequential", 0.7), ("f64", 0.2)):
        den = E.ORDER_TOTALS[m](e) != O.row_sum_lanesplit(e)
        rows = (E.codes_from(e, m) != ref).any(-1)
        print(m, "denominators %.3f, rows with another code %d of %d" % (den.mean(), rows.sum(), len(e)))
        assert den.mean() > lo and rows.sum() <= 2


@pytest.mark.parametrize("name", E.ORDER)
def test_order_cases(name):
    """Every wrong order of the denominator's sum that applies to the case changes the OUTPUT of
    at least MIN_ROWS of its rows, and exactly the rows whose code of key B the sweep saw it get
    wrong; the oracle's codes are the sweep's; key B alone carries values."""
    entry = E.CASES[name][0]
    c = E.case(name)
    v = c["view"]
    models = c["order_models"]
    assert models == (E.ORDER_MODELS[1:] if name == "cross128_order" else E.ORDER_MODELS)
    B, S = v["k"].shape[:2]
    b = np.arange(B)
    jA, jB = c["jA"][:, 0], c["jB"][:, 0]
    e = E.case_exps(name)[:, :, 0]                                # [B, 8, S]
    ctx, qp = E.expected(name, True)
    assert np.all(e[b, :, jA] == 1) and np.all(e[b, :, jB] < 1)
    np.testing.assert_array_equal(qp[b, :, 0, jB], np.repeat(c["code_b"][:, None], 8, 1))
    dust = (e[:, 0] > 0) & (e[:, 0] < 1)
    dust[b, jB] = False
    assert (dust.sum(-1) >= 40).all()
    ed = e[:, 0][dust]
    assert ed.min() > np.exp(-7.01) and ed.max() < np.exp(-1.99)
    # the dust is spread over the lanes and over every wave's block that has 16 keys or more
    for i in range(c["n_layouts"]):
        j = np.flatnonzero(dust[np.flatnonzero(c["layout"] == i)[0]])
        assert len(set(j % 64)) >= 25 and set(j >> 7) >= {w for w in range(4) if S >= 128 * w + 16}
        sk = v["sk"][np.flatnonzero(c["layout"] == i)[0]][j]
        assert len(set(sk)) == len(j)                             # a scale of its own
    assert np.all(v["v"][b, jB] != 0) and np.all(v["sv"] > 0)
    live = e[:, 0] > 0
    live[b, jB] = False
    assert not v["v"][live].any()
    if entry == "self":
        assert c["step"] == 511 and c["kv_bs"] == 512
        new_a = jA == c["step"]
        assert new_a.any() and (~new_a).any()
        assert np.all(v["sk"][~live & (np.arange(S) != jB[:, None])] == E.SK_DEAD)
    counts = {}
    for k, m in enumerate(models):
        ch = E.changed_rows(name, m, True, "ctx")[:, 0]
        np.testing.assert_array_equal(ch, c["bad"][:, k])
        counts[m] = int(ch.sum())
    print(name, "rows", B, "layouts", c["n_layouts"], "ties", len(set(c["tie"])), counts)
    assert all(n >= MIN_ROWS for n in counts.values()), counts
    assert c["bad"].any(-1).all()                                 # no row without a purpose
    if name == "cross128_order":      # two lane rounds in one wave: per-wave sums are the canon
        assert not E.changed_rows(name, "wave_sums", True, "ctx").any()


def test_order_rows_equal_the_patched_oracle():
    """On the cheapest order case the same rows change when the whole oracle runs with
    O.softmax_quant replaced by the wrong order."""
    name = "cross128_order"
    v = E.case(name)["view"]
    ctx = E.expected(name, True)[0]
    for m in E.ORDER_MODELS:
        with E.patched(m):
            got, _ = O.attention(v["q"], v["sq"], v["k"], v["sk"], v["v"], v["sv"], v["mask"], 8, dec=True)
        np.testing.assert_array_equal((got != ctx).any(-1), E.changed_rows(name, m, True, "ctx"))

"""tests/kvfault_ref.py, the contract of qtx_greedy_decode_kvfault, pinned to the pinned oracle
(CPU only): where the cached semantics must coincide with something the oracle already states,
it does; where it must differ from the campaign semantics, it does; and the GPU cases of
tests/kvfault_cases.py cover token changers, score changers and a fault without effect.
"""
import dataclasses
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dfault_cases as D  # noqa: E402
import kvfault_cases as K  # noqa: E402
import kvfault_ref as R  # noqa: E402

L = D.L


@pytest.fixture(scope="module")
def inp():
    return D.make_src()


def run(om, inp, fault=None, upset=None, step=0):
    return R.trial(om, inp[0], inp[1], L, "main", fault, upset, step)


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def test_no_fault_is_the_oracles_decode(oracle_model, inp):
    g = R.golden(oracle_model, inp[0], inp[1], L, "main")
    np.testing.assert_array_equal(g["ys"], oracle_model.greedy_decode(inp[0], inp[1], max_len=L))
    np.testing.assert_array_equal(g["top_ids"][:, :, 0], g["ys"][:, 1:])
    never = run(oracle_model, inp, *K.cases()["never"][:2], step=L - 1)
    assert never[3] is None
    np.testing.assert_array_equal(never[0], g["ys"])


@pytest.mark.parametrize("name", ["out_ffn2_l5_s2", "in_co_l5_s3"])
def test_behind_the_kv_projections_equals_the_campaign(oracle_model, inp, name):
    """A last-layer target behind the K/V projections leaves the caches golden, so the ids are
    the campaign loop's with the fault's row moved to the sentence's last prefix position."""
    f, _, i = K.cases()[name]
    b = f.row
    fc = dataclasses.replace(f, row=b * (i + 1) + i)
    want = oracle_model.greedy_decode(inp[0], inp[1], max_len=L, fault=fc.as_dict(), fault_step=i)
    got = run(oracle_model, inp, f, None, i)
    np.testing.assert_array_equal(got[0], want)
    assert R.effect(oracle_model, inp[0], inp[1], L, "main", got) == "tokens"


@pytest.mark.parametrize("cache", ["self_k", "self_v", "cross_k", "cross_v"])
def test_last_step_upset_equals_the_transient_weight_fault(oracle_model, inp, cache):
    pairs, i = K.identity_pairs()
    assert i == L - 2
    u, f = pairs[cache]
    a, b = run(oracle_model, inp, None, u, i), run(oracle_model, inp, f, None, i)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    np.testing.assert_array_equal(bits(a[2]), bits(b[2]))
    for x, y in zip(a[3], b[3]):
        np.testing.assert_array_equal(x, y)
    assert R.effect(oracle_model, inp[0], inp[1], L, "main", a) != "none"


def test_a_cached_fault_persists(oracle_model, inp):
    """A V-projection fault in a lower layer: the scores differ from golden at steps after
    the faulty one, and the ids from the campaign semantics' (which recomputes the row)."""
    f, _, i = K.cases()["in_v_l2_s2"]
    g = R.golden(oracle_model, inp[0], inp[1], L, "main")
    got = run(oracle_model, inp, f, None, i)
    later = (bits(got[2]) != bits(g["top_logp"])).any((0, 2))
    assert later[i + 1:].any() and not later[:i].any()
    fc = dataclasses.replace(f, row=f.row * (i + 1) + i)
    camp = oracle_model.greedy_decode(inp[0], inp[1], max_len=L, fault=fc.as_dict(), fault_step=i)
    assert not np.array_equal(got[0], camp)
    # RANDOM on QK^T at step 4: the same ids, but the cached decode's scores keep differing
    f, _, i = K.cases()["rand_qk_s4"]
    got = run(oracle_model, inp, f, None, i)
    np.testing.assert_array_equal(got[0], g["ys"])
    later = (bits(got[2]) != bits(g["top_logp"])).any((0, 2))
    assert later[i:].all() and not later[:i].any()


def test_gpu_cases_cover(oracle_model, inp):
    """Among the GPU cases some change tokens, some only scores, and the padded-key upset,
    the missed window and the never-applied trials change nothing."""
    eff = {n: R.effect(oracle_model, inp[0], inp[1], L, "main", run(oracle_model, inp, f, u, s))
           for n, (f, u, s) in K.cases().items()}
    for n in ("up_ck_pad", "w16_cpv_miss", "never", "up_never"):
        assert eff[n] == "none", n
    assert all(e != "none" for n, e in eff.items()
               if n not in ("up_ck_pad", "w16_cpv_miss", "never", "up_never")), eff
    faults = [e for n, e in eff.items() if not n.startswith("up_")]
    upsets = [e for n, e in eff.items() if n.startswith("up_")]
    for group in (faults, upsets):
        assert "tokens" in group and "scores" in group
    # the cells the path tests rely on
    assert eff["cv_s0"] == "tokens" and eff["up_cv_last"] != "none" and eff["up_sv_j3"] == "tokens"

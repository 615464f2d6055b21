"""The trials shared by tests/test_kvfault_ref.py (CPU) and tests/test_gpu_kvfault.py (GPU): step
faults and cache upsets of the KV-cached decode at tests/dfault_cases.py's shapes (B = 3, S = 14
with lengths 14 / 9 / 12, max_len = 8).  A helper module, not a conftest.  Expected values come
from tests/kvfault_ref.py, never from the code under test.
"""
from dfault_cases import B, L, S  # noqa: F401


def cases():
    """name -> (Fault or None, CacheUpset or None, step).  Step-fault rows index the step's
    [B] tokens (attention: Sq = 1, Sk = step + 1 self keys or S cross keys)."""
    from qtx.fault import CacheUpset as U
    from qtx.fault import Fault as F
    c = {
        # ---- linear targets ---------------------------------------------------------------
        # a K projection of the lowest layer: the row stays in the cache of every layer
        "out_k_l0_s1": F("OUTPUT", 1, 0, "K", row=0, col=100, value=50.0),
        "in_v_l2_s2": F("INPUT", 1, 2, "V", row=1, col=50, bit=7),
        # the first step, every row
        "w_k_l1_s0": F("WEIGHT", 1, 1, "K", row=77, col=300, bit=7),
        "out_ffn2_l0_s2": F("OUTPUT", 1, 0, "FFN2", row=2, col=100, value=3.0e4),
        # window rows 0..1 of the step's [B] rows
        "w16_ffn1_s3": F("WEIGHT16", 1, 3, "FFN1", row=7, col=100, bit=7, win_start=0, win_len=2),
        "in16_o_s2": F("INPUT16", 1, 2, "O", row=1, col=40, bit=7, win_start=32, win_len=16),
        # the one-time memory K/V projection (rows [B * S])
        "ck_s0": F("WEIGHT", 1, 1, "CK", row=40, col=200, bit=7),
        "cv_s0": F("INPUT", 1, 0, "CV", row=1 * S + 3, col=17, bit=7),
        # last layer, behind the K/V projections: the caches stay golden
        "out_ffn2_l5_s2": F("OUTPUT", 1, 5, "FFN2", row=0, col=100, value=3.0e4),
        "in_co_l5_s3": F("INPUT", 1, 5, "CO", row=1, col=9, bit=7),
        "last_step": F("OUTPUT", 1, 5, "FFN2", row=0, col=100, value=3.0e4),
        "never": F("OUTPUT", 1, 5, "FFN2", row=0, col=100, value=3.0e4),
        # ---- attention targets at Sq = 1 ----------------------------------------------------
        # sentence 2, head 3, key 2 of 5
        "rand_qk_s4": F("RANDOM", 1, 0, "QK", row=2, col=3 * 5 + 2, value=1.0e4),
        # sentence 0, head 1, key 3 of 6
        "in_pv_s5": F("INPUT", 1, 4, "PV", row=0, col=1 * 6 + 3, bit=5),
        # key 5 of 6 (5 % 4 == 1: inside a 4-key value group), sentence 1
        "w_pv_s5_j5": F("WEIGHT", 1, 2, "PV", row=1 * 6 + 5, col=2 * 64 + 7, bit=7),
        # the sentence padded to 9 (masked keys)
        "in_cqk_s3": F("INPUT", 1, 1, "CQK", row=1, col=4 * 64 + 9, bit=7),
        "w16_cpv_s2": F("WEIGHT16", 1, 3, "CPV", row=1 * S + 6, col=5 * 64 + 3, bit=7,
                        win_start=0, win_len=1),
        # a window that misses the step's only query row: no effect
        "w16_cpv_miss": F("WEIGHT16", 1, 3, "CPV", row=1 * S + 6, col=5 * 64 + 3, bit=7,
                          win_start=1, win_len=3),
        # key counts 1 and 4 (5: rand_qk_s4): either side of the first group boundary
        "w_pv_s0": F("WEIGHT", 1, 0, "PV", row=0, col=5, bit=7),
        "in16_qk_s3": F("INPUT16", 1, 2, "QK", row=0, col=70, bit=7, win_start=0, win_len=4),
    }
    steps = {"out_k_l0_s1": 1, "in_v_l2_s2": 2, "w_k_l1_s0": 0, "out_ffn2_l0_s2": 2,
             "w16_ffn1_s3": 3, "in16_o_s2": 2, "ck_s0": 0, "cv_s0": 0, "out_ffn2_l5_s2": 2,
             "in_co_l5_s3": 3, "last_step": L - 2, "never": L - 1, "rand_qk_s4": 4,
             "in_pv_s5": 5, "w_pv_s5_j5": 5, "in_cqk_s3": 3, "w16_cpv_s2": 2, "w16_cpv_miss": 2,
             "w_pv_s0": 0, "in16_qk_s3": 3}
    out = {n: (f, None, steps[n]) for n, f in c.items()}
    ups = {
        "up_sk": (U("self_k", 0, row=0 * L + 1, col=33, bit=7), 3),
        # both sides of a 4-key group: j = 3 (j % 4 == 3) and j = 5 (j % 4 == 1)
        "up_sv_j3": (U("self_v", 1, row=1 * L + 3, col=70, bit=7), 5),
        "up_sv_j5": (U("self_v", 2, row=2 * L + 5, col=200, bit=7), L - 2),
        "up_ck": (U("cross_k", 0, row=0 * S + 4, col=10, bit=7), 2),
        # the last key, in a ragged group (S = 14)
        "up_cv_last": (U("cross_v", 2, row=0 * S + 13, col=300, bit=7), 0),
        # a padded source position of sentence 1: masked, no effect
        "up_ck_pad": (U("cross_k", 0, row=1 * S + 12, col=10, bit=7), 1),
        # the smallest step
        "up_sk_scale22": (U("self_k", 0, row=0 * L + 0, bit=22, field="scale"), 1),
        "up_sv_scale31": (U("self_v", 3, row=1 * L + 2, bit=31, field="scale"), 4),
        "up_cv_scale31": (U("cross_v", 1, row=2 * S + 5, bit=31, field="scale"), 2),
        "up_never": (U("self_k", 0, row=0 * L + 1, col=33, bit=7), L - 1),
    }
    out.update({n: (None, u, s) for n, (u, s) in ups.items()})
    return out


# an upset effective at the last step and the transient attention WEIGHT fault on the same
# element at that step: the same result (self K <-> QK, self V <-> PV, cross K <-> CQK,
# cross V <-> CPV)
def identity_pairs():
    from qtx.fault import CacheUpset as U
    from qtx.fault import Fault as F
    i = L - 2
    Sk = i + 1
    return {
        "self_k": (U("self_k", 0, row=2 * L + 3, col=1 * 64 + 5, bit=7),
                   F("WEIGHT", 1, 0, "QK", row=2 * Sk + 3, col=1 * 64 + 5, bit=7)),
        "self_v": (U("self_v", 5, row=0 * L + 5, col=6 * 64 + 1, bit=7),
                   F("WEIGHT", 1, 5, "PV", row=0 * Sk + 5, col=6 * 64 + 1, bit=7)),
        "cross_k": (U("cross_k", 4, row=1 * S + 2, col=3 * 64 + 60, bit=7),
                    F("WEIGHT", 1, 4, "CQK", row=1 * S + 2, col=3 * 64 + 60, bit=7)),
        "cross_v": (U("cross_v", 5, row=2 * S + 7, col=0 * 64 + 31, bit=7),
                    F("WEIGHT", 1, 5, "CPV", row=2 * S + 7, col=0 * 64 + 31, bit=7)),
    }, i

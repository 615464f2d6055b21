"""Self-attention's q / k / v per-token scales and codes formed in one pass (k_dec_attn<true, *>,
csrc/qtx_decode.hip: three row maxima through one reduction, the three scales behind one
range test, the three codes behind one near-tie vote), through qtx_decode_attention against
the oracle, bit for bit: the appended cache row, both appended scales, the context and the
head maxima.  The three row maxima sit in different lanes, and each slow path — a row
maximum >= 2^60 (the scale's true division) and a quantizer near-tie (the code's true
division, tests/rounding_edges.py) — is triggered in q only, in k only, in v only and in all
three, next to a sentence that triggers nothing."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rounding_edges as E  # noqa: E402
from test_gpu_dec_attn_mfma import _release, caches, run_self, torch  # noqa: E402,F401

pytestmark = pytest.mark.gpu
f32 = np.float32
B, STEP, KV_BS = 3, 21, 40
# column of each third's maximum per sentence: lane (col / 4) % 64 differs between q, k and v
PEAK = {"q": (4 * 5, 256 + 4 * 40 + 1, 4 * 63 + 3), "k": (256 + 4 * 23 + 1, 4 * 2 + 2, 4 * 17),
        "v": (4 * 60 + 3, 4 * 31, 256 + 4 * 9 + 2)}
THIRD = {"q": 0, "k": 512, "v": 1024}


def base_y(rng):
    y = rng.standard_normal((B, 1536)).astype(f32)
    for t, cols in PEAK.items():
        for b, c in enumerate(cols):
            y[b, THIRD[t] + c] = f32(5.5 + b) * (-1) ** b
    return y


def test_maxima_in_different_lanes(torch):
    rng = np.random.default_rng(1)
    y = base_y(rng)
    lanes = {t: [(np.abs(y[b, o:o + 512]).argmax() // 4) % 64 for b in range(B)] for t, o in THIRD.items()}
    assert all(len({lanes["q"][b], lanes["k"][b], lanes["v"][b]}) == 3 for b in range(B))
    run_self(torch, y, *caches(rng, B, KV_BS), STEP)


@pytest.mark.parametrize("which", ["q", "k", "v", "qkv"])
def test_maximum_from_2_60(torch, which):
    """Sentence 0: the third's maximum exactly 2^60 (the first value of the slow path);
    sentence 2: 1.5 * 2^61 under values of ~1e15; sentence 1 triggers nothing."""
    rng = np.random.default_rng(60 + len(which) + ord(which[0]))
    y = base_y(rng)
    for t in which:
        o = THIRD[t]
        y[0, o + PEAK[t][0]] = f32(2.0 ** 60)
        y[2, o:o + 512] *= f32(1e15)
        y[2, o + PEAK[t][2]] = -f32(1.5 * 2.0 ** 61)
    run_self(torch, y, *caches(rng, B, KV_BS), STEP)


@pytest.mark.parametrize("which", ["q", "k", "v", "qkv"])
def test_quantizer_near_tie(torch, which):
    """Lone rows (one element near a rounding tie, one that the reciprocal product gets
    wrong) in sentences 0 and 2 of the chosen thirds: only the head that holds the element
    votes for the true division.  The other thirds keep their random rows."""
    rng = np.random.default_rng(70 + len(which) + ord(which[0]))
    y = base_y(rng)
    lone = E.decode_y(B, lone=True)
    for t in which:
        o = THIRD[t]
        y[0, o:o + 512] = lone[0, o:o + 512]
        y[2, o:o + 512] = lone[2, o:o + 512]
    run_self(torch, y, *caches(rng, B, KV_BS), STEP)


def test_both_triggers_in_different_thirds(torch):
    """q's maximum >= 2^60 while k holds the near-tie and v neither, and the rotations."""
    rng = np.random.default_rng(80)
    lone = E.decode_y(B, lone=True)
    y = base_y(rng)
    for b, (big, tie) in enumerate((("q", "k"), ("k", "v"), ("v", "q"))):
        y[b, THIRD[big] + PEAK[big][b]] = f32(2.0 ** 62)
        o = THIRD[tie]
        y[b, o:o + 512] = lone[b, o:o + 512]
    run_self(torch, y, *caches(rng, B, KV_BS), STEP)

"""CPU: the head counts qtx_model_create accepts, and include/qtx_heads.h's symbols."""
import os

import pytest

from qtx import _build, _lib


@pytest.mark.parametrize("n_heads,ok", [(4, True), (8, True), (16, True), (2, False), (32, False), (6, False)])
def test_tensor_count_head_counts(n_heads, ok):
    c = _lib.QtxConfig(64, 97, 2, 512, 512, n_heads, 64, 8)
    n = _lib.lib().qtx_model_tensor_count(c)
    assert (n == 12 * 2 + 20 * 2 + 2 * (2 * 2 + 1 + 3 * 2 + 1) + 4) if ok else n == -1
    if not ok:
        assert b"d_model" in _lib.lib().qtx_last_error()


def test_heads_header_matches_table():
    names = _lib.header_symbols(os.path.join(_build.REPO, "include", "qtx_heads.h"))
    assert set(names) == set(_lib.SIGNATURES_HEADS) == {"qtx_attention_heads_i8", "qtx_decode_attention_heads"}
    others = {**_lib.SIGNATURES, **_lib.SIGNATURES_ENCTRIALS, **_lib.SIGNATURES_BEAM_LONG,
              **_lib.SIGNATURES_WIDE_VOCAB}
    assert not set(names) & set(others)
    L = _lib.lib()
    for n in names:
        assert getattr(L, n).argtypes == _lib.SIGNATURES_HEADS[n][1]

"""CPU: include/qtx_beam_heads.h's one symbol, its ctypes table, and the entry's host-side
refusals (pointers that are never dereferenced: no GPU needed)."""
import ctypes as C
import os

import pytest

from qtx import _build, _lib

P = C.c_void_p
NAME = "qtx_decode_attention_beam_heads"


def test_header_matches_table():
    names = _lib.header_symbols(os.path.join(_build.REPO, "include", "qtx_beam_heads.h"))
    assert names == sorted(_lib.SIGNATURES_BEAM_HEADS) == [NAME]
    others = {**_lib.SIGNATURES, **_lib.SIGNATURES_ENCTRIALS, **_lib.SIGNATURES_BEAM_LONG,
              **_lib.SIGNATURES_WIDE_VOCAB, **_lib.SIGNATURES_HEADS}
    assert NAME not in others
    assert getattr(_lib.lib(), NAME).argtypes == _lib.SIGNATURES_BEAM_HEADS[NAME][1]


@pytest.mark.parametrize("anc,n_heads", [(0, 4), (0, 16), (0x3000, 2)], ids=["null4", "null16", "heads2"])
def test_refused_on_the_host(anc, n_heads):
    rc = getattr(_lib.lib(), NAME)(P(0x1000), 1536, P(0x1000), P(0x2000), P(0x10), P(0x10), 140, P(0x10),
                                   P(anc), 4, 8, P(0x10), P(0x10), n_heads, P(0))
    assert rc == 1 and _lib.lib().qtx_last_error()

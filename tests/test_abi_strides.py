"""The stride / alignment rules of include/qtx.h are checked on the host, before any launch:
with no GPU (and pointers that are never dereferenced) a misaligned call still returns
QTX_E_INVALID, where a call that reached a launch would return a HIP error instead."""
import ctypes as C

import pytest

from qtx import _lib
from qtx._lib import RowGemm

P = C.c_void_p
E_INVALID = 1


def rows(**kw):
    a = RowGemm()
    base = dict(A=0x1000, sa=0x1000, W=0x2000, sw=0x1000, bias=0x1000, M=7, N=1536, K=512, epi=0,
                out8=0x4000, ldo8=512, o8_ts=3584, os=0x8000, os_ts=7)
    base.update(kw)
    for k, v in base.items():
        setattr(a, k, v)
    return _lib.lib().qtx_linear_rows(C.byref(a), P(0))


@pytest.mark.parametrize("kp", [0, 1, 2])
@pytest.mark.parametrize("bad", [dict(ldo8=516), dict(ldo8=496), dict(o8_ts=3592),
                                 dict(out8=0x4004), dict(A=0x1004), dict(W=0x2008),
                                 dict(o8_ts=-512), dict(os_ts=-7)])
def test_linear_rows_strides(kp, bad):
    assert rows(kp=kp, **bad) == E_INVALID
    assert _lib.lib().qtx_last_error()


@pytest.mark.parametrize("kp,ldo8", [(0, 2040), (0, 2056), (1, 2048 + 16), (2, 2048 + 32), (3, 1024)])
def test_linear_rows_hidden_stride(kp, ldo8):
    """epi 3: ldo8 >= N and a multiple of 16 (a KP out8: of 64)."""
    assert rows(kp=kp, epi=3, N=2048, ldo8=ldo8, pmax_in=0x100, pmax_n=4,
                pmax_out=0x9000) == E_INVALID


def skinny(amode, X=0x1000, ldx=524, A=0x1000, W=0x2000):
    return _lib.lib().qtx_skinny_linear(amode, P(A), P(0x10), P(X), ldx, P(0x10), P(0x10), P(0x10), 1,
                                        P(W), P(0x10), P(0x10), 5, 512, 512, 8, 0, P(0), P(0x9000),
                                        P(0), P(0))


@pytest.mark.parametrize("amode", [1, 2, 3])
@pytest.mark.parametrize("bad", [dict(ldx=522), dict(ldx=508), dict(X=0x1004), dict(W=0x2004)])
def test_skinny_strides(amode, bad):
    assert skinny(amode, **bad) == E_INVALID


def test_skinny_int8_operand_alignment():
    assert skinny(0, X=0, ldx=0, A=0x1008) == E_INVALID
    assert skinny(0, X=0, ldx=0, W=0x2008) == E_INVALID


@pytest.mark.parametrize("kv_new,y,ldy,kc,vc", [(1, 0x1000, 1538, 0x1000, 0x2000),
                                                (1, 0x1000, 1024, 0x1000, 0x2000),
                                                (1, 0x1004, 1536, 0x1000, 0x2000),
                                                (0, 0x1000, 508, 0x1000, 0x2000),
                                                (0, 0x1000, 514, 0x1000, 0x2000),
                                                (1, 0x1000, 1536, 0x1004, 0x2000),
                                                (0, 0x1000, 512, 0x1000, 0x2008)])
def test_decode_attention_strides(kv_new, y, ldy, kc, vc):
    rc = _lib.lib().qtx_decode_attention(kv_new, P(y), ldy, P(kc), P(vc), P(0x10), P(0x10), 8,
                                         P(0x10), 5, P(0x10), 2, P(0x10), P(0x10), P(0))
    assert rc == E_INVALID

"""Guard bands, poisoned outputs and non-trivial strides for every C-ABI kernel entry point.

Every output and scratch buffer of a call lives between two poisoned guards
(tests/guarded.py) at exactly the extent include/qtx.h documents; after the call the
guards (and pitch gaps) must be intact and the FULL payload must equal the oracle
(oracle/qtx_oracle.py) bit for bit — log-probs within the platform log's 2e-6, as in
test_gpu_ops.py.  Every case runs with both poison bytes, so an element a kernel never
wrote cannot equal the expectation in both runs.  Inputs with a stride parameter (ldx, ldy,
the mask strides, S < kv_bs) go through padded_input: their gaps hold NaN / 0x7f / the
complementary mask value, which change the result if a kernel uses them.

Shapes are the smallest at which each code path can still go wrong: ragged in every
blocked dimension, one M per row-block size a launcher can choose.

Every case runs at two alignments (the `gb` fixture): align256 (the ids that name only a
poison), where each pointer is a fresh allocation or a 256-byte aligned payload, and
align16 (ids align16-poisonA5; one poison only), where every
pointer of the case — inputs, scales, biases, masks, weights, packed weights, outputs and
workspaces — sits at 16 (mod 256), the least alignment include/qtx.h promises to accept.  A
workspace at such a base puts every carved sub-buffer at 16 (mod 256) too.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from oracle import qtx_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from guarded import POISONS, guarded, guarded_pitched, padded_input, skewed  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
S0 = C.c_void_p(0)
OK, E_INVALID, E_HIP, E_WORKSPACE, E_UNSUPPORTED = 0, 1, 2, 3, 4
NAN = f32(np.nan)


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


class Guards:
    """The guarded buffers of one case: new() / pitched() / init() allocate, check()
    synchronises and asserts every guard."""

    def __init__(self, torch, poison, skew=0):
        self.torch, self.poison, self.skew, self.checks, self.keep = torch, poison, skew, [], []

    def _tdtype(self, dt):
        t = self.torch
        return {np.dtype(np.float32): t.float32, np.dtype(np.int8): t.int8,
                np.dtype(np.uint8): t.uint8, np.dtype(np.int32): t.int32,
                np.dtype(np.int64): t.int64}[np.dtype(dt)]

    def new(self, shape, dtype, name, pitch_bytes=None):
        t, c = guarded(self.torch, shape, self._tdtype(dtype), self.poison, name=name,
                       pitch_bytes=pitch_bytes, skew=self.skew)
        self.checks.append(c)
        return t

    def pitched(self, rows, row_bytes, pitch_bytes, dtype, name):
        t, c = guarded_pitched(self.torch, rows, row_bytes, pitch_bytes, self._tdtype(dtype),
                               self.poison, name=name, skew=self.skew)
        self.checks.append(c)
        return t

    def init(self, array, name):
        """A guarded in/out buffer holding `array`."""
        a = np.ascontiguousarray(array)
        t = self.new(a.shape, a.dtype, name)
        t.copy_(self.torch.from_numpy(a))
        return t

    def dev(self, a):
        """A plain (exact-size) input."""
        t = skewed(self.torch, a, self.skew)
        self.keep.append(t)
        return t

    def pad(self, a, pitch, fill):
        t = padded_input(self.torch, a, pitch, fill, skew=self.skew)
        self.keep.append(t)
        return t

    def check(self):
        try:
            self.torch.cuda.synchronize()
        except RuntimeError as e:       # a device fault: nothing more may run on this GPU
            pytest.exit(f"GPU error at synchronize, stopping the session: {e}", returncode=3)
        for c in self.checks:
            c()

    def assert_poison(self, t, name):
        """The payload was not written at all."""
        raw = t.contiguous().view(self.torch.uint8).cpu().numpy()
        bad = np.flatnonzero(raw != self.poison)
        assert bad.size == 0, f"{name}: payload byte {bad[0]} written"


# (poison, skew): align256 under both poisons — these keep the ids they had before the
# alignment parameter existed — and align16 under 0xA5 only: the unwritten-element argument of
# the two poisons is made at align256, and the file's time grows by half instead of doubling
GB_PARAMS = [(p, 0) for p in POISONS] + [(POISONS[0], 16)]


@pytest.fixture(params=GB_PARAMS,
                ids=[f"poison{p:02X}" if not k else f"align{k}-poison{p:02X}" for p, k in GB_PARAMS])
def gb(request, torch):
    return Guards(torch, *request.param)


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else S0


def lib():
    from qtx import _lib
    return _lib.lib()


def assert_ok(rc, what=""):
    if rc == E_HIP:                     # a HIP runtime error: nothing more may run on this GPU
        pytest.exit(f"HIP error in {what}, stopping the session: {lib().qtx_last_error()}",
                    returncode=3)
    assert rc == OK, (what, rc, lib().qtx_last_error())


def call(name, *args):
    assert_ok(getattr(lib(), name)(*args), name)


def np_(t):
    return t.cpu().numpy()


_MEMO = {}


def memo(key, fn):
    """References are computed once and shared by the cases (both poisons, every flag)."""
    if key not in _MEMO:
        _MEMO[key] = fn()
    return _MEMO[key]


def to_kp(a, pad=0):
    """[M, K] int8 -> the KP layout (include/qtx.h): row pair p, 64-byte K chunk c = one
    128-byte line (p * K/64 + c), rows 2p | 2p+1 at +0 | +64; odd M padded by a row of `pad`."""
    M, K = a.shape
    if M & 1:
        a = np.concatenate([a, np.full((1, K), pad, a.dtype)])
    return np.ascontiguousarray(a.reshape(-1, 2, K // 64, 64).transpose(0, 2, 1, 3)).reshape(-1, K)


def from_kp(a, M=None):
    K = a.shape[1]
    r = a.reshape(-1, K // 64, 2, 64).transpose(0, 2, 1, 3).reshape(-1, K)
    return r if M is None else r[:M]


def i8(byte):
    return np.uint8(byte).astype(np.int8)


def assert_kp(got, want, poison, pad_scratch, name):
    """A KP output [M + (M & 1), K]: rows < M equal the oracle; the pad row of an odd M is
    scratch where the header says so, and must be untouched (poison) otherwise."""
    M = want.shape[0]
    rows = from_kp(got)
    np.testing.assert_array_equal(rows[:M], want, err_msg=name)
    if (M & 1) and not pad_scratch:
        bad = np.flatnonzero(rows[M] != i8(poison))
        assert bad.size == 0, f"{name}: KP pad row written at column {bad[0]}"


# =====================================================================================
# row kernels
# =====================================================================================
def _rows_x(D):
    rng = np.random.default_rng(D)
    x = (rng.standard_normal((5, D)) * rng.uniform(1e-3, 10, (5, 1))).astype(f32)
    x[0] = 0
    x[1, :4] = [127.0, 0.5, 1.5, -2.5]
    x[1, 4:] = 0
    return x


@pytest.mark.parametrize("qmax", [127, 7])
@pytest.mark.parametrize("D", [512, 2048])
def test_row_quant(gb, D, qmax):
    x = _rows_x(D)
    q, s = gb.new((5, D), np.int8, "q"), gb.new((5,), f32, "s")
    call("qtx_row_quant", P(gb.dev(x)), 5, D, float(qmax), P(q), P(s), S0)
    gb.check()
    qo, so = O.quant_rows(x, 8 if qmax == 127 else 4)
    np.testing.assert_array_equal(np_(q), qo)
    np.testing.assert_array_equal(np_(s), so)


def test_layernorm_quant(gb, oracle_model):
    x = (_rows_x(512) + f32(0.25) * np.arange(512, dtype=f32)[None, :] / 512).astype(f32)
    a, b = oracle_model.enc[0]["ln"][0]
    y, q, s = gb.new((5, 512), f32, "y"), gb.new((5, 512), np.int8, "q"), gb.new((5,), f32, "s")
    call("qtx_layernorm_quant", P(gb.dev(x)), P(gb.dev(a)), P(gb.dev(b)), 5, 512, P(y), P(q),
         P(s), S0)
    gb.check()
    yo = O.layer_norm(x, a, b)
    np.testing.assert_array_equal(np_(y), yo)
    qo, so = O.quant_rows(yo)
    np.testing.assert_array_equal(np_(q), qo)
    np.testing.assert_array_equal(np_(s), so)
    # the forms with an optional output left out
    q2, s2 = gb.new((5, 512), np.int8, "q2"), gb.new((5,), f32, "s2")
    call("qtx_layernorm_quant", P(gb.dev(x)), P(gb.dev(a)), P(gb.dev(b)), 5, 512, S0, P(q2),
         P(s2), S0)
    y3 = gb.new((5, 512), f32, "y3")
    call("qtx_layernorm_quant", P(gb.dev(x)), P(gb.dev(a)), P(gb.dev(b)), 5, 512, P(y3), S0,
         S0, S0)
    gb.check()
    np.testing.assert_array_equal(np_(q2), qo)
    np.testing.assert_array_equal(np_(s2), so)
    np.testing.assert_array_equal(np_(y3), yo)


# =====================================================================================
# qtx_linear_i8: one ragged shape per kernel launch_gemm can choose
# =====================================================================================
@pytest.mark.parametrize("M,N,K,flags,bits", [
    (257, 272, 512, 1, 8),    # k_gemm256 (M >= 256, K % 256 == 0): ragged in M and N
    (257, 272, 320, 2, 8),    # the 128-tile k_gemm (K % 256 != 0)
    (33, 272, 512, 3, 8),     # the 32-tile k_gemm (M < 256)
    (257, 272, 512, 2, 4),    # int4, 128-tile
    (33, 48, 64, 0, 4)])      # int4, 32-tile
def test_linear_i8(gb, M, N, K, flags, bits):
    def ref():
        rng = np.random.default_rng(M * N + K + bits)
        qx, sx = O.quant_rows(rng.standard_normal((M, K)).astype(f32))
        qw, sw = O.quant_weight((rng.standard_normal((N, K)) * 0.05).astype(f32), bits)
        b = rng.standard_normal(N).astype(f32)
        res = rng.standard_normal((M, N)).astype(f32)
        y = O.linear_epilogue(O.int_gemm(qx, qw), sx, sw, b, relu=bool(flags & 1))
        return qx, sx, qw, sw, b, res, (res + y if flags & 2 else y)
    qx, sx, qw, sw, b, res, want = memo(("lin", M, N, K, flags, bits), ref)
    wd = gb.dev(qw)
    if bits == 4:
        packed = gb.new((N, K // 2), np.uint8, "packed")
        call("qtx_pack_int4", P(wd), N, K, P(packed), S0)
        wd = packed
    out = gb.new((M, N), f32, "out")
    call("qtx_linear_i8", P(gb.dev(qx)), P(gb.dev(sx)), P(wd), P(gb.dev(sw)), P(gb.dev(b)), M, N,
         K, bits, flags, P(gb.dev(res)) if flags & 2 else S0, P(out), S0)
    gb.check()
    np.testing.assert_array_equal(np_(out), want)


# =====================================================================================
# qtx_linear_rows
# =====================================================================================
def rows_rc(**kw):
    from qtx._lib import RowGemm
    a = RowGemm()
    for k, v in kw.items():
        setattr(a, k, v.data_ptr() if hasattr(v, "data_ptr") else v)
    return lib().qtx_linear_rows(C.byref(a), S0)


def rows_call(**kw):
    assert_ok(rows_rc(**kw), "qtx_linear_rows")


def _rows_ref(M, N, K):
    def ref():
        rng = np.random.default_rng(1000 * M + N + K)
        qx, sx = O.quant_rows(rng.standard_normal((M, K)).astype(f32))
        if K == 2048:      # an FFN hidden
            qx, sx = O.quant_rows(np.maximum(rng.standard_normal((M, K)), 0).astype(f32))
        qw, sw = O.quant_weight((rng.standard_normal((N, K)) * 0.05).astype(f32), 8)
        b = rng.standard_normal(N).astype(f32)
        y = O.linear_epilogue(O.int_gemm(qx, qw), sx, sw, b)
        return dict(qx=qx, sx=sx, qw=qw, sw=sw, b=b, y=y,
                    res=(rng.standard_normal((M, 512)) * 2).astype(f32))
    return memo(("rows", M, N, K), ref)


def _rows_operands(gb, r, kp):
    """A / W in the layout kp asks for (W through the library's packer, its output guarded)."""
    N, K = r["qw"].shape
    A = gb.dev(r["qx"] if kp == 0 else to_kp(r["qx"]))
    if kp == 0:
        W = gb.dev(r["qw"])
    else:
        W = gb.new((N, K), np.int8, "W packed")
        call("qtx_pack_w_kp" if kp == 1 else "qtx_pack_w_ws", P(gb.dev(r["qw"])), N, K, P(W), S0)
    return dict(A=A, sa=gb.dev(r["sx"]), W=W, sw=gb.dev(r["sw"]), bias=gb.dev(r["b"]),
                M=r["qx"].shape[0], N=N, K=K, kp=kp)


ROWS_CASES = [(kp, epi) for kp in (0, 1, 2) for epi in (0, 1, 2, 3)] + [(3, 3)]


@pytest.mark.parametrize("M", [7, 65, 129])
@pytest.mark.parametrize("kp,epi", ROWS_CASES)
def test_linear_rows(gb, oracle_model, kp, epi, M):
    """M odd (a KP pad row), one past a 64-row weight-stationary block, one past a 128-row
    tile; every epilogue of every layout.  kp = 3: the exchange scratch at exactly
    32 * M + 2048 bytes, the status word read where the header puts it."""
    poison = gb.poison
    N = {0: 1536, 1: 512, 2: 2048, 3: 2048}[epi]
    r = _rows_ref(M, N, 512)
    base = _rows_operands(gb, r, kp)
    y = r["y"]
    if epi == 0:
        out8, os_ = gb.new((3, M, 512), np.int8, "out8"), gb.new((3, M), f32, "os")
        rows_call(epi=0, out8=out8, ldo8=512, o8_ts=M * 512, os=os_, os_ts=M, **base)
        gb.check()
        for t in range(3):
            q, s = O.quant_rows(y[:, 512 * t:512 * (t + 1)])
            np.testing.assert_array_equal(np_(out8[t]), q)
            np.testing.assert_array_equal(np_(os_[t]), s)
    elif epi == 1:
        la, lb = oracle_model.dec[1]["ln"][0]
        x = r["res"] + y
        ln = O.layer_norm(x, la, lb)
        q, s = memo(("rows-lnq", M), lambda: O.quant_rows(ln))
        ln_ab = dict(ln_a=gb.dev(la), ln_b=gb.dev(lb))
        # the quantized form (lnq + lns), then the fp32 form (lnout)
        xd = gb.init(r["res"], "xout")
        Mp = M + (M & 1) if kp else M
        lnq, lns = gb.new((Mp, 512), np.int8, "lnq"), gb.new((M,), f32, "lns")
        rows_call(epi=1, res=xd, xout=xd, lnq=lnq, lns=lns, **ln_ab, **base)
        xd2 = gb.init(r["res"], "xout2")
        lnout = gb.new((M, 512), f32, "lnout")
        rows_call(epi=1, res=xd2, xout=xd2, lnout=lnout, **ln_ab, **base)
        gb.check()
        np.testing.assert_array_equal(np_(xd), x)
        np.testing.assert_array_equal(np_(lns), s)
        if kp:
            # kp = 2: the pad row of an odd M is written as scratch (include/qtx.h)
            assert_kp(np_(lnq), q, poison, kp >= 2, "lnq")
        else:
            np.testing.assert_array_equal(np_(lnq), q)
        np.testing.assert_array_equal(np_(xd2), x)
        np.testing.assert_array_equal(np_(lnout), ln)
    else:
        h = np.where(y > 0, y, f32(0)).astype(f32)
        pm_want = h.reshape(M, 4, 512).max(-1).T
        if epi == 2:
            pm = gb.new((4, M), f32, "pmax_out")
            rows_call(epi=2, pmax_out=pm, **base)
            gb.check()
            np.testing.assert_array_equal(np_(pm), pm_want)
            return
        qh, sh = memo(("rows-h", M), lambda: O.quant_rows(h))
        Mp = M + (M & 1) if kp else M
        h8, os_ = gb.new((Mp, 2048), np.int8, "out8"), gb.new((M,), f32, "os")
        if kp == 3:
            nb = (M + 31) // 32
            gx = gb.new((32 * M + 2048,), np.uint8, "exchange scratch")
            rows_call(epi=3, pmax_out=gx, out8=h8, ldo8=2048, os=os_, **base)
            gb.check()
            status = int(np_(gx)[1024 * nb + 4:1024 * nb + 8].view(np.uint32)[0])
            assert status == 0
        else:
            # a NaN tail after pmax_in [4][M]: a partial past p < pmax_n must not be read
            rows_call(epi=3, pmax_in=gb.pad(pm_want, M, NAN), pmax_n=4, out8=h8, ldo8=2048,
                      os=os_, **base)
            gb.check()
        np.testing.assert_array_equal(np_(os_), sh)
        if kp:
            # kp = 2 / 3: the pad row of an odd M is written as scratch (include/qtx.h)
            assert_kp(np_(h8), qh, poison, kp >= 2, "out8")
        else:
            np.testing.assert_array_equal(np_(h8), qh)


@pytest.mark.parametrize("lnq", [True, False])
def test_linear_rows_splitk_part(gb, oracle_model, lnq):
    """epi 1, kp = 1, K = 2048 split over 4 workgroups per row tile at M = 129: `part` at
    exactly ksplit * M * 2 KB."""
    M, ks = 129, 4
    r = _rows_ref(M, 512, 2048)
    base = _rows_operands(gb, r, 1)
    la, lb = oracle_model.dec[1]["ln"][0]
    xd = gb.init(r["res"], "xout")
    part = gb.new((ks * M * 512,), np.int32, "part")
    assert part.numel() * 4 == ks * M * 2048
    out = dict(lnq=gb.new((M + 1, 512), np.int8, "lnq"), lns=gb.new((M,), f32, "lns")) if lnq \
        else dict(lnout=gb.new((M, 512), f32, "lnout"))
    rows_call(epi=1, res=xd, xout=xd, ln_a=gb.dev(la), ln_b=gb.dev(lb), part=part, ksplit=ks,
              **out, **base)
    gb.check()
    x = r["res"] + r["y"]
    np.testing.assert_array_equal(np_(xd), x)
    ln = O.layer_norm(x, la, lb)
    if lnq:
        q, s = O.quant_rows(ln)
        assert_kp(np_(out["lnq"]), q, gb.poison, False, "lnq")
        np.testing.assert_array_equal(np_(out["lns"]), s)
    else:
        np.testing.assert_array_equal(np_(out["lnout"]), ln)
    # every partial was written (the epilogue sums all of them)
    raw = np_(part).view(np.uint8)
    assert not (raw.reshape(-1, 4) == gb.poison).all(axis=1).any()


@pytest.mark.parametrize("M", [7, 65, 129])
@pytest.mark.parametrize("kp", [0, 1, 2])
def test_linear_rows_strided_qkv(gb, kp, M):
    """epi 0 with Q, K and V in ONE pitched buffer (ldo8 = 1600, o8_ts = 512) and the
    scales at os_ts = M + 3: the 64 gap bytes per row and the 3 gap floats per tile keep
    their poison."""
    r = _rows_ref(M, 1536, 512)
    base = _rows_operands(gb, r, kp)
    out8 = gb.pitched(M, 1536, 1600, np.int8, "out8")
    os_ = gb.pitched(3, 4 * M, 4 * (M + 3), f32, "os")
    rows_call(epi=0, out8=out8, ldo8=1600, o8_ts=512, os=os_, os_ts=M + 3, **base)
    gb.check()
    got8, gots = np_(out8), np_(os_)
    for t in range(3):
        q, s = O.quant_rows(r["y"][:, 512 * t:512 * (t + 1)])
        np.testing.assert_array_equal(got8[:, 512 * t:512 * (t + 1)], q)
        np.testing.assert_array_equal(gots[t], s)


@pytest.mark.parametrize("kp", [0, 1, 2])
def test_linear_rows_misaligned_is_invalid(gb, kp):
    """The kernels store out8 in 16-byte vectors: ldo8 % 16, o8_ts % 16 and a 16-byte
    aligned out8 are checked on the host (QTX_E_INVALID) — nothing is launched, every output
    byte keeps its poison."""
    M = 7
    r = _rows_ref(M, 1536, 512)
    base = _rows_operands(gb, r, kp)
    out8 = gb.new((3 * M * 520 + 16,), np.int8, "out8")
    os_ = gb.new((3, M), f32, "os")
    ok = dict(epi=0, out8=out8, ldo8=512, o8_ts=M * 512, os=os_, os_ts=M)
    for bad in (dict(ldo8=520 - 4), dict(o8_ts=M * 512 + 8), dict(out8=out8.data_ptr() + 4),
                dict(out8=out8.data_ptr() + 8), dict(A=base["A"].data_ptr() + 8),
                dict(W=base["W"].data_ptr() + 8), dict(ldo8=496)):
        assert rows_rc(**{**ok, **base, **bad}) == E_INVALID, bad
    gb.check()
    gb.assert_poison(out8, "out8")
    gb.assert_poison(os_, "os")


# =====================================================================================
# fused FFN and the packers
# =====================================================================================
def _ffn_ref(M, F):
    def ref():
        rng = np.random.default_rng(M + F)
        x1 = (rng.standard_normal((M, 512)) * 2).astype(f32)
        la = (1 + 0.1 * rng.standard_normal(512)).astype(f32)
        lb = (0.1 * rng.standard_normal(512)).astype(f32)
        qx, sx = O.quant_rows(O.layer_norm(x1, la, lb))
        qw1, sw1 = O.quant_weight((rng.standard_normal((F, 512)) * 0.05).astype(f32), 8)
        qw2, sw2 = O.quant_weight((rng.standard_normal((512, F)) * 0.05).astype(f32), 8)
        b1 = (rng.standard_normal(F) * 0.1).astype(f32)
        b2 = (rng.standard_normal(512) * 0.1).astype(f32)
        na = (1 + 0.1 * rng.standard_normal(512)).astype(f32)
        nb = (0.1 * rng.standard_normal(512)).astype(f32)
        h = O.linear_epilogue(O.int_gemm(qx, qw1), sx, sw1, b1, relu=True)
        qh, sh = O.quant_rows(h)
        x2 = x1 + O.linear_epilogue(O.int_gemm(qh, qw2), sh, sw2, b2)
        ln = O.layer_norm(x2, na, nb)
        q, s = O.quant_rows(ln)
        return dict(x1=x1, qx=qx, sx=sx, qw1=qw1, sw1=sw1, qw2=qw2, sw2=sw2, b1=b1, b2=b2,
                    na=na, nb=nb, x2=x2, ln=ln, q=q, s=s)
    return memo(("ffn", M, F), ref)


@pytest.mark.parametrize("lnq", [True, False])
@pytest.mark.parametrize("F", [256, 2048])
@pytest.mark.parametrize("M", [7, 129])
def test_ffn_rows(gb, M, F, lnq):
    from qtx._lib import FfnRows
    r = _ffn_ref(M, F)
    wf = gb.new((F * 1024,), np.int8, "wf")
    call("qtx_pack_ffn", P(gb.dev(r["qw1"])), P(gb.dev(r["qw2"])), F, P(wf), S0)
    a = FfnRows()
    a.A, a.sa, a.wf = gb.dev(to_kp(r["qx"])).data_ptr(), gb.dev(r["sx"]).data_ptr(), wf.data_ptr()
    a.sw1, a.b1 = gb.dev(r["sw1"]).data_ptr(), gb.dev(r["b1"]).data_ptr()
    a.sw2, a.b2 = gb.dev(r["sw2"]).data_ptr(), gb.dev(r["b2"]).data_ptr()
    x = gb.init(r["x1"], "x")
    a.x, a.ln_a, a.ln_b = x.data_ptr(), gb.dev(r["na"]).data_ptr(), gb.dev(r["nb"]).data_ptr()
    a.M, a.F = M, F
    if lnq:
        q8, qs = gb.new((M + (M & 1), 512), np.int8, "lnq"), gb.new((M,), f32, "lns")
        a.lnq, a.lns = q8.data_ptr(), qs.data_ptr()
    else:
        lo = gb.new((M, 512), f32, "lnout")
        a.lnout = lo.data_ptr()
    rc = lib().qtx_ffn_rows(C.byref(a), S0)
    assert_ok(rc, "qtx_ffn_rows")
    gb.check()
    np.testing.assert_array_equal(np_(x), r["x2"])
    if lnq:
        assert_kp(np_(q8), r["q"], gb.poison, False, "lnq")
        np.testing.assert_array_equal(np_(qs), r["s"])
    else:
        np.testing.assert_array_equal(np_(lo), r["ln"])


def _ffn_pack_ref(w1, w2):
    """qtx_pack_ffn's stream (include/qtx.h) restated (as tests/test_gpu_ffn.py)."""
    F = w1.shape[0]
    out = np.zeros((F // 64, 4, 16, 64, 16), np.int8)
    lane = np.arange(64)
    f, g = lane & 15, lane >> 4
    b = np.arange(16)
    for c in range(F // 64):
        for fr in range(16):
            for hh in range(2):
                s, j = 4 * hh + (fr >> 2), fr & 3
                idx = 64 * s + 16 * g[:, None] + b[None, :]
                out[c, hh, fr] = np.take_along_axis(w1[64 * c + 16 * j + f], idx, axis=1)
            for ch in range(2):
                col = np.where(fr < 8, 16 * f + 8 * ch + fr, 256 + 16 * f + 8 * ch + fr - 8)
                k = 64 * c + 16 * (b[None, :] >> 2) + 4 * g[:, None] + (b[None, :] & 3)
                out[c, 2 + ch, fr] = np.take_along_axis(w2[col], k, axis=1)
    return out.reshape(-1)


def test_pack_ffn(gb):
    F = 256                               # the smallest legal F
    rng = np.random.default_rng(3)
    w1 = rng.integers(-127, 128, (F, 512)).astype(np.int8)
    w2 = rng.integers(-127, 128, (512, F)).astype(np.int8)
    out = gb.new((F * 1024,), np.int8, "out")
    call("qtx_pack_ffn", P(gb.dev(w1)), P(gb.dev(w2)), F, P(out), S0)
    gb.check()
    np.testing.assert_array_equal(np_(out), _ffn_pack_ref(w1, w2))


def test_pack_w_kp(gb):
    N, K = 512, 64                        # the smallest legal N and K
    w = np.random.default_rng(N + K).integers(-127, 128, (N, K)).astype(np.int8)
    out = gb.new((N, K), np.int8, "out")
    call("qtx_pack_w_kp", P(gb.dev(w)), N, K, P(out), S0)
    gb.check()
    rho = np.arange(512)
    order = (rho & ~127) + 8 * (rho & 15) + ((rho >> 4) & 7)
    np.testing.assert_array_equal(np_(out), to_kp(w[order]))


def test_pack_w_ws(gb):
    N = 512
    w = np.random.default_rng(5).integers(-127, 128, (N, 512)).astype(np.int8)
    out = gb.new((N, 512), np.int8, "out")
    call("qtx_pack_w_ws", P(gb.dev(w)), N, 512, P(out), S0)
    gb.check()
    t, wv, s, j, l = np.meshgrid(np.arange(N // 512), np.arange(8), np.arange(8), np.arange(4),
                                 np.arange(64), indexing="ij")
    n = 512 * t + 64 * wv + 16 * ((l & 15) >> 2) + 4 * j + (l & 3)
    k0 = 64 * s + 16 * (l >> 4)
    idx = k0.reshape(-1)[:, None] + np.arange(16)[None, :]
    np.testing.assert_array_equal(np_(out),
                                  np.take_along_axis(w[n.reshape(-1)], idx, axis=1).reshape(N, 512))


@pytest.mark.parametrize("N,K", [(1, 70), (3, 64)])
def test_pack_int4(gb, N, K):
    """N = 1: fewer output bytes than one workgroup's threads."""
    q = np.random.default_rng(K).integers(-8, 8, (N, K)).astype(np.int8)
    out = gb.new((N, K // 2), np.uint8, "packed")
    call("qtx_pack_int4", P(gb.dev(q)), N, K, P(out), S0)
    gb.check()
    u = q.view(np.uint8) & 0xF
    np.testing.assert_array_equal(np_(out), u[:, 0::2] | (u[:, 1::2] << 4))


# =====================================================================================
# attention
# =====================================================================================
def _attn_ref(B, Sq, Sk, form, dec):
    def ref():
        rng = np.random.default_rng(Sq * 7 + Sk + B)
        q = rng.integers(-127, 128, (B, Sq, 512)).astype(np.int8)
        k = rng.integers(-127, 128, (B, Sk, 512)).astype(np.int8)
        v = rng.integers(-127, 128, (B, Sk, 512)).astype(np.int8)
        sq, sk, sv = (rng.uniform(0.002, 0.03, (B, n)).astype(f32) for n in (Sq, Sk, Sk))
        if form == "key":
            km = np.ones((B, Sk), np.uint8)
            km[0, Sk - Sk // 3:] = 0
            km[-1, 1::7] = 0
            mask = np.broadcast_to(km[:, None, :], (B, Sq, Sk)).copy()
        else:
            mask = (rng.uniform(size=(B, Sq, Sk)) < 0.7).astype(np.uint8)
            mask[:, :, 0] = 1
            mask[0, :, -1] = 1          # the element before a gap is kept here, masked there
            mask[-1, :, -1] = 0
            km = None
        ctx, qp = O.attention(q, sq, k, sk, v, sv, mask, 8, dec=bool(dec))
        return dict(q=q, k=k, v=v, sq=sq, sk=sk, sv=sv, mask=mask, km=km, ctx=ctx, qp=qp)
    return memo(("attn", B, Sq, Sk, form, dec), ref)


@pytest.mark.parametrize("dec", [0, 1])
@pytest.mark.parametrize("form", ["full", "key"])
@pytest.mark.parametrize("B,Sq,Sk", [(2, 5, 37), (1, 7, 130)])
def test_attention(gb, B, Sq, Sk, form, dec):
    """(2, 5, 37): the MFMA kernel; (1, 7, 130): k_attention past 128 keys.  The mask is
    passed with padded strides m_is = Sk + 5, m_bs = Sq * m_is + 11 whose gaps hold the
    complement of the neighbouring mask value; "key": the m_is = 0 broadcast form."""
    r = _attn_ref(B, Sq, Sk, form, dec)
    if form == "key":
        m_is, m_bs = 0, Sk + 5
        md = gb.pad(r["km"], m_bs, "complement")
    else:
        m_is = Sk + 5
        m_bs = Sq * m_is + 11
        md = gb.pad(r["mask"], (m_bs, m_is), "complement")
    ctx = gb.new((B, Sq, 512), f32, "ctx")
    call("qtx_attention_i8", P(gb.dev(r["q"])), P(gb.dev(r["sq"])), P(gb.dev(r["k"])),
         P(gb.dev(r["sk"])), P(gb.dev(r["v"])), P(gb.dev(r["sv"])), P(md), m_bs, m_is, B, 8, Sq,
         Sk, P(ctx), dec, S0)
    gb.check()
    np.testing.assert_array_equal(np_(ctx), r["ctx"])


@pytest.mark.parametrize("B,S,keymask", [(2, 5, True), (2, 100, True), (2, 5, False)])
def test_attention_quant(gb, B, S, keymask):
    def ref():
        rng = np.random.default_rng(S * 11 + B)
        q, k, v = (rng.integers(-127, 128, (B, S, 512)).astype(np.int8) for _ in range(3))
        sq, sk, sv = (rng.uniform(0.002, 0.03, (B, S)).astype(f32) for _ in range(3))
        km = np.ones((B, S), np.uint8)
        if keymask:
            km[0, S - S // 3:] = 0
            km[-1, 1::7] = 0
        co, _ = O.attention(q, sq, k, sk, v, sv, km[:, None, :], 8)
        return q, k, v, sq, sk, sv, km, O.quant_rows(co)
    q, k, v, sq, sk, sv, km, (qc, sc) = memo(("attnq", B, S, keymask), ref)
    ctx8, sctx = gb.new((B, S, 512), np.int8, "ctx8"), gb.new((B, S), f32, "sctx")
    call("qtx_attention_i8_quant", P(gb.dev(q)), P(gb.dev(sq)), P(gb.dev(k)), P(gb.dev(sk)),
         P(gb.dev(v)), P(gb.dev(sv)), P(gb.dev(km)) if keymask else S0, B, S, P(ctx8), P(sctx), S0)
    gb.check()
    np.testing.assert_array_equal(np_(sctx), sc)
    np.testing.assert_array_equal(np_(ctx8), qc)


@pytest.mark.parametrize("dec", [0, 1])
@pytest.mark.parametrize("want_qk,want_pc", [(True, True), (False, True), (True, False)])
def test_attention_trace(gb, want_qk, want_pc, dec):
    B, Sq, Sk = 2, 5, 37
    r = _attn_ref(B, Sq, Sk, "full", dec)
    acc = memo(("attn-acc", dec), lambda: np.einsum(
        "bhid,bhjd->bhij", O.split_heads(r["q"], 8).astype(np.int64),
        O.split_heads(r["k"], 8).astype(np.int64)).astype(f32))
    m_is = Sk + 5
    m_bs = Sq * m_is + 11
    ctx = gb.new((B, Sq, 512), f32, "ctx")
    qk = gb.new((B, 8, Sq, Sk), f32, "qk_acc")
    pc = gb.new((B, 8, Sq, Sk), f32, "p_codes")
    call("qtx_attention_trace", P(gb.dev(r["q"])), P(gb.dev(r["sq"])), P(gb.dev(r["k"])),
         P(gb.dev(r["sk"])), P(gb.dev(r["v"])), P(gb.dev(r["sv"])),
         P(gb.pad(r["mask"], (m_bs, m_is), "complement")), m_bs, m_is, B, 8, Sq, Sk, P(ctx),
         P(qk) if want_qk else S0, P(pc) if want_pc else S0, dec, S0)
    gb.check()
    np.testing.assert_array_equal(np_(ctx), r["ctx"])
    if want_qk:
        np.testing.assert_array_equal(np_(qk), acc)
    else:
        gb.assert_poison(qk, "qk_acc")
    if want_pc:
        np.testing.assert_array_equal(np_(pc), r["qp"].astype(f32))
    else:
        gb.assert_poison(pc, "p_codes")


# =====================================================================================
# qtx_skinny_linear: one case per dispatch branch of skinny_mode
# =====================================================================================
LDX_PAD = 12


def tile_max(y):
    M, N = y.shape
    return np.abs(y).reshape(M, N // 16, 16).max(-1).T


def _pmax_n(amode, M, N, K):
    """amode 2: every M meets each of pmax_n = 1, 8, 100, 128 over the four (N, K) shapes."""
    base = {1: 0, 3: 1, 5: 1, 33: 2, 97: 3, 193: 0}[M]
    return (1, 8, 100, 128)[(base + N // 512 + K // 2048) % 4] if amode == 2 else 0


def _skinny_ref(amode, M, N, K, bits, oracle_model):
    def ref():
        rng = np.random.default_rng(M + N + K + 7 * amode + bits)
        x = (rng.standard_normal((M, K)) * 3).astype(f32)
        if amode >= 2 and K == 2048:
            x = np.maximum(x, 0).astype(f32)          # a ReLU hidden
        if amode >= 2 and M > 1:
            x[M - 1] = 0                               # an all-zero row: the 1e-5 clamp
        a, bb = oracle_model.dec[0]["ln"][2]
        if amode == 0:
            qx, sx = O.quant_rows(x)
        elif amode == 1:
            qx, sx = O.quant_rows(O.layer_norm(x, a, bb))
        else:
            qx, sx = O.quant_rows(x)
        n = _pmax_n(amode, M, N, K)
        parts = None
        if amode == 2:     # complete partial row maxima over n (uneven) column groups
            parts = np.stack([np.abs(c).max(-1) if c.shape[1] else np.zeros(M, f32)
                              for c in np.array_split(x, n, axis=1)]).astype(f32)
        qw, sw = O.quant_weight((rng.standard_normal((N, K)) * 0.05).astype(f32), bits)
        b = rng.standard_normal(N).astype(f32)
        res = rng.standard_normal((M, N)).astype(f32)
        return dict(x=x, qx=qx, sx=sx, parts=parts, n=n, qw=qw, sw=sw, b=b, res=res,
                    acc=O.int_gemm(qx, qw), ln=(a, bb))
    return memo(("skinny", amode, M, N, K, bits), ref)


def _skinny_run(gb, r, amode, M, N, K, bits, flags, X=None, ldx=None):
    """One qtx_skinny_linear call on guarded out / pmax_out; returns (rc, out, pm)."""
    wd = gb.dev(r["qw"])
    if bits == 4:
        packed = gb.new((N, K // 2), np.uint8, "packed")
        call("qtx_pack_int4", P(wd), N, K, P(packed), S0)
        wd = packed
    out = gb.new((M, N), f32, "out")
    pm = gb.new((N // 16, M), f32, "pmax_out")
    A = sa = lna = lnb = pin = None
    if amode == 0:
        A, sa = gb.dev(r["qx"]), gb.dev(r["sx"])
        ldx = 0
    else:
        ldx = K + LDX_PAD if ldx is None else ldx
        if X is None:
            X = gb.pad(r["x"], K + LDX_PAD, NAN)      # NaN gaps between the rows and a NaN tail
        if amode == 1:
            lna, lnb = gb.dev(r["ln"][0]), gb.dev(r["ln"][1])
        if amode == 2:
            pin = gb.pad(r["parts"], M, NAN)          # [pmax_n][M], a NaN tail after it
    xp = X if isinstance(X, C.c_void_p) else P(X)
    rc = lib().qtx_skinny_linear(amode, P(A), P(sa), xp, ldx, P(lna), P(lnb), P(pin), r["n"],
                                 P(wd), P(gb.dev(r["sw"])), P(gb.dev(r["b"])), M, N, K, bits,
                                 flags, P(gb.dev(r["res"])), P(out), P(pm), S0)
    return rc, out, pm


def _skinny_shapes():
    for N, K in [(48, 512), (512, 512), (1536, 512), (512, 2048)]:
        for amode in (0, 1, 2, 3):
            if amode == 1 and K != 512:
                continue                               # the LayerNorm prologue is K = 512 only
            Ms = [1, 5, 33, 97, 193]
            if K == 2048 and amode >= 2:
                Ms.insert(1, 3)                        # k_skinny8_ffn2's 4-row blocks
            for M in Ms:
                yield amode, M, N, K


@pytest.mark.parametrize("flags", [0, 1, 2, 5])
@pytest.mark.parametrize("amode,M,N,K", list(_skinny_shapes()))
def test_skinny(gb, oracle_model, amode, M, N, K, flags):
    """N = 48 forces the K-split k_skinny even at M >= 96; N = 1536 with the LayerNorm
    prologue runs k_skinny_wide at every M, the other K = 512 shapes from M = 97 (8-row
    blocks); K = 2048: k_skinny8_ffn2 (M <= 32, flags 2, amode 2 / 3), else k_skinny with 4- /
    8- / 16-row blocks (M = 33 / 97 / 193).  amode 1-3 read X at ldx = K + 12 with NaN gaps,
    amode 2 its partial maxima with a NaN tail (pmax_n cycles through 1, 8, 100, 128)."""
    r = _skinny_ref(amode, M, N, K, 8, oracle_model)
    rc, out, pm = _skinny_run(gb, r, amode, M, N, K, 8, flags)
    assert_ok(rc, "qtx_skinny_linear")
    gb.check()
    y = O.linear_epilogue(r["acc"], r["sx"], r["sw"], r["b"], relu=bool(flags & 1))
    if flags & 2:
        y = r["res"] + y
    np.testing.assert_array_equal(np_(out), y)
    if flags & 4:
        np.testing.assert_array_equal(np_(pm), tile_max(y))
    else:
        gb.assert_poison(pm, "pmax_out")


@pytest.mark.parametrize("amode,M,N,K,flags", [(1, 5, 1536, 512, 5), (2, 33, 512, 2048, 2),
                                               (3, 97, 512, 512, 2), (1, 5, 512, 512, 0),
                                               (3, 5, 48, 2048, 0)])
def test_skinny_int4(gb, oracle_model, amode, M, N, K, flags):
    """4-bit weights with the fp32 prologues (k_skinny_wide, k_skinny K = 2048 and 512)."""
    r = _skinny_ref(amode, M, N, K, 4, oracle_model)
    rc, out, pm = _skinny_run(gb, r, amode, M, N, K, 4, flags)
    assert_ok(rc, "qtx_skinny_linear")
    gb.check()
    y = O.linear_epilogue(r["acc"], r["sx"], r["sw"], r["b"], relu=bool(flags & 1))
    if flags & 2:
        y = r["res"] + y
    np.testing.assert_array_equal(np_(out), y)
    if flags & 4:
        np.testing.assert_array_equal(np_(pm), tile_max(y))


@pytest.mark.parametrize("flags", [3, 4, 6, 7])
@pytest.mark.parametrize("amode,M,N,K", [(0, 5, 512, 512), (1, 5, 1536, 512), (3, 5, 512, 2048),
                                         (2, 97, 512, 512), (0, 97, 48, 2048)])
def test_skinny_rejected_flags(gb, oracle_model, amode, M, N, K, flags):
    """The flag combinations the dispatcher has no kernel for: QTX_E_UNSUPPORTED, and every
    output byte still holds the poison."""
    r = _skinny_ref(amode, M, N, K, 8, oracle_model)
    rc, out, pm = _skinny_run(gb, r, amode, M, N, K, 8, flags)
    assert rc == E_UNSUPPORTED
    gb.check()
    gb.assert_poison(out, "out")
    gb.assert_poison(pm, "pmax_out")


def test_skinny_rejected_shapes(gb, oracle_model):
    """amode 1 with K = 2048, N % 16 != 0: QTX_E_UNSUPPORTED; an X the 16-byte row loads
    cannot address (ldx % 4 != 0, ldx < K, a base off 16 bytes): QTX_E_INVALID on the host.
    Nothing is launched."""
    M = 5
    r = dict(_skinny_ref(3, M, 512, 2048, 8, oracle_model))
    rc, out, pm = _skinny_run(gb, r, 1, M, 512, 2048, 8, 0)
    assert rc == E_UNSUPPORTED
    gb.assert_poison(out, "out")
    r = _skinny_ref(3, M, 512, 512, 8, oracle_model)
    X = gb.pad(r["x"], 512 + LDX_PAD, NAN)
    for amode in (1, 2, 3):
        rr = dict(r, parts=np.abs(r["x"]).max(-1)[None, :].astype(f32), n=1)
        for kw in (dict(ldx=512 + 10), dict(ldx=508), dict(X=C.c_void_p(X.data_ptr() + 4)),
                   dict(X=C.c_void_p(X.data_ptr() + 8))):
            rc, out, pm = _skinny_run(gb, rr, amode, M, 512, 512, 8, 0, **{"X": X, **kw})
            assert rc == E_INVALID, (amode, kw)
            gb.assert_poison(out, "out")
    gb.check()


# =====================================================================================
# qtx_decode_attention
# =====================================================================================
def vgroup4(v, fill=0):
    """[B, n, 512] int8 -> qtx_decode_attention's 4-key group layout [B, ceil(n/4), 512, 4]."""
    B, n, D = v.shape
    g4 = (n + 3) // 4
    vp = np.full((B, 4 * g4, D), fill, np.int8)
    vp[:, :n] = v
    return np.ascontiguousarray(vp.reshape(B, g4, 4, D).transpose(0, 1, 3, 2))


def head_max(ctx):
    return np.abs(ctx).reshape(-1, 8, 64).max(-1).T


@pytest.mark.parametrize("step", [0, 5])
def test_decode_self_attention(gb, step):
    """B = 3, kv_bs = 8: y at ldy = 1536 + 8 with NaN gaps; the caches and their scales are
    unchanged everywhere except row `step` (grouped-V pad keys included)."""
    B, kv_bs = 3, 8

    def ref():
        rng = np.random.default_rng(B * 1000 + step)
        y = rng.standard_normal((B, 1536)).astype(f32)
        kc = rng.integers(-127, 128, (B, kv_bs, 512)).astype(np.int8)
        vc = rng.integers(-127, 128, (B, kv_bs, 512)).astype(np.int8)
        skc = rng.uniform(0.002, 0.03, (B, kv_bs)).astype(f32)
        svc = rng.uniform(0.002, 0.03, (B, kv_bs)).astype(f32)
        qq, sq = O.quant_rows(y[:, :512])
        qk, sk = O.quant_rows(y[:, 512:1024])
        qv, sv = O.quant_rows(y[:, 1024:])
        kc2, vc2, skc2, svc2 = kc.copy(), vc.copy(), skc.copy(), svc.copy()
        kc2[:, step], vc2[:, step], skc2[:, step], svc2[:, step] = qk, qv, sk, sv
        n = step + 1
        ctx, _ = O.attention(qq[:, None], sq[:, None], kc2[:, :n], skc2[:, :n], vc2[:, :n],
                             svc2[:, :n], np.ones((B, 1, n), np.uint8), dec=True)
        return y, (kc, vc, skc, svc), (kc2, vc2, skc2, svc2), ctx[:, 0]
    y, (kc, vc, skc, svc), (kc2, vc2, skc2, svc2), ctx = memo(("dself", step), ref)
    kcd, vcd = gb.init(kc, "kc"), gb.init(vgroup4(vc), "vc")
    skd, svd = gb.init(skc, "skc"), gb.init(svc, "svc")
    ctxd, pm = gb.new((B, 512), f32, "ctx"), gb.new((8, B), f32, "pmax")
    call("qtx_decode_attention", 1, P(gb.pad(y, 1536 + 8, NAN)), 1536 + 8, P(kcd), P(vcd),
         P(skd), P(svd), kv_bs, P(gb.dev(np.array([step], np.int32))), 0, S0, B, P(ctxd), P(pm),
         S0)
    gb.check()
    np.testing.assert_array_equal(np_(kcd), kc2)
    np.testing.assert_array_equal(np_(vcd), vgroup4(vc2))
    np.testing.assert_array_equal(np_(skd), skc2)
    np.testing.assert_array_equal(np_(svd), svc2)
    np.testing.assert_array_equal(np_(ctxd), ctx)
    np.testing.assert_array_equal(np_(pm), head_max(ctx))


@pytest.mark.parametrize("masked_sentence", [False, True])
def test_decode_cross_attention(gb, masked_sentence):
    """S = 5 keys inside kv_bs = 8 cache rows: rows S .. kv_bs - 1 hold 0x7f codes and NaN
    scales, which must not reach the result; the caches are read only.  masked_sentence: one
    sentence's mask is all zero (the reference's uniform softmax over -1e9 scores)."""
    B, S, kv_bs = 3, 5, 8

    def ref():
        rng = np.random.default_rng(B + S + masked_sentence)
        y = rng.standard_normal((B, 512)).astype(f32)
        kc = rng.integers(-127, 128, (B, S, 512)).astype(np.int8)
        vc = rng.integers(-127, 128, (B, S, 512)).astype(np.int8)
        skc = rng.uniform(0.002, 0.03, (B, S)).astype(f32)
        svc = rng.uniform(0.002, 0.03, (B, S)).astype(f32)
        mask = np.ones((B, S), np.uint8)
        mask[0, 3:] = 0
        mask[2, 1] = 0
        if masked_sentence:
            mask[1, :] = 0
        qq, sq = O.quant_rows(y)
        ctx, _ = O.attention(qq[:, None], sq[:, None], kc, skc, vc, svc, mask[:, None], dec=True)
        return y, kc, vc, skc, svc, mask, ctx[:, 0]
    y, kc, vc, skc, svc, mask, ctx = memo(("dcross", masked_sentence), ref)
    kcp = np.full((B, kv_bs, 512), 0x7f, np.int8)
    kcp[:, :S] = kc
    vcp = np.full((B, kv_bs, 512), 0x7f, np.int8)
    vcp[:, :S] = vc
    skp, svp = np.full((B, kv_bs), NAN, f32), np.full((B, kv_bs), NAN, f32)
    skp[:, :S], svp[:, :S] = skc, svc
    kcd, vcd = gb.init(kcp, "kc"), gb.init(vgroup4(vcp), "vc")
    skd, svd = gb.init(skp, "skc"), gb.init(svp, "svc")
    ctxd, pm = gb.new((B, 512), f32, "ctx"), gb.new((8, B), f32, "pmax")
    call("qtx_decode_attention", 0, P(gb.pad(y, 512 + 8, NAN)), 512 + 8, P(kcd), P(vcd), P(skd),
         P(svd), kv_bs, S0, S, P(gb.dev(mask)), B, P(ctxd), P(pm), S0)
    gb.check()
    np.testing.assert_array_equal(np_(ctxd), ctx)
    np.testing.assert_array_equal(np_(pm), head_max(ctx))
    np.testing.assert_array_equal(np_(kcd), kcp)                 # read only
    np.testing.assert_array_equal(np_(vcd), vgroup4(vcp))
    np.testing.assert_array_equal(np_(skd), skp)
    np.testing.assert_array_equal(np_(svd), svp)


def test_decode_attention_misaligned_is_invalid(gb):
    """y is read in 16-byte vectors: ldy % 4 != 0, ldy below the row width or a base off
    16 bytes is QTX_E_INVALID on the host; nothing is launched."""
    B, kv_bs = 2, 8
    y = gb.dev(np.zeros(B * 1600 + 16, f32))
    kc, vc = gb.init(np.zeros((B, kv_bs, 512), np.int8), "kc"), gb.init(np.zeros((B, 2, 512, 4), np.int8), "vc")
    sk, sv = gb.init(np.ones((B, kv_bs), f32), "skc"), gb.init(np.ones((B, kv_bs), f32), "svc")
    ctx, pm = gb.new((B, 512), f32, "ctx"), gb.new((8, B), f32, "pmax")
    step = gb.dev(np.array([0], np.int32))
    for yp, ldy in ((y.data_ptr(), 1538), (y.data_ptr(), 1024), (y.data_ptr() + 4, 1536),
                    (y.data_ptr() + 8, 1536)):
        rc = lib().qtx_decode_attention(1, C.c_void_p(yp), ldy, P(kc), P(vc), P(sk), P(sv), kv_bs,
                                        P(step), 0, S0, B, P(ctx), P(pm), S0)
        assert rc == E_INVALID, (yp - y.data_ptr(), ldy)
    gb.check()
    gb.assert_poison(ctx, "ctx")
    gb.assert_poison(pm, "pmax")
    assert not np_(kc).any() and not np_(vc).any()


# =====================================================================================
# decode tail, generator, embeddings
# =====================================================================================
def test_decode_argmax_embed(gb, gpu_model, oracle_model):
    """M = 3: ids is [M, ids_bs] and only column s + 1 may change; x_next and the two step
    words are guarded."""
    M, V, ids_bs, s = 3, 4444, 9, 4
    rng = np.random.default_rng(12)
    lg = (rng.standard_normal((M, V)) * 2).astype(f32)
    lg[1, [7, 4000]] = lg[1].max() + 1.0          # an exact tie: the exact log-softmax path
    ids0 = np.arange(M * ids_bs, dtype=np.int64).reshape(M, ids_bs) - 100
    ids = gb.init(ids0, "ids")
    step = gb.init(np.array([s, 0], np.int32), "step words")
    xn = gb.new((M, 512), f32, "x_next")
    call("qtx_decode_argmax_embed", gpu_model.handle, P(gb.dev(lg)), M, P(ids), ids_bs, P(step),
         P(xn), S0)
    gb.check()
    want = O.log_softmax_argmax(lg)[1]
    assert want[1] == 7
    ids0[:, s + 1] = want
    np.testing.assert_array_equal(np_(ids), ids0)
    np.testing.assert_array_equal(np_(step), [s + 1, 0])
    emb = oracle_model.embed(want[:, None], oracle_model.tgt_lut, pos0=s + 1)[:, 0]
    np.testing.assert_array_equal(np_(xn), emb)


@pytest.mark.parametrize("want_logp", [True, False])
def test_generator(gb, gpu_model, golden_ops, oracle_model, want_logp):
    """M = 5 (one ragged 16-row block): logp, ids and ws at exactly M * tgt_vocab floats; and
    the logp = NULL form."""
    M, V = 5, 4444
    gx = golden_ops["gen_x"]
    x = (np.concatenate([gx] * (M // len(gx) + 1))[:M]
         * np.linspace(0.1, 3, M, dtype=f32)[:, None]).astype(f32)
    logits, (lo, io) = memo("gen", lambda: (oracle_model.logits(x), oracle_model.generator(x)))
    logp = gb.new((M, V), f32, "logp")
    ids = gb.new((M,), np.int64, "ids")
    ws = gb.new((M * V,), f32, "ws", pitch_bytes=4 * V)
    call("qtx_generator", gpu_model.handle, P(gb.dev(x)), M, P(logp) if want_logp else S0,
         P(ids), P(ws), M * V * 4, S0)
    gb.check()
    np.testing.assert_array_equal(np_(ws).reshape(M, V), logits)
    np.testing.assert_array_equal(np_(ids), io)
    if want_logp:
        got = np_(logp)
        assert np.isfinite(got).all() and np.abs(got - lo).max() <= 2e-6
    else:
        gb.assert_poison(logp, "logp")
    # one byte short: QTX_E_WORKSPACE before anything is written
    ids2 = gb.new((M,), np.int64, "ids2")
    ws2 = gb.new((M * V,), f32, "ws2", pitch_bytes=4 * V)
    rc = lib().qtx_generator(gpu_model.handle, P(gb.dev(x)), M, S0, P(ids2), P(ws2),
                             M * V * 4 - 1, S0)
    assert rc == E_WORKSPACE
    gb.check()
    gb.assert_poison(ids2, "ids2")
    gb.assert_poison(ws2, "ws2")


def test_embed(gb, gpu_model, oracle_model):
    B, T, pos0 = 2, 3, 9
    ids = np.array([[5, 4443, 0], [17, 1, 2222]], np.int64)
    for which, lut in ((0, oracle_model.src_lut), (1, oracle_model.tgt_lut)):
        out = gb.new((B, T, 512), f32, "out")
        call("qtx_embed", gpu_model.handle, which, P(gb.dev(ids)), B, T, pos0, P(out), S0)
        gb.check()
        np.testing.assert_array_equal(np_(out), oracle_model.embed(ids, lut, pos0=pos0))


# =====================================================================================
# model-level calls: ws of exactly the queried size inside guards
# =====================================================================================
def make_batch(rng, B, S):
    src = np.full((B, S), 2, np.int64)
    for b, n in enumerate(rng.integers(4, S + 1, B)):
        src[b, 0] = 0
        src[b, 1:n - 1] = rng.integers(4, 5337, max(n - 2, 0))
        src[b, n - 1] = 1
    return src, (src != 2)[:, None, :]


def test_encoder_workspace(gb, gpu_model, oracle_model):
    B, S = 2, 9

    def ref():
        src, m = make_batch(np.random.default_rng(29), B, S)
        x = oracle_model.embed(src, oracle_model.src_lut)
        return x, m, oracle_model.encode(x, m)
    x, m, want = memo("enc", ref)
    h = gpu_model.handle
    nb = lib().qtx_encoder_workspace_size(h, B, S)
    assert nb > 0
    xd, md = gb.dev(x), gb.dev(m.reshape(B, S).astype(np.uint8))
    out, ws = gb.new((B, S, 512), f32, "out"), gb.new((nb,), np.uint8, "ws", pitch_bytes=S * 2048)
    assert lib().qtx_encoder_forward(h, P(xd), P(md), B, S, P(out), P(ws), nb - 1, S0) == E_WORKSPACE
    gb.check()
    gb.assert_poison(out, "out")
    gb.assert_poison(ws, "ws")
    call("qtx_encoder_forward", h, P(xd), P(md), B, S, P(out), P(ws), nb, S0)
    gpu_model.check()
    gb.check()
    np.testing.assert_array_equal(np_(out), want)


def test_decoder_workspace(gb, gpu_model, oracle_model):
    B, T, S = 2, 4, 9

    def ref():
        rng = np.random.default_rng(31)
        src, m = make_batch(rng, B, S)
        memory = oracle_model.encode(oracle_model.embed(src, oracle_model.src_lut), m)
        y = oracle_model.embed(rng.integers(0, 4444, (B, T)), oracle_model.tgt_lut)
        tm = np.tril(np.ones((T, T), np.uint8))
        return y, memory, m, tm, oracle_model.decode(y, memory, m, tm[None])
    y, memory, m, tm, want = memo("dec", ref)
    h = gpu_model.handle
    nb = lib().qtx_decoder_workspace_size(h, B, T, S)
    assert nb > 0
    args = (P(gb.dev(y)), P(gb.dev(memory)), P(gb.dev(m.reshape(B, S).astype(np.uint8))),
            P(gb.dev(tm)), 0, B, T, S)
    out, ws = gb.new((B, T, 512), f32, "out"), gb.new((nb,), np.uint8, "ws", pitch_bytes=S * 2048)
    assert lib().qtx_decoder_forward(h, *args, P(out), P(ws), nb - 1, S0) == E_WORKSPACE
    gb.check()
    gb.assert_poison(out, "out")
    gb.assert_poison(ws, "ws")
    call("qtx_decoder_forward", h, *args, P(out), P(ws), nb, S0)
    gpu_model.check()
    gb.check()
    np.testing.assert_array_equal(np_(out), want)


def test_greedy_workspace(gb, gpu_model, oracle_model):
    """(B, S, max_len) = (3, 13, 23), the shape of test_greedy_ragged_groups_matches_oracle."""
    B, S, max_len = 3, 13, 23

    def ref():
        src, m = make_batch(np.random.default_rng(B * 100 + S), B, S)
        return src, m, oracle_model.greedy_decode(src, m, max_len)
    src, m, want = memo("greedy", ref)
    h = gpu_model.handle
    nb = lib().qtx_greedy_workspace_size(h, B, S, max_len)
    assert nb > 0
    sd, md = gb.dev(src), gb.dev(m.reshape(B, S).astype(np.uint8))
    ids = gb.new((B, max_len), np.int64, "ids")
    ws = gb.new((nb,), np.uint8, "ws", pitch_bytes=S * 2048)
    assert lib().qtx_greedy_decode(h, P(sd), P(md), B, S, max_len, 0, P(ids), P(ws), nb - 1,
                                   S0) == E_WORKSPACE
    gb.check()
    gb.assert_poison(ids, "ids")
    gb.assert_poison(ws, "ws")
    call("qtx_greedy_decode", h, P(sd), P(md), B, S, max_len, 0, P(ids), P(ws), nb, S0)
    gpu_model.check()
    gb.check()
    np.testing.assert_array_equal(np_(ids), want)

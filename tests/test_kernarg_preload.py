"""Kernel-argument preload of the decode-step kernels, read from the compiled gfx950 code
object (no GPU needed): csrc/qtx_decode.hip compiled to device assembly with the product's
flags for that source (qtx/_build.py compile_flags) must give every k_skinny*, k_dec_attn*,
k_generator_mfma and k_argmax_embed kernel a non-zero
.amdhsa_user_sgpr_kernarg_preload_length — a by-value struct as the leading parameter, or a
build without -amdgpu-kernarg-preload-count, gives 0."""
import os
import re
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "onnx-transformer_amd"))
STEP_KERNELS = ("k_skinny", "k_dec_attn", "k_generator_mfma", "k_argmax_embed")


def test_step_kernels_preload_their_arguments(tmp_path):
    from qtx import _build
    try:
        hipcc = _build.hipcc()
    except RuntimeError:
        pytest.skip("hipcc not installed")
    src = os.path.join(_build.CSRC, "qtx_decode.hip")
    out = tmp_path / "decode.s"
    subprocess.run([hipcc, *_build.compile_flags(src), "--cuda-device-only", "-S", "-o", str(out), src],
                   check=True, capture_output=True, timeout=900)
    lengths, cur = {}, None
    for line in open(out):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            cur = m.group(1)
            lengths[cur] = 0        # no directive in the block: nothing preloaded
            continue
        m = re.match(r"\s*\.amdhsa_user_sgpr_kernarg_preload_length\s+(\d+)", line)
        if m and cur:
            lengths[cur] = int(m.group(1))
        if ".end_amdhsa_kernel" in line:
            cur = None
    step = {k: n for k, n in lengths.items() if any(s in k for s in STEP_KERNELS)}
    # every kernel family is there (the mangled names carry the source names)
    for s in STEP_KERNELS:
        assert any(s in k for k in step), f"no {s} kernel in the code object"
    none = sorted(k for k, n in step.items() if n == 0)
    assert not none, f"{len(none)} step kernels without preloaded arguments, e.g. {none[:3]}"

"""Kernel-argument preload of the decode-step kernels, read from the compiled gfx950 code
object (no GPU needed): every source that qtx/_build.py gives -amdgpu-kernarg-preload-count
(SOURCE_FLAGS), compiled to device assembly with the product's flags for that source
(compile_flags), must give every k_skinny*, k_dec_attn*, k_generator_mfma, k_argmax_embed,
k_tok_wide and k_top2_wide kernel in it a non-zero .amdhsa_user_sgpr_kernarg_preload_length — a
by-value struct as the leading parameter, or a build without the flag, gives 0.  The kernels'
comments rely on it (parameters in order of first use; the leading ones arrive in SGPRs)."""
import os
import re
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "onnx-transformer_amd"))
from qtx import _build  # noqa: E402

STEP_KERNELS = ("k_skinny", "k_dec_attn", "k_generator_mfma", "k_argmax_embed", "k_tok_wide",
                "k_top2_wide")
PRELOAD_SOURCES = sorted(s for s, fl in _build.SOURCE_FLAGS.items()
                         if any("-amdgpu-kernarg-preload-count" in f for f in fl))


def families_of(src):
    """The step-kernel families a source defines or instantiates: those its code (comments
    removed) names."""
    text = open(src).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return [s for s in STEP_KERNELS if re.search(r"\b" + s, text)]


def test_every_preload_source_is_a_product_source():
    assert "qtx_decode.hip" in PRELOAD_SOURCES and len(PRELOAD_SOURCES) >= 5
    assert set(PRELOAD_SOURCES) <= set(_build.SOURCES)
    for s in PRELOAD_SOURCES:
        assert "-amdgpu-kernarg-preload-count=14" in _build.compile_flags(os.path.join(_build.CSRC, s))
    # every family has a home, and the first source holds the four it always held
    homes = {f for s in PRELOAD_SOURCES for f in families_of(os.path.join(_build.CSRC, s))}
    assert homes == set(STEP_KERNELS)
    assert set(STEP_KERNELS[:4]) <= set(families_of(os.path.join(_build.CSRC, "qtx_decode.hip")))


@pytest.mark.parametrize("source", PRELOAD_SOURCES)
def test_step_kernels_preload_their_arguments(tmp_path, source):
    """Helper kernels are outside the list.  Found at length 0: none — with the flag the
    compiler preloads the leading scalars of every kernel of these sources, k_beam_ancestry
    and k_beam_anc_init (qtx_decode_beam.hip) and qtx_decode.hip's pack, mask, fault and beam
    helpers included."""
    try:
        hipcc = _build.hipcc()
    except RuntimeError:
        pytest.skip("hipcc not installed")
    src = os.path.join(_build.CSRC, source)
    families = families_of(src)
    assert families, f"{source} asks for the preload and defines no step kernel"
    out = tmp_path / "device.s"
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
    step = {k: n for k, n in lengths.items() if any(s in k for s in families)}
    # every kernel family is there (the mangled names carry the source names)
    for s in families:
        assert any(s in k for k in step), f"no {s} kernel in the code object of {source}"
    none = sorted(k for k, n in step.items() if n == 0)
    assert not none, f"{len(none)} step kernels without preloaded arguments, e.g. {none[:3]}"
    others = sorted(k for k, n in lengths.items() if n == 0 and k not in step)
    print(f"{source}: {len(step)} step kernels preloaded; other kernels at 0: {others}")

"""Teacher-forced target scoring's C-ABI and Python surface without a GPU: exported symbols,
the workspace size without a model, and the refusals that need no device (in the manner of
tests/test_scored_abi.py; the size's monotony needs a model: tests/test_gpu_score.py)."""
import ctypes
import os

from qtx import _build, _lib

NEW = ("qtx_score_workspace_size", "qtx_score_targets", "qtx_score_logits", "qtx_score_rows")
E_INVALID = 1


def test_new_symbols_exported_and_bound():
    L = ctypes.CDLL(_build.build())
    for name in NEW:
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES, name
        assert name in _lib.header_symbols(), name


def test_header_states_the_contract():
    text = open(os.path.join(_build.REPO, "include", "qtx.h")).read()
    doc = text[text.index("teacher-forced target scoring"):text.index("size_t qtx_score_workspace_size")]
    for cite in ("encoder_decoder.py:19-23", "batch.py:17-30", "train.py:28-30", "generator.py:15"):
        assert cite in doc, cite
    assert "Writes exactly" in doc


def test_workspace_size_without_model_or_shape_is_zero():
    L = _lib.lib()
    assert L.qtx_score_workspace_size(None, 2, 16, 72, 1, 0) == 0
    for args in ((0, 16, 72, 1, 0), (2, 0, 72, 1, 0), (2, 16, 1, 1, 0), (2, 16, 72, 0, 0),
                 (2, 16, 72, 1, -1)):
        assert L.qtx_score_workspace_size(None, *args) == 0, args


def test_null_and_unpaired_arguments_are_invalid_without_gpu():
    L = _lib.lib()
    one = ctypes.c_void_p(16)          # a non-null pointer that is never dereferenced
    assert L.qtx_score_targets(None, one, one, 1, 4, one, 4, 1, 2, None, 0, one, one, one, one,
                               one, 1 << 20, None) == E_INVALID
    assert b"null" in L.qtx_last_error()
    assert L.qtx_score_rows(None, one, 1, one, one, one, one, one, one, 1 << 20, None) == E_INVALID
    assert L.qtx_score_logits(None, one, 1, 8, one, one, one, one, None) == E_INVALID
    assert L.qtx_score_logits(one, one, 1, 8, None, one, one, one, None) == E_INVALID
    # top_ids without top_logp, and a one-word vocabulary
    assert L.qtx_score_logits(one, one, 1, 8, one, one, one, None, None) == E_INVALID
    assert b"pair" in L.qtx_last_error()
    assert L.qtx_score_logits(one, one, 1, 1, one, one, None, None, None) == E_INVALID
    # no rows: nothing to do, nothing dereferenced
    assert L.qtx_score_logits(one, one, 0, 8, one, one, None, None, None) == 0


def test_python_surface():
    import qtx
    from qtx import data, decode
    for name in ("score_targets", "rescore_beam", "TargetScores"):
        assert name in qtx.__all__ and getattr(qtx, name) is getattr(decode, name)
    assert hasattr(data, "perplexity") and hasattr(data, "PerplexityResult")
    from qtx.model import QtxModel
    assert callable(QtxModel.score)

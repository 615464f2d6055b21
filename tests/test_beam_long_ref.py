"""The guard of tests/test_gpu_beam_long.py's model case, on the reference alone, and the
accounting of include/qtx_beam_long.h."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_long as BL  # noqa: E402
import long_target as LT  # noqa: E402


def test_final_hypotheses_descend_through_late_moves():
    """Some final hypothesis descends through a slot whose parent at a step >= 129 was another
    slot and whose rows a later step read: an attention that ignored the ancestry table past
    position 128 would change tokens or scores of the model test."""
    ref = BL.reference()
    assert ref["steps_run"] == LT.L - 1
    moves = LT.beam_late_moves(ref)
    assert moves and all(s >= 129 for _, _, s in moves), moves


def test_header_entries_are_bound():
    """Every function of include/qtx_beam_long.h is in its ctypes table, and nothing else is."""
    from qtx import _build, _lib
    names = _lib.header_symbols(os.path.join(_build.REPO, "include", "qtx_beam_long.h"))
    assert names == sorted(_lib.SIGNATURES_BEAM_LONG) and len(names) == 2
    assert not set(names) & (set(_lib.SIGNATURES) | set(_lib.SIGNATURES_ENCTRIALS))

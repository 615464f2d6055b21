"""The accounting of include/qtx_enctrials.h: what tests/test_abi.py and tests/test_gpu_min_align.py
pin for include/qtx.h, for the second public header.  Every function it declares is exported by
the library, is in the second ctypes table (and nothing else is), and, if it takes a pointer, is
named in tests/test_gpu_enctrials.py's coverage table beside its minimum-alignment case or an
exemption with its reason."""
import ctypes
import os
import re
import sys

from qtx import _build, _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(_build.REPO, "include", "qtx_enctrials.h")


def declarations():
    """name -> parameter text of every function the header declares (comments removed)."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return dict(re.findall(r"\b(qtx_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text))


def test_header_symbols_exported_and_in_the_table():
    names = _lib.header_symbols(HEADER)
    assert names and names == sorted(declarations())
    L = ctypes.CDLL(_build.build())
    assert not [n for n in names if not hasattr(L, n)]
    assert sorted(_lib.SIGNATURES_ENCTRIALS) == names
    assert not set(_lib.SIGNATURES_ENCTRIALS) & set(_lib.SIGNATURES)
    assert set(_lib.header_symbols()) == set(_lib.SIGNATURES)      # qtx.h keeps its own set
    fn = _lib.lib().qtx_linear_rows_faults
    assert fn.argtypes is not None and len(fn.argtypes) == 5       # lib() applies the table


def test_structs_match_the_header():
    assert ctypes.sizeof(_lib.RowFault) == 40
    text = open(HEADER).read()
    fields = re.search(r"typedef struct \{(.*?)\} qtx_row_fault;", text, re.S).group(1)
    names = re.findall(r"\b([a-z]+)\s*[,;]", fields)
    assert names == [n for n, _ in _lib.RowFault._fields_]


def test_every_pointer_entry_is_accounted_for():
    import importlib
    import test_gpu_enctrials as T
    with_ptr = sorted(n for n, params in declarations().items() if "*" in params)
    assert with_ptr == sorted(set(T.COVERED) | set(T.EXEMPT))
    assert not set(T.COVERED) & set(T.EXEMPT)
    for name, where in T.COVERED.items():
        module, test = where.split("::")
        assert callable(getattr(importlib.import_module(module), test)), (name, where)
    assert all(isinstance(r, str) and r for r in T.EXEMPT.values())

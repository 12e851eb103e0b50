"""CPU checks of the row-removal ABI: the header declares and documents it,
the library exports it, the ctypes table binds it, and its null checks run
without a device."""
import re
from pathlib import Path

from rag_faiss_embedding_amd import _lib

HEADER = Path(__file__).resolve().parents[1] / "include" / "fx_index.h"


def test_header_declares_remove_ids_and_documents_its_option():
    text = HEADER.read_text()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"int\s+fx_index_remove_ids\s*\(\s*FxIndex\s*\*\s*index\s*,\s*const\s+FxSelector\s*\*\s*sel\s*,"
                     r"\s*int64_t\s*\*\s*n_removed\s*\)\s*;", code)
    assert '"remove_stage"' in text
    assert "faiss_Index_remove_ids" in text  # the call table at the top


def test_library_exports_and_binds_remove_ids():
    assert hasattr(_lib.lib, "fx_index_remove_ids")
    res, args = _lib.SIGNATURES["fx_index_remove_ids"]
    assert res is _lib._i and len(args) == 3
    assert _lib.lib.fx_index_remove_ids.argtypes == args


def test_null_arguments_without_device():
    import ctypes
    assert _lib.lib.fx_index_remove_ids(None, None, None) == -1
    assert "null" in _lib.last_error()
    n = ctypes.c_int64(7)
    assert _lib.lib.fx_index_remove_ids(None, None, ctypes.byref(n)) == -1
    assert _lib.lib.fx_index_set_option(None, b"remove_stage", 0) == -1

"""CPU checks of the range_search C ABI (include/fx_index.h): the header
declares it, the library exports it, and its argument validation needs no
device."""
import ctypes
import re
from pathlib import Path

from rag_faiss_embedding_amd import _lib

HEADER = Path(__file__).resolve().parents[1] / "include" / "fx_index.h"
NEW = ("fx_index_range_search", "fx_index_range_result", "fx_index_last_range_stats")


def test_header_declares_and_library_exports_range_search():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    names = set(re.findall(r"\b(fx_[a-z0-9_]+)\s*\(", text))
    for n in NEW:
        assert n in names, n
        assert hasattr(_lib.lib, n), n
        assert n in _lib.SIGNATURES, n


def test_header_documents_the_call_site_and_the_option():
    text = HEADER.read_text()
    assert "faiss_Index_range_search" in text
    assert '"range_cap"' in text


def test_null_index_is_an_argument_error():
    lims = (ctypes.c_int64 * 2)()
    assert _lib.lib.fx_index_range_search(None, 1, None, 0, 0, 1.0, lims) == -1
    assert _lib.lib.fx_index_range_result(None, None, None, 0) == -1
    c, p = ctypes.c_int64(0), ctypes.c_int(0)
    assert _lib.lib.fx_index_last_range_stats(None, ctypes.byref(c), ctypes.byref(p)) == -1


def test_nan_radius_is_rejected_by_name():
    lims = (ctypes.c_int64 * 2)()
    assert _lib.lib.fx_index_range_search(None, 1, None, 0, 0, float("nan"), lims) == -1
    assert "radius" in _lib.last_error()

"""CPU checks of the filtered-search C ABI (include/fx_index.h): the header
declares the selector calls, the library exports them, and their argument
validation needs no device."""
import ctypes
import re
from pathlib import Path

from rag_faiss_embedding_amd import _lib

HEADER = Path(__file__).resolve().parents[1] / "include" / "fx_index.h"
NEW = ("fx_selector_create", "fx_selector_free", "fx_selector_stats", "fx_index_search_sel")


def test_header_declares_and_library_exports_the_selector_calls():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    names = set(re.findall(r"\b(fx_[a-z0-9_]+)\s*\(", text))
    for n in NEW:
        assert n in names, n
        assert hasattr(_lib.lib, n), n
        assert n in _lib.SIGNATURES, n
    for c in ("FX_SEL_BITMAP = 0", "FX_SEL_IDS = 1", "FX_SEL_RANGE = 2"):
        assert c in text, c


def test_header_documents_the_faiss_counterparts():
    text = HEADER.read_text()
    for n in ("faiss_SearchParameters_new", "faiss_IDSelectorBatch_new", "faiss_Index_search_with_params"):
        assert n in text, n
    assert "FX_E_UNSUPPORTED" in text[text.index("fx_selector_stats"):text.index("int fx_index_search_sel")]


def test_null_arguments_are_argument_errors():
    h = ctypes.c_void_p()
    ids = (ctypes.c_int64 * 2)(1, 2)
    assert _lib.lib.fx_selector_create(None, 1, ids, 2, 0, 0, ctypes.byref(h)) == -1
    assert "index" in _lib.last_error() and not h.value
    assert _lib.lib.fx_selector_create(None, 1, ids, 2, 0, 0, None) == -1
    r, t = ctypes.c_int64(0), ctypes.c_int64(0)
    assert _lib.lib.fx_selector_stats(None, ctypes.byref(r), ctypes.byref(t)) == -1
    _lib.lib.fx_selector_free(None)  # a no-op, like free(NULL)


def test_bad_kind_is_rejected_by_name():
    h = ctypes.c_void_p()
    for kind in (3, -1, 77):
        assert _lib.lib.fx_selector_create(None, kind, None, 0, 0, 0, ctypes.byref(h)) == -1
        assert "kind" in _lib.last_error() and str(kind) in _lib.last_error()


def test_search_without_an_index_is_an_argument_error():
    assert _lib.lib.fx_index_search_sel(None, None, 1, None, 0, 0, 5, None, None, 0) == -1
    assert "index" in _lib.last_error()

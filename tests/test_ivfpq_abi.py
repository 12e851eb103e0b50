"""CPU checks of the IndexIVFPQ section of the C ABI: the header declares the fx_ivfpq_* set, the
library exports and binds it, and the arguments are validated without a device."""
import ctypes
import re
from pathlib import Path

from rag_faiss_embedding_amd import _lib

HEADER = Path(__file__).resolve().parents[1] / "include" / "fx_index.h"
IVFPQ = ["fx_ivfpq_add", "fx_ivfpq_create", "fx_ivfpq_free", "fx_ivfpq_get_centroids", "fx_ivfpq_is_trained",
         "fx_ivfpq_last_counts", "fx_ivfpq_last_plan", "fx_ivfpq_list_codes", "fx_ivfpq_list_ids",
         "fx_ivfpq_list_sizes", "fx_ivfpq_ntotal", "fx_ivfpq_profile", "fx_ivfpq_profile_read", "fx_ivfpq_reset",
         "fx_ivfpq_residuals", "fx_ivfpq_search", "fx_ivfpq_set_centroids", "fx_ivfpq_set_stream"]
E_ARG, E_UNSUPPORTED = -1, -4
TITLE = "inverted file over product-quantized codes: faiss IndexIVFPQ"


def test_header_declares_and_library_exports_the_ivfpq_set():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    names = sorted(n for n in set(re.findall(r"\b(fx_[a-z0-9_]+)\s*\(", text)) if n.startswith("fx_ivfpq_"))
    assert names == IVFPQ
    for n in IVFPQ:
        assert hasattr(_lib.lib, n) and n in _lib.SIGNATURES
    # the signatures mirror fx_ivfsq_'s where the issue says so
    for n in ("add", "search", "reset", "ntotal", "list_sizes", "list_ids", "list_codes", "set_stream", "last_counts",
              "last_plan", "profile", "profile_read", "is_trained"):
        assert _lib.SIGNATURES["fx_ivfpq_" + n] == _lib.SIGNATURES["fx_ivfsq_" + n], n
    raw = HEADER.read_text()
    assert TITLE in raw
    section = raw[raw.index(TITLE):]
    section = section[:section.index("typedef struct FxIvfPq")]
    assert "NOT checked against" in section and "decoded row" in section and "fx_ivfpq_last_plan" in section
    assert "Out of scope" in section and "FX_E_UNSUPPORTED for nbits != 8" in section
    # the parents no longer list it as out of scope
    for start in ("inverted file: faiss IndexIVFFlat", "product quantizer: faiss IndexPQ",
                  "inverted file over 8-bit codes: faiss IndexIVFScalarQuantizer"):
        sec = raw[raw.index(start):]
        sec = sec[:sec.index("typedef struct")]
        assert "IndexIVFPQ" not in sec[sec.index("Out of scope"):], start


def test_argument_validation_without_a_device():
    L = _lib.lib
    h = ctypes.c_void_p()
    x = (ctypes.c_float * 8)()
    c = (ctypes.c_uint8 * 8)()
    D = (ctypes.c_float * 4)()
    I = (ctypes.c_int64 * 4)()
    n = ctypes.c_int64(0)
    i = ctypes.c_int(0)
    assert L.fx_ivfpq_create(None, 4, 8, 2, 8, 1, 1, None) == E_ARG
    assert L.fx_ivfpq_create(None, 0, 8, 2, 8, 1, 1, ctypes.byref(h)) == E_ARG and "dimension" in _lib.last_error()
    assert L.fx_ivfpq_create(None, 4, 0, 2, 8, 1, 1, ctypes.byref(h)) == E_ARG and "nlist" in _lib.last_error()
    assert L.fx_ivfpq_create(None, 4, 1 << 31, 2, 8, 1, 1, ctypes.byref(h)) == E_UNSUPPORTED
    assert L.fx_ivfpq_create(None, 4, 8, 3, 8, 1, 1, ctypes.byref(h)) == E_ARG and "multiple of M" in _lib.last_error()
    assert L.fx_ivfpq_create(None, 4, 8, 0, 8, 1, 1, ctypes.byref(h)) == E_ARG
    assert L.fx_ivfpq_create(None, 4, 8, 2, 4, 1, 1, ctypes.byref(h)) == E_UNSUPPORTED and "nbits" in _lib.last_error()
    assert L.fx_ivfpq_create(None, 4, 8, 2, 8, 7, 1, ctypes.byref(h)) == E_ARG and "metric" in _lib.last_error()
    assert L.fx_ivfpq_create(None, 4, 8, 2, 8, 1, 1, ctypes.byref(h)) == E_ARG and "quantizer" in _lib.last_error()
    assert not h.value
    assert L.fx_ivfpq_residuals(None, 1, x, 0, 0, x, 0) == E_ARG and "null" in _lib.last_error()
    assert L.fx_ivfpq_residuals(None, -1, x, 0, 0, x, 0) == E_ARG
    assert L.fx_ivfpq_residuals(None, 1, x, 9, 0, x, 0) == E_ARG and "dtype" in _lib.last_error()
    assert L.fx_ivfpq_residuals(None, 1, x, 0, 5, x, 0) == E_ARG
    assert L.fx_ivfpq_residuals(None, 1, x, 0, 0, x, 5) == E_ARG and "out_mem" in _lib.last_error()
    assert L.fx_ivfpq_add(None, 1, x, 0, 0, None, 0) == E_ARG and "null" in _lib.last_error()
    assert L.fx_ivfpq_add(None, -1, x, 0, 0, None, 0) == E_ARG
    assert L.fx_ivfpq_add(None, 1, x, 7, 0, None, 0) == E_ARG and "dtype" in _lib.last_error()
    assert L.fx_ivfpq_add(None, 1, x, 0, 0, I, 4) == E_ARG and "ids_mem" in _lib.last_error()
    assert L.fx_ivfpq_search(None, 1, x, 0, 0, 1, 1, D, I, 0) == E_ARG and "null" in _lib.last_error()
    assert L.fx_ivfpq_search(None, 1, x, 0, 0, 0, 1, D, I, 0) == E_ARG and "k must be positive" in _lib.last_error()
    assert L.fx_ivfpq_search(None, 1, x, 0, 0, 1, 0, D, I, 0) == E_ARG and "nprobe" in _lib.last_error()
    assert L.fx_ivfpq_search(None, 1, x, 0, 0, _lib.MAX_K + 1, 1, D, I, 0) == E_UNSUPPORTED
    assert "FX_MAX_K" in _lib.last_error()
    assert L.fx_ivfpq_search(None, 1, x, 9, 0, 1, 1, D, I, 0) == E_ARG and "dtype" in _lib.last_error()
    assert L.fx_ivfpq_search(None, 1, x, 0, 3, 1, 1, D, I, 0) == E_ARG
    assert L.fx_ivfpq_is_trained(None, ctypes.byref(i)) == E_ARG
    assert L.fx_ivfpq_get_centroids(None, x) == E_ARG
    assert L.fx_ivfpq_set_centroids(None, x) == E_ARG
    assert L.fx_ivfpq_reset(None) == E_ARG
    assert L.fx_ivfpq_ntotal(None, ctypes.byref(n)) == E_ARG
    assert L.fx_ivfpq_list_sizes(None, I) == E_ARG
    assert L.fx_ivfpq_list_ids(None, 0, I, 4, ctypes.byref(n)) == E_ARG
    assert L.fx_ivfpq_list_codes(None, 0, c, 1, ctypes.byref(n)) == E_ARG
    assert L.fx_ivfpq_set_stream(None, None) == E_ARG
    assert L.fx_ivfpq_last_counts(None, ctypes.byref(n), ctypes.byref(n), ctypes.byref(n)) == E_ARG
    assert L.fx_ivfpq_last_plan(None, ctypes.byref(i), ctypes.byref(i), ctypes.byref(i), ctypes.byref(n),
                                ctypes.byref(n)) == E_ARG
    assert L.fx_ivfpq_profile(None, 1) == E_ARG
    assert L.fx_ivfpq_profile_read(None, None, None, None, None, None) == E_ARG
    L.fx_ivfpq_free(None)

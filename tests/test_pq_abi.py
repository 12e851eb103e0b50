"""CPU checks of the product-quantizer section of the C ABI: the header declares
the fx_pq_* set, the library exports and binds it, and the arguments are
validated without a device."""
import ctypes
import re
from pathlib import Path

from rag_faiss_embedding_amd import _lib

HEADER = Path(__file__).resolve().parents[1] / "include" / "fx_index.h"
PQ = ["fx_pq_add", "fx_pq_create", "fx_pq_decode", "fx_pq_encode", "fx_pq_free", "fx_pq_get_centroids",
      "fx_pq_get_codes", "fx_pq_is_trained", "fx_pq_last_counts", "fx_pq_last_plan", "fx_pq_ntotal", "fx_pq_profile",
      "fx_pq_profile_read", "fx_pq_reconstruct_batch", "fx_pq_reconstruct_n", "fx_pq_reset", "fx_pq_search",
      "fx_pq_set_centroids", "fx_pq_set_stream"]
E_ARG, E_UNSUPPORTED = -1, -4


def test_header_declares_and_library_exports_the_pq_set():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    names = sorted(n for n in set(re.findall(r"\b(fx_[a-z0-9_]+)\s*\(", text)) if n.startswith("fx_pq_"))
    assert names == PQ
    for n in PQ:
        assert hasattr(_lib.lib, n) and n in _lib.SIGNATURES
    assert "product quantizer: faiss IndexPQ" in HEADER.read_text()
    section = HEADER.read_text().split("product quantizer: faiss IndexPQ")[1].split("typedef struct FxPq")[0]
    assert "NOT checked against" in section and "fx_pq_set_centroids" in section


def test_argument_validation_without_a_device():
    L = _lib.lib
    h = ctypes.c_void_p()
    x = (ctypes.c_float * 8)()
    c = (ctypes.c_uint8 * 8)()
    D = (ctypes.c_float * 4)()
    I = (ctypes.c_int64 * 4)()
    n = ctypes.c_int64(0)
    i = ctypes.c_int(0)
    assert L.fx_pq_create(8, 2, 8, 1, 0, None) == E_ARG
    assert L.fx_pq_create(0, 2, 8, 1, 0, ctypes.byref(h)) == E_ARG and "dimension" in _lib.last_error()
    assert L.fx_pq_create(10, 4, 8, 1, 0, ctypes.byref(h)) == E_ARG and "multiple of M" in _lib.last_error()
    assert L.fx_pq_create(8, 0, 8, 1, 0, ctypes.byref(h)) == E_ARG
    assert L.fx_pq_create(8, 2, 4, 1, 0, ctypes.byref(h)) == E_UNSUPPORTED and "nbits" in _lib.last_error()
    assert L.fx_pq_create(8, 2, 8, 7, 0, ctypes.byref(h)) == E_ARG and "metric" in _lib.last_error()
    assert not h.value
    assert L.fx_pq_add(None, 1, x, 0, 0) == E_ARG and "null" in _lib.last_error()
    assert L.fx_pq_add(None, -1, x, 0, 0) == E_ARG
    assert L.fx_pq_add(None, 1, x, 7, 0) == E_ARG and "dtype" in _lib.last_error()
    assert L.fx_pq_add(None, 1, x, 0, 5) == E_ARG
    assert L.fx_pq_search(None, 1, x, 0, 0, 1, D, I, 0) == E_ARG and "null" in _lib.last_error()
    assert L.fx_pq_search(None, 1, x, 0, 0, 0, D, I, 0) == E_ARG and "k must be positive" in _lib.last_error()
    assert L.fx_pq_search(None, 1, x, 0, 0, _lib.MAX_K + 1, D, I, 0) == E_UNSUPPORTED
    assert "FX_MAX_K" in _lib.last_error()
    assert L.fx_pq_search(None, 1, x, 9, 0, 1, D, I, 0) == E_ARG and "dtype" in _lib.last_error()
    assert L.fx_pq_search(None, 1, x, 0, 3, 1, D, I, 0) == E_ARG
    assert L.fx_pq_is_trained(None, ctypes.byref(i)) == E_ARG
    assert L.fx_pq_get_centroids(None, x) == E_ARG
    assert L.fx_pq_set_centroids(None, x) == E_ARG
    assert L.fx_pq_reset(None) == E_ARG
    assert L.fx_pq_ntotal(None, ctypes.byref(n)) == E_ARG
    assert L.fx_pq_reconstruct_n(None, 0, 1, x, 0) == E_ARG
    assert L.fx_pq_reconstruct_n(None, -1, 1, x, 0) == E_ARG
    assert L.fx_pq_reconstruct_batch(None, 1, I, 0, x, 0) == E_ARG
    assert L.fx_pq_encode(None, 1, x, 0, c, 0) == E_ARG
    assert L.fx_pq_decode(None, 1, c, x, 0) == E_ARG
    assert L.fx_pq_get_codes(None, 0, 1, c, 0) == E_ARG
    assert L.fx_pq_get_codes(None, 0, 1, c, 4) == E_ARG and "out_mem" in _lib.last_error()
    assert L.fx_pq_set_stream(None, None) == E_ARG
    assert L.fx_pq_last_counts(None, ctypes.byref(n), ctypes.byref(n), ctypes.byref(n)) == E_ARG
    assert L.fx_pq_last_plan(None, ctypes.byref(i), ctypes.byref(i), ctypes.byref(i), ctypes.byref(i), ctypes.byref(n),
                             ctypes.byref(n)) == E_ARG
    assert L.fx_pq_profile(None, 1) == E_ARG
    assert L.fx_pq_profile_read(None, None, None, None, None) == E_ARG
    L.fx_pq_free(None)

"""CPU checks of the scalar-quantizer section of the C ABI: the header declares
the fx_sq_* set, the library exports and binds it, and the arguments are
validated without a device."""
import ctypes
import re
from pathlib import Path

from rag_faiss_embedding_amd import _lib

HEADER = Path(__file__).resolve().parents[1] / "include" / "fx_index.h"
SQ = ["fx_sq_add", "fx_sq_create", "fx_sq_decode", "fx_sq_encode", "fx_sq_free", "fx_sq_get_trained",
      "fx_sq_is_trained", "fx_sq_last_counts", "fx_sq_last_plan", "fx_sq_ntotal", "fx_sq_profile",
      "fx_sq_profile_read", "fx_sq_reconstruct_batch", "fx_sq_reconstruct_n", "fx_sq_reset", "fx_sq_search",
      "fx_sq_set_stream", "fx_sq_set_trained", "fx_sq_train"]
E_ARG, E_UNSUPPORTED = -1, -4


def test_header_declares_and_library_exports_the_sq_set():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    names = sorted(n for n in set(re.findall(r"\b(fx_[a-z0-9_]+)\s*\(", text)) if n.startswith("fx_sq_"))
    assert names == SQ
    for n in SQ:
        assert hasattr(_lib.lib, n) and n in _lib.SIGNATURES
    assert "scalar quantizer: faiss IndexScalarQuantizer" in HEADER.read_text()
    assert "NOT checked against" in HEADER.read_text()


def test_argument_validation_without_a_device():
    L = _lib.lib
    h = ctypes.c_void_p()
    x = (ctypes.c_float * 8)()
    c = (ctypes.c_uint8 * 8)()
    D = (ctypes.c_float * 4)()
    I = (ctypes.c_int64 * 4)()
    n = ctypes.c_int64(0)
    i = ctypes.c_int(0)
    assert L.fx_sq_create(4, 0, 1, 0, None) == E_ARG
    assert L.fx_sq_create(0, 0, 1, 0, ctypes.byref(h)) == E_ARG and "dimension" in _lib.last_error()
    assert L.fx_sq_create(4, 1, 1, 0, ctypes.byref(h)) == E_ARG and "qtype" in _lib.last_error()
    assert L.fx_sq_create(4, 0, 7, 0, ctypes.byref(h)) == E_ARG and "metric" in _lib.last_error()
    assert L.fx_sq_train(None, 1, x, 0, 0, 0) == E_ARG and "null" in _lib.last_error()
    assert L.fx_sq_train(None, -1, x, 0, 0, 0) == E_ARG
    assert L.fx_sq_train(None, 1, x, 9, 0, 0) == E_ARG and "dtype" in _lib.last_error()
    assert L.fx_sq_train(None, 1, x, 0, 5, 0) == E_ARG
    assert L.fx_sq_add(None, 1, x, 0, 0) == E_ARG and "null" in _lib.last_error()
    assert L.fx_sq_add(None, -1, x, 0, 0) == E_ARG
    assert L.fx_sq_add(None, 1, x, 7, 0) == E_ARG and "dtype" in _lib.last_error()
    assert L.fx_sq_search(None, 1, x, 0, 0, 1, D, I, 0) == E_ARG and "null" in _lib.last_error()
    assert L.fx_sq_search(None, 1, x, 0, 0, 0, D, I, 0) == E_ARG and "k must be positive" in _lib.last_error()
    assert L.fx_sq_search(None, 1, x, 0, 0, _lib.MAX_K + 1, D, I, 0) == E_UNSUPPORTED
    assert "FX_MAX_K" in _lib.last_error()
    assert L.fx_sq_search(None, 1, x, 9, 0, 1, D, I, 0) == E_ARG and "dtype" in _lib.last_error()
    assert L.fx_sq_search(None, 1, x, 0, 3, 1, D, I, 0) == E_ARG
    assert L.fx_sq_is_trained(None, ctypes.byref(i)) == E_ARG
    assert L.fx_sq_get_trained(None, x) == E_ARG
    assert L.fx_sq_set_trained(None, x) == E_ARG
    assert L.fx_sq_reset(None) == E_ARG
    assert L.fx_sq_ntotal(None, ctypes.byref(n)) == E_ARG
    assert L.fx_sq_reconstruct_n(None, 0, 1, x, 0) == E_ARG
    assert L.fx_sq_reconstruct_batch(None, 1, I, 0, x, 0) == E_ARG
    assert L.fx_sq_encode(None, 1, x, 0, c, 0) == E_ARG
    assert L.fx_sq_decode(None, 1, c, x, 0) == E_ARG
    assert L.fx_sq_set_stream(None, None) == E_ARG
    assert L.fx_sq_last_counts(None, ctypes.byref(n), ctypes.byref(n), ctypes.byref(n)) == E_ARG
    assert L.fx_sq_last_plan(None, ctypes.byref(i), ctypes.byref(i), ctypes.byref(i), ctypes.byref(i), ctypes.byref(n),
                             ctypes.byref(n)) == E_ARG
    assert L.fx_sq_profile(None, 1) == E_ARG
    assert L.fx_sq_profile_read(None, None, None, None, None) == E_ARG
    L.fx_sq_free(None)

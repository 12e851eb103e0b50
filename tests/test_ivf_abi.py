"""CPU checks of the inverted-file section of the C ABI: the header declares
the fx_ivf_* set, the library exports it, and the arguments are validated
without a device."""
import ctypes
import re
from pathlib import Path

from rag_faiss_embedding_amd import _lib

HEADER = Path(__file__).resolve().parents[1] / "include" / "fx_index.h"
IVF = ["fx_ivf_add", "fx_ivf_create", "fx_ivf_free", "fx_ivf_last_counts", "fx_ivf_last_plan", "fx_ivf_list_ids",
       "fx_ivf_list_sizes", "fx_ivf_ntotal", "fx_ivf_profile", "fx_ivf_profile_read", "fx_ivf_reset", "fx_ivf_search",
       "fx_ivf_set_stream"]
E_ARG, E_UNSUPPORTED = -1, -4


def test_header_declares_and_library_exports_the_ivf_set():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    names = sorted(n for n in set(re.findall(r"\b(fx_[a-z0-9_]+)\s*\(", text)) if n.startswith("fx_ivf_"))
    assert names == IVF
    for n in IVF:
        assert hasattr(_lib.lib, n) and n in _lib.SIGNATURES
    assert "inverted file: faiss IndexIVFFlat" in HEADER.read_text()


def test_argument_validation_without_a_device():
    L = _lib.lib
    h = ctypes.c_void_p()
    x = (ctypes.c_float * 4)()
    D = (ctypes.c_float * 4)()
    I = (ctypes.c_int64 * 4)()
    assert L.fx_ivf_create(None, 4, 8, 0, 1, ctypes.byref(h)) == E_ARG and "quantizer" in _lib.last_error()
    assert L.fx_ivf_create(None, 4, 0, 0, 1, ctypes.byref(h)) == E_ARG and "nlist" in _lib.last_error()
    assert L.fx_ivf_create(None, 4, 8, 0, 1, None) == E_ARG
    assert L.fx_ivf_search(None, 1, x, 0, 0, 1, 1, D, I, 0) == E_ARG and "null" in _lib.last_error()
    assert L.fx_ivf_search(None, 1, x, 0, 0, 0, 1, D, I, 0) == E_ARG and "k must be positive" in _lib.last_error()
    assert L.fx_ivf_search(None, 1, x, 0, 0, 1, 0, D, I, 0) == E_ARG and "nprobe" in _lib.last_error()
    assert L.fx_ivf_search(None, 1, x, 0, 0, _lib.MAX_K + 1, 1, D, I, 0) == E_UNSUPPORTED
    assert "FX_MAX_K" in _lib.last_error()
    assert L.fx_ivf_search(None, 1, x, 9, 0, 1, 1, D, I, 0) == E_ARG and "dtype" in _lib.last_error()
    assert L.fx_ivf_search(None, 1, x, 0, 3, 1, 1, D, I, 0) == E_ARG
    assert L.fx_ivf_add(None, 1, x, 0, 0, None, 0) == E_ARG and "null" in _lib.last_error()
    assert L.fx_ivf_add(None, -1, x, 0, 0, None, 0) == E_ARG
    assert L.fx_ivf_add(None, 1, x, 7, 0, None, 0) == E_ARG and "dtype" in _lib.last_error()
    n = ctypes.c_int64(0)
    assert L.fx_ivf_reset(None) == E_ARG
    assert L.fx_ivf_ntotal(None, ctypes.byref(n)) == E_ARG
    assert L.fx_ivf_list_sizes(None, None) == E_ARG
    assert L.fx_ivf_list_ids(None, 0, None, 0, ctypes.byref(n)) == E_ARG
    assert L.fx_ivf_set_stream(None, None) == E_ARG
    assert L.fx_ivf_last_counts(None, ctypes.byref(n), ctypes.byref(n), ctypes.byref(n)) == E_ARG
    assert L.fx_ivf_profile(None, 1) == E_ARG
    L.fx_ivf_free(None)

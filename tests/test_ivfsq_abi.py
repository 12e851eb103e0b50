"""CPU checks of the IndexIVFScalarQuantizer section of the C ABI: the header declares the fx_ivfsq_*
set, the library exports and binds it, and the arguments are validated without a device."""
import ctypes
import re
from pathlib import Path

from rag_faiss_embedding_amd import _lib

HEADER = Path(__file__).resolve().parents[1] / "include" / "fx_index.h"
IVFSQ = ["fx_ivfsq_add", "fx_ivfsq_create", "fx_ivfsq_free", "fx_ivfsq_get_trained", "fx_ivfsq_is_trained",
         "fx_ivfsq_last_counts", "fx_ivfsq_last_plan", "fx_ivfsq_list_codes", "fx_ivfsq_list_ids",
         "fx_ivfsq_list_sizes", "fx_ivfsq_ntotal", "fx_ivfsq_profile", "fx_ivfsq_profile_read", "fx_ivfsq_reset",
         "fx_ivfsq_search", "fx_ivfsq_set_stream", "fx_ivfsq_set_trained", "fx_ivfsq_train"]
E_ARG, E_UNSUPPORTED = -1, -4


def test_header_declares_and_library_exports_the_ivfsq_set():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    names = sorted(n for n in set(re.findall(r"\b(fx_[a-z0-9_]+)\s*\(", text)) if n.startswith("fx_ivfsq_"))
    assert names == IVFSQ
    for n in IVFSQ:
        assert hasattr(_lib.lib, n) and n in _lib.SIGNATURES
    # nothing new under the two parents' prefixes (tests/test_ivf_abi.py, tests/test_sq_abi.py pin those sets)
    assert not [n for n in IVFSQ if n.startswith("fx_ivf_") or n.startswith("fx_sq_")]
    raw = HEADER.read_text()
    assert "inverted file over 8-bit codes: faiss IndexIVFScalarQuantizer" in raw
    section = raw[raw.index("inverted file over 8-bit codes: faiss IndexIVFScalarQuantizer"):]
    section = section[:section.index("typedef struct FxIvfSq")]
    assert "NOT checked against" in section and "decode(code)|^2" in section and "reconstruct" in section
    # the parents no longer list it as out of scope
    for start in ("inverted file: faiss IndexIVFFlat", "scalar quantizer: faiss IndexScalarQuantizer"):
        sec = raw[raw.index(start):]
        sec = sec[:sec.index("typedef struct")]
        assert "IndexIVFScalarQuantizer" not in sec[sec.index("Out of scope"):], start


def test_argument_validation_without_a_device():
    L = _lib.lib
    h = ctypes.c_void_p()
    x = (ctypes.c_float * 8)()
    c = (ctypes.c_uint8 * 8)()
    D = (ctypes.c_float * 4)()
    I = (ctypes.c_int64 * 4)()
    n = ctypes.c_int64(0)
    i = ctypes.c_int(0)
    assert L.fx_ivfsq_create(None, 4, 8, 0, 1, 1, None) == E_ARG
    assert L.fx_ivfsq_create(None, 0, 8, 0, 1, 1, ctypes.byref(h)) == E_ARG and "dimension" in _lib.last_error()
    assert L.fx_ivfsq_create(None, 4, 0, 0, 1, 1, ctypes.byref(h)) == E_ARG and "nlist" in _lib.last_error()
    assert L.fx_ivfsq_create(None, 4, 1 << 31, 0, 1, 1, ctypes.byref(h)) == E_UNSUPPORTED
    assert L.fx_ivfsq_create(None, 4, 8, 1, 1, 1, ctypes.byref(h)) == E_ARG and "qtype" in _lib.last_error()
    assert L.fx_ivfsq_create(None, 4, 8, 0, 7, 1, ctypes.byref(h)) == E_ARG and "metric" in _lib.last_error()
    assert L.fx_ivfsq_create(None, 4, 8, 0, 1, 1, ctypes.byref(h)) == E_ARG and "quantizer" in _lib.last_error()
    assert not h.value
    assert L.fx_ivfsq_train(None, 1, x, 0, 0, 0) == E_ARG and "null" in _lib.last_error()
    assert L.fx_ivfsq_train(None, -1, x, 0, 0, 0) == E_ARG
    assert L.fx_ivfsq_train(None, 1, x, 9, 0, 0) == E_ARG and "dtype" in _lib.last_error()
    assert L.fx_ivfsq_train(None, 1, x, 0, 5, 0) == E_ARG
    assert L.fx_ivfsq_add(None, 1, x, 0, 0, None, 0) == E_ARG and "null" in _lib.last_error()
    assert L.fx_ivfsq_add(None, -1, x, 0, 0, None, 0) == E_ARG
    assert L.fx_ivfsq_add(None, 1, x, 7, 0, None, 0) == E_ARG and "dtype" in _lib.last_error()
    assert L.fx_ivfsq_add(None, 1, x, 0, 0, I, 4) == E_ARG and "ids_mem" in _lib.last_error()
    assert L.fx_ivfsq_search(None, 1, x, 0, 0, 1, 1, D, I, 0) == E_ARG and "null" in _lib.last_error()
    assert L.fx_ivfsq_search(None, 1, x, 0, 0, 0, 1, D, I, 0) == E_ARG and "k must be positive" in _lib.last_error()
    assert L.fx_ivfsq_search(None, 1, x, 0, 0, 1, 0, D, I, 0) == E_ARG and "nprobe" in _lib.last_error()
    assert L.fx_ivfsq_search(None, 1, x, 0, 0, _lib.MAX_K + 1, 1, D, I, 0) == E_UNSUPPORTED
    assert "FX_MAX_K" in _lib.last_error()
    assert L.fx_ivfsq_search(None, 1, x, 9, 0, 1, 1, D, I, 0) == E_ARG and "dtype" in _lib.last_error()
    assert L.fx_ivfsq_search(None, 1, x, 0, 3, 1, 1, D, I, 0) == E_ARG
    assert L.fx_ivfsq_is_trained(None, ctypes.byref(i)) == E_ARG
    assert L.fx_ivfsq_get_trained(None, x) == E_ARG
    assert L.fx_ivfsq_set_trained(None, x) == E_ARG
    assert L.fx_ivfsq_reset(None) == E_ARG
    assert L.fx_ivfsq_ntotal(None, ctypes.byref(n)) == E_ARG
    assert L.fx_ivfsq_list_sizes(None, I) == E_ARG
    assert L.fx_ivfsq_list_ids(None, 0, I, 4, ctypes.byref(n)) == E_ARG
    assert L.fx_ivfsq_list_codes(None, 0, c, 1, ctypes.byref(n)) == E_ARG
    assert L.fx_ivfsq_set_stream(None, None) == E_ARG
    assert L.fx_ivfsq_last_counts(None, ctypes.byref(n), ctypes.byref(n), ctypes.byref(n)) == E_ARG
    assert L.fx_ivfsq_last_plan(None, ctypes.byref(i), ctypes.byref(i), ctypes.byref(i), ctypes.byref(n),
                                ctypes.byref(n)) == E_ARG
    assert L.fx_ivfsq_profile(None, 1) == E_ARG
    assert L.fx_ivfsq_profile_read(None, None, None, None, None, None) == E_ARG
    L.fx_ivfsq_free(None)

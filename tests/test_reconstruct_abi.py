"""CPU checks of the read-back ABI (include/fx_index.h "stored vectors by key"):
the header declares and documents the three calls with their faiss
counterparts, the library exports them, the ctypes table binds them, and their
argument checks run without a device."""
import ctypes
import re
from pathlib import Path

from rag_faiss_embedding_amd import _lib

HEADER = Path(__file__).resolve().parents[1] / "include" / "fx_index.h"
NEW = ("fx_index_reconstruct_batch", "fx_index_search_and_reconstruct", "fx_index_compute_distance_subset")


def _code():
    return re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)


def _params(name):
    m = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)\s*;", _code())
    assert m, name
    return [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]


def test_header_declares_the_three_calls():
    assert _params(NEW[0]) == ["FxIndex* index", "int64_t n", "const int64_t* keys", "int keys_mem", "void* out",
                               "int out_dtype", "int out_mem"]
    assert _params(NEW[1]) == ["FxIndex* index", "const FxSelector* sel", "int64_t nq", "const void* q", "int q_dtype",
                               "int q_mem", "int k", "float* D", "int64_t* I", "void* R", "int r_dtype", "int out_mem"]
    assert _params(NEW[2]) == ["FxIndex* index", "int64_t nq", "const void* q", "int q_dtype", "int q_mem", "int k",
                               "const int64_t* keys", "int keys_mem", "float* D", "int out_mem"]
    assert [len(_params(n)) for n in NEW] == [7, 12, 10]


def test_library_exports_and_binds_the_calls():
    for name in NEW:
        assert hasattr(_lib.lib, name), name
        res, args = _lib.SIGNATURES[name]
        assert res is _lib._i
        assert getattr(_lib.lib, name).argtypes == args
    assert [len(_lib.SIGNATURES[n][1]) for n in NEW] == [7, 12, 10]


def test_header_names_the_faiss_counterparts_and_the_rules():
    text = HEADER.read_text()
    for name in ("faiss_Index_reconstruct_batch", "faiss_Index_search_and_reconstruct",
                 "faiss_IndexFlat_compute_distance_subset"):
        assert name in text, name
    flat = re.sub(r"[\s*]+", " ", text)
    # the NaN rule and the +-FLT_MAX rule of a key that names no row
    assert "the NaN rule" in flat and "0xFFFFFFFF" in flat and "0xFFFF" in flat and "memset(-1)" in flat
    assert "the +-FLT_MAX rule" in flat
    assert re.search(r"FLT_MAX on an L2 index and -FLT_MAX on an IP index", flat)
    assert "before an address is formed" in flat
    assert "Never recorded into or replayed from a search graph" in flat


def test_argument_checks_without_device():
    lib = _lib.lib
    keys = (ctypes.c_int64 * 2)(0, 1)
    out = (ctypes.c_float * 8)()
    D = (ctypes.c_float * 2)()
    I = (ctypes.c_int64 * 2)()
    # a null index
    assert lib.fx_index_reconstruct_batch(None, 2, keys, 0, out, _lib.F32, 0) == -1
    assert "null" in _lib.last_error()
    assert lib.fx_index_search_and_reconstruct(None, None, 1, out, 0, 0, 2, D, I, out, _lib.F32, 0) == -1
    assert lib.fx_index_compute_distance_subset(None, 1, out, 0, 0, 2, keys, 0, D, 0) == -1
    # an out_dtype that is neither fp32 nor any storage dtype: FX_E_UNSUPPORTED
    assert lib.fx_index_reconstruct_batch(None, 2, keys, 0, out, 7, 0) == -4
    assert "out_dtype" in _lib.last_error()
    assert lib.fx_index_reconstruct_batch(None, 2, keys, 0, out, -1, 0) == -4
    # a negative count
    assert lib.fx_index_reconstruct_batch(None, -1, keys, 0, out, _lib.F32, 0) == -1
    assert lib.fx_index_search_and_reconstruct(None, None, -1, out, 0, 0, 2, D, I, out, _lib.F32, 0) == -1
    assert lib.fx_index_compute_distance_subset(None, -1, out, 0, 0, 2, keys, 0, D, 0) == -1

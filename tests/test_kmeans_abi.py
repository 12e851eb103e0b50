"""CPU checks of the k-means ABI (include/fx_index.h "k-means"): the header
declares and documents the calls with their faiss counterparts, the library
exports them, the ctypes table binds them, and their argument checks run
without a device."""
import ctypes
import re
from pathlib import Path

from rag_faiss_embedding_amd import _lib

HEADER = Path(__file__).resolve().parents[1] / "include" / "fx_index.h"
NEW = ("fx_kmeans_step", "fx_kmeans_update", "fx_kmeans_finish", "fx_kmeans_status", "fx_kmeans_profile_read")


def _code():
    return re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)


def _params(name):
    m = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)\s*;", _code())
    assert m, name
    return [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]


def test_header_declares_the_calls():
    assert _params("fx_kmeans_step") == ["FxIndex* centroids", "int64_t n", "const void* x", "int x_dtype", "int x_mem",
                                         "int64_t* assign", "float* dist", "double* sums", "int64_t* counts",
                                         "double* obj", "int accumulate"]
    assert _params("fx_kmeans_update") == ["FxIndex* centroids", "int64_t n", "const void* x", "int x_dtype",
                                           "int x_mem", "const int64_t* assign", "const float* dist", "double* sums",
                                           "int64_t* counts", "double* obj", "int accumulate"]
    assert _params("fx_kmeans_finish") == ["FxIndex* centroids", "const double* sums", "const int64_t* counts",
                                           "int spherical", "float* centroids_out", "int64_t* n_split"]
    assert _params("fx_kmeans_status") == ["FxIndex* centroids", "int64_t* bad_assign"]


def test_library_exports_and_binds_the_calls():
    for name in NEW:
        assert hasattr(_lib.lib, name), name
        res, args = _lib.SIGNATURES[name]
        assert res is _lib._i
        assert getattr(_lib.lib, name).argtypes == args
    assert [len(_lib.SIGNATURES[n][1]) for n in NEW] == [11, 11, 6, 2, 5]


def test_header_names_the_faiss_counterparts_and_the_rules():
    text = HEADER.read_text()
    for name in ("faiss.Kmeans", "Clustering::train", "faiss_Clustering_train", "split_clusters"):
        assert name in text, name
    flat = re.sub(r"[\s*]+", " ", text)
    assert "forms no key and no address" in flat
    assert "no floating-point atomics" in flat
    assert "faiss draws it at random" in flat  # the donor rule, where it differs from faiss
    assert '"kmeans_chunk"' in flat and "131,072" in flat
    assert "FX_E_INTEGRITY" in flat


def test_argument_checks_without_device():
    lib = _lib.lib
    buf = (ctypes.c_double * 8)()
    # a null index
    assert lib.fx_kmeans_step(None, 1, buf, _lib.F32, 0, None, None, buf, buf, buf, 0) == -1
    assert "null index" in _lib.last_error()
    assert lib.fx_kmeans_update(None, 1, buf, _lib.F32, 0, buf, None, buf, buf, buf, 0) == -1
    assert lib.fx_kmeans_finish(None, buf, buf, 0, buf, buf) == -1
    assert lib.fx_kmeans_status(None, None) == -1
    assert lib.fx_kmeans_profile_read(None, None, None, None, None) == -1
    # n < 0, a dtype outside the three, a bad x_mem, null sums / counts / obj: FX_E_ARG, each with its message
    for call in (lib.fx_kmeans_step, lib.fx_kmeans_update):
        assert call(None, -1, buf, _lib.F32, 0, buf, None, buf, buf, buf, 0) == -1
        assert "negative n" in _lib.last_error()
        assert call(None, 1, buf, 7, 0, buf, None, buf, buf, buf, 0) == -1
        assert "dtype" in _lib.last_error()
        assert call(None, 1, buf, _lib.F32, 5, buf, None, buf, buf, buf, 0) == -1
        assert "x_mem" in _lib.last_error()
        for nulls in ((None, buf, buf), (buf, None, buf), (buf, buf, None)):
            assert call(None, 1, buf, _lib.F32, 0, buf, None, *nulls, 0) == -1
            assert "null sums" in _lib.last_error()
    for nulls in ((None, buf, buf, buf), (buf, None, buf, buf), (buf, buf, None, buf), (buf, buf, buf, None)):
        assert lib.fx_kmeans_finish(None, nulls[0], nulls[1], 0, nulls[2], nulls[3]) == -1
        assert "null buffer" in _lib.last_error()


def test_option_is_documented_with_the_others():
    flat = re.sub(r"[\s*]+", " ", HEADER.read_text())
    assert re.search(r'"kmeans_chunk" 0 \(= 131,072\) or 1 \.\. 2\^30', flat)

"""Host logic of IndexIVFPQ on CPU: the Python layer of faiss.py against a recording stand-in for the
C library, and the store's build_ivf(pq_m=) against recording stand-in indexes.  The kernels are
checked in test_ivfpq_gpu.py."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

from rag_faiss_embedding_amd import _lib
from rag_faiss_embedding_amd import faiss as fx


class _RecLib:
    """The C calls of IndexIVFPQ, recorded; every call succeeds."""

    def __init__(self, d, qntotal, M=2):
        self.d, self.M, self.qntotal, self.ntotal, self.calls, self.trained = d, M, qntotal, 0, [], False
        self.ncent = M * 256 * (d // M)
        self.lists = {0: (np.array([7, 9], dtype=np.int64), np.arange(2 * M, dtype=np.uint8).reshape(2, M))}

    def fx_index_dim(self, h, out):
        out._obj.value = self.d
        return 0

    def fx_index_ntotal(self, h, out):
        out._obj.value = self.qntotal
        return 0

    def fx_index_free(self, h):
        pass

    def fx_ivfpq_create(self, q, d, nlist, M, nbits, metric, by_residual, out):
        self.calls.append(("create", (d, nlist, M, nbits, metric, by_residual)))
        out._obj.value = 0x3000
        return 0

    def fx_ivfpq_free(self, h):
        self.calls.append(("free", ()))

    def fx_ivfpq_set_stream(self, h, s):
        return 0

    def fx_ivfpq_ntotal(self, h, out):
        out._obj.value = self.ntotal
        return 0

    def fx_ivfpq_is_trained(self, h, out):
        out._obj.value = 1 if self.trained else 0
        return 0

    def fx_ivfpq_get_centroids(self, h, out):
        self.calls.append(("get_centroids", ()))
        a = np.ctypeslib.as_array(ctypes.cast(out, ctypes.POINTER(ctypes.c_float)), shape=(self.ncent,))
        a[:] = np.arange(self.ncent, dtype=np.float32)
        return 0

    def fx_ivfpq_set_centroids(self, h, arr):
        a = np.ctypeslib.as_array(ctypes.cast(arr, ctypes.POINTER(ctypes.c_float)), shape=(self.ncent,))
        self.calls.append(("set_centroids", a.copy()))
        self.trained = True
        return 0

    def fx_ivfpq_add(self, h, n, x, code, mem, ids, imem):
        self.calls.append(("add", (n, code, mem, ids is not None, imem)))
        self.ntotal += n
        return 0

    def fx_ivfpq_search(self, h, nq, x, code, mem, k, nprobe, D, I, omem):
        self.calls.append(("search", (nq, code, mem, k, nprobe, omem)))
        return 0

    def fx_ivfpq_reset(self, h):
        self.calls.append(("reset", ()))
        self.ntotal = 0
        return 0

    def fx_ivfpq_list_codes(self, h, l, out, cap, n):
        ids, codes = self.lists.get(l, (np.zeros(0, np.int64), np.zeros((0, self.M), np.uint8)))
        n._obj.value = len(ids)
        if cap:
            ctypes.memmove(out, codes.ctypes.data, min(cap, len(ids)) * self.M)
        return 0

    def fx_ivfpq_list_ids(self, h, l, out, cap, n):
        ids, _ = self.lists.get(l, (np.zeros(0, np.int64), None))
        n._obj.value = len(ids)
        if cap:
            ctypes.memmove(out, ids.ctypes.data, min(cap, len(ids)) * 8)
        return 0

    def fx_ivfpq_last_plan(self, h, p, c, s, qb, g):
        p._obj.value, c._obj.value, s._obj.value, qb._obj.value, g._obj.value = 1, 2, 6, 37, 99
        return 0

    def fx_ivfpq_last_counts(self, h, a, b, c):
        a._obj.value, b._obj.value, c._obj.value = 3, 3, 0
        return 0


def _quantizer(d=4, qntotal=8, cls=None):
    q = (cls or fx.IndexFlatL2).__new__(cls or fx.IndexFlatL2)
    q._lib = _RecLib(d, qntotal)
    q._h = ctypes.c_void_p(1)
    q.device = 0
    q.storage_dtype = "float32"
    return q


def _ivfpq(nlist=8, qntotal=8, M=2, **kw):
    q = _quantizer(qntotal=qntotal)
    return fx.IndexIVFPQ(q, 4, nlist, M, **kw), q._lib


X = np.zeros((3, 4), dtype=np.float32)


def test_constructor_checks_the_quantizer_and_the_shape():
    ix, rec = _ivfpq(metric=fx.METRIC_INNER_PRODUCT, by_residual=False)
    assert rec.calls == [("create", (4, 8, 2, 8, 0, 0))]
    assert (ix.d, ix.nlist, ix.nprobe, ix.metric_type, ix.ntotal, ix.code_size) == (4, 8, 1, 0, 0, 2)
    assert ix.by_residual is False
    assert (ix.pq.M, ix.pq.dsub, ix.pq.ksub, ix.pq.nbits, ix.pq.code_size) == (2, 2, 256, 8, 2)
    ix, rec = _ivfpq()
    assert rec.calls == [("create", (4, 8, 2, 8, 1, 1))] and ix.by_residual is True  # faiss's defaults
    assert ix.pq.niter == 25 and ix.niter == 10
    assert issubclass(fx.IndexIVFPQ, fx.IndexIVFFlat) and fx.IndexIVFPQ._PFX == "fx_ivfpq_"
    with pytest.raises(AssertionError):
        fx.IndexIVFPQ(_quantizer(d=5), 4, 8, 2)
    with pytest.raises(AssertionError):
        fx.IndexIVFPQ(_quantizer(), 4, 8, 2, device=1)
    with pytest.raises(AssertionError):
        fx.IndexIVFPQ(object(), 4, 8, 2)
    for nbits in (4, 6, 12):
        with pytest.raises(NotImplementedError, match="not offered"):
            fx.IndexIVFPQ(_quantizer(), 4, 8, 2, nbits)
    with pytest.raises(ValueError, match="multiple of M"):
        fx.IndexIVFPQ(_quantizer(), 4, 8, 3)


def test_is_trained_needs_the_quantizer_and_the_codebook():
    ix, rec = _ivfpq(nlist=8, qntotal=0)
    assert not ix.is_trained
    rec.qntotal = 8
    assert not ix.is_trained  # centroids alone are not enough
    with pytest.raises(AssertionError, match="not trained"):
        ix.add(X)
    with pytest.raises(AssertionError, match="not trained"):
        ix.search(X, 2)
    with pytest.raises(RuntimeError, match="fewer than the 256"):
        ix.train(X)
    cents = np.arange(rec.ncent, dtype=np.float32)[::-1]
    ix.pq.centroids = cents.reshape(2, 256, 2)
    assert rec.calls[-1][0] == "set_centroids" and (rec.calls[-1][1] == cents).all() and ix.is_trained
    assert (ix.pq.centroids == np.arange(rec.ncent)).all() and rec.calls[-1] == ("get_centroids", ())
    with pytest.raises(AssertionError):
        ix.pq.centroids = cents[:5]
    n = len(rec.calls)
    ix.train(X)  # a no-op on a trained index
    assert len(rec.calls) == n
    ix.add(X)
    assert rec.calls[-1] == ("add", (3, 0, 0, False, 0)) and ix.ntotal == 3
    with pytest.raises(AssertionError, match="holds rows"):
        ix.pq.centroids = cents
    with pytest.raises(AssertionError, match="holds rows"):
        rec.trained = False
        ix.train(np.zeros((300, 4), dtype=np.float32))


def test_train_runs_one_kmeans_per_sub_quantizer_on_the_residual_slices(monkeypatch):
    ix, rec = _ivfpq(pq_niter=7, seed=99)
    x = np.arange(300 * 4, dtype=np.float32).reshape(300, 4)
    seen, runs = [], []
    monkeypatch.setattr(fx, "KMEANS_CHUNK", 128)

    def residuals(rows):
        seen.append(np.asarray(rows).shape[0])
        return torch.from_numpy(np.asarray(rows) + 1000)  # (a stand-in for fx_ivfpq_residuals)

    class Km:
        def __init__(self, d, k, niter, seed, device):
            self.args = (d, k, niter, seed, device)

        def train(self, piece):
            runs.append((self.args, piece.numpy().copy()))
            self.centroids = np.full((256, 2), len(runs), dtype=np.float32)

    monkeypatch.setattr(ix, "_residuals", residuals)
    monkeypatch.setattr(fx, "Kmeans", Km)
    ix.train(x)
    assert seen == [128, 128, 44]  # chunk by chunk
    assert [r[0] for r in runs] == [(2, 256, 7, 99, 0)] * 2
    assert (runs[0][1] == x[:, :2] + 1000).all() and (runs[1][1] == x[:, 2:] + 1000).all()
    got = rec.calls[-1]
    assert got[0] == "set_centroids" and (got[1][:512] == 1).all() and (got[1][512:] == 2).all()
    assert ix.is_trained


def test_search_takes_nprobe_and_refuses_what_is_not_offered():
    ix, rec = _ivfpq()
    rec.trained = True
    ix.search(X, 2)
    ix.nprobe = 5
    ix.search(X, 2)
    ix.search(X, 2, params=fx.SearchParametersIVF(nprobe=100))  # clamped to nlist
    assert [c[1][4] for c in rec.calls if c[0] == "search"] == [1, 5, 8]
    with pytest.raises(NotImplementedError, match="IndexIVFPQ.search takes no selector"):
        ix.search(X, 2, params=fx.SearchParametersIVF(sel=fx.IDSelectorRange(0, 2)))
    with pytest.raises(NotImplementedError, match="MAX_K"):
        ix.search(X, _lib.MAX_K + 1)
    with pytest.raises(AssertionError):
        ix.search(X, 0)
    with pytest.raises(AssertionError):
        ix.search(X, 2, params=fx.SearchParametersIVF(nprobe=0))
    with pytest.raises(NotImplementedError, match="IndexIVFPQ"):
        fx.write_index(ix, "/nonexistent/x.bin")


def test_adds_keep_one_id_mode_and_reset_keeps_the_trainings():
    ix, rec = _ivfpq()
    rec.trained = True
    ix.add_with_ids(X, np.array([5, -7, 1 << 40]))
    assert rec.calls[-1] == ("add", (3, 0, 0, True, 0))
    with pytest.raises(AssertionError, match="add_with_ids"):
        ix.add(X)
    ix.reset()
    assert rec.calls[-1] == ("reset", ()) and ix.ntotal == 0 and ix.is_trained
    ix.add(X)
    with pytest.raises(AssertionError, match="without labels"):
        ix.add_with_ids(X, np.arange(3))


def test_list_accessors_and_readers():
    ix, rec = _ivfpq()
    assert ix.get_list_ids(0).tolist() == [7, 9]
    codes = ix.get_list_codes(0)
    assert codes.dtype == np.uint8 and codes.shape == (2, 2) and codes.tolist() == [[0, 1], [2, 3]]
    assert ix.get_list_codes(3).shape == (0, 2)
    assert ix.last_ivf_plan() == {"path": "exact", "chunks": 2, "slots": 6, "q_batch": 37, "grid": 99}
    assert (ix.last_fallbacks(), ix.last_exact_fallbacks(), ix.last_dropped_candidates()) == (3, 3, 0)


# --------------------------------------------------------------------------
# the store over recording stand-in indexes
# --------------------------------------------------------------------------
class _RecIndex:
    metric_type = 1

    def __init__(self, d=4, dtype="float32", device=0):
        self.d, self.ntotal, self.calls = d, 0, []

    def add(self, x):
        self.ntotal += len(x)

    def search(self, x, k, **kw):
        self.calls.append(("search", k, kw))
        nq = np.asarray(x).shape[0]
        return (np.tile(np.arange(k, dtype=np.float32), (nq, 1)), np.tile(np.arange(k, dtype=np.int64), (nq, 1)))


class _RecIvf:
    def __init__(self, quantizer, d, nlist, metric, dtype="float32", device=0):
        self.args, self.nprobe, self.calls = (d, nlist, metric, dtype, device), 1, []

    def train(self, x):
        self.calls.append(("train", x))

    def add_from_index(self, x):
        self.calls.append(("add_from_index", x))

    def search(self, x, k, params=None):
        self.calls.append(("search", k, params.nprobe))
        nq = np.asarray(x).shape[0]
        return (np.tile(np.arange(k, dtype=np.float32), (nq, 1)),
                np.tile(np.arange(k, dtype=np.int64)[::-1].copy(), (nq, 1)))


class _RecIvfSq(_RecIvf):
    def __init__(self, quantizer, d, nlist, qtype, metric, device=0):
        self.args, self.nprobe, self.calls = (d, nlist, qtype, metric, device), 1, []


class _RecIvfPq(_RecIvf):
    def __init__(self, quantizer, d, nlist, M, nbits, metric, device=0):
        self.args, self.nprobe, self.calls = (d, nlist, M, nbits, metric, device), 1, []
        assert isinstance(quantizer, _RecIndex)


class _RecFx:
    IndexFlatL2 = _RecIndex
    IndexIVFFlat = _RecIvf
    IndexIVFScalarQuantizer = _RecIvfSq
    IndexIVFPQ = _RecIvfPq
    ScalarQuantizer = fx.ScalarQuantizer
    SearchParameters = fx.SearchParameters
    SearchParametersIVF = fx.SearchParametersIVF
    IDSelectorBatch = fx.IDSelectorBatch
    METRIC_L2 = fx.METRIC_L2

    @staticmethod
    def read_index(path, dtype="float32", device=0):
        return _RecIndex()


@pytest.fixture()
def store(monkeypatch, tmp_path):
    fs = importlib.import_module("rag_faiss_embedding_amd.faiss_store")
    monkeypatch.setattr(fs, "_fx", _RecFx)
    monkeypatch.setattr(fs.FAISSVectorStore, "_instance", None)
    monkeypatch.setattr(fs.FAISSVectorStore, "_initialized", False)
    st = fs.FAISSVectorStore(dimension=4, index_path=str(tmp_path / "none.bin"))
    st.add_vectors(np.zeros((6, 4), dtype=np.float32), [100, 101, 102, 101, 104, 105])
    return st


Q = np.zeros(4, dtype=np.float32)


def test_store_builds_product_quantized_lists_with_pq_m(store):
    ix = store.build_ivf(3, nprobe=2, pq_m=2)
    assert isinstance(ix, _RecIvfPq) and store.ivf is ix
    assert ix.args == (4, 3, 2, 8, fx.METRIC_L2, 0) and ix.nprobe == 2
    assert ix.calls == [("train", store.index), ("add_from_index", store.index)]  # the rows never leave the GPU
    D, ids = store.search(Q, 2, nprobe=5)  # search(nprobe=) uses it unchanged
    assert ix.calls[-1] == ("search", 2, 5) and ids == [101, 100]
    store.add_vectors(np.zeros((1, 4), dtype=np.float32), [7])
    assert store.ivf is None


def test_store_refuses_qtype_and_pq_m_together(store):
    with pytest.raises(ValueError, match="qtype and pq_m"):
        store.build_ivf(3, qtype=fx.ScalarQuantizer.QT_8bit, pq_m=2)
    assert store.ivf is None


def test_store_default_call_behaves_as_before(store):
    ix = store.build_ivf(3, nprobe=2)
    assert type(ix) is _RecIvf and ix.args == (4, 3, fx.METRIC_L2, "float32", 0)
    ix = store.build_ivf(3, qtype=fx.ScalarQuantizer.QT_8bit)
    assert type(ix) is _RecIvfSq and ix.args == (4, 3, fx.ScalarQuantizer.QT_8bit, fx.METRIC_L2, 0)

"""Host logic of IndexPQ on CPU: the Python layer of faiss.py against a
recording stand-in for the C library, and the store's build_pq /
search(pq=True) against recording stand-in indexes.  The kernels are checked in
test_pq_gpu.py."""
import importlib

import numpy as np
import pytest

from rag_faiss_embedding_amd import faiss as fx


class _RecLib:
    """The C calls of IndexPQ, recorded; every call succeeds."""

    def __init__(self):
        self.ntotal, self.trained, self.calls = 0, False, []

    def fx_pq_create(self, d, M, nbits, metric, device, out):
        self.calls.append(("create", (d, M, nbits, metric, device)))
        out._obj.value = 0x4000
        return 0

    def fx_pq_free(self, h):
        self.calls.append(("free", ()))

    def fx_pq_set_stream(self, h, s):
        return 0

    def fx_pq_ntotal(self, h, out):
        out._obj.value = self.ntotal
        return 0

    def fx_pq_is_trained(self, h, out):
        out._obj.value = int(self.trained)
        return 0

    def fx_pq_set_centroids(self, h, arr):
        self.calls.append(("set_centroids", ()))
        self.trained = True
        return 0

    def fx_pq_add(self, h, n, x, code, mem):
        self.calls.append(("add", (n, code, mem)))
        self.ntotal += n
        return 0

    def fx_pq_search(self, h, nq, x, code, mem, k, D, I, omem):
        self.calls.append(("search", (nq, code, mem, k, omem)))
        return 0

    def fx_pq_reset(self, h):
        self.calls.append(("reset", ()))
        self.ntotal = 0
        return 0


@pytest.fixture()
def rec(monkeypatch):
    r = _RecLib()
    monkeypatch.setattr(fx.IndexPQ, "_lib", r)
    return r


X = np.zeros((3, 16), dtype=np.float32)


def test_product_quantizer_fields(rec):
    ix = fx.IndexPQ(16, 2, 8, fx.METRIC_INNER_PRODUCT, niter=7, seed=99)
    assert rec.calls == [("create", (16, 2, 8, 0, 0))]
    pq = ix.pq
    assert (pq.M, pq.nbits, pq.dsub, pq.ksub, pq.code_size, pq.niter, pq.seed) == (2, 8, 8, 256, 2, 7, 99)
    assert (ix.d, ix.code_size, ix.metric_type, ix.ntotal, ix.is_trained) == (16, 2, 0, 0, False)
    assert fx.IndexPQ(768, 96).pq.dsub == 8


def test_bad_shapes_never_reach_the_library(rec):
    for nbits in (4, 6, 12, 16):
        with pytest.raises(NotImplementedError, match=f"nbits = {nbits}"):
            fx.IndexPQ(16, 2, nbits)
    with pytest.raises(ValueError, match="multiple of M"):
        fx.IndexPQ(10, 4)
    with pytest.raises(ValueError):
        fx.IndexPQ(16, 0)
    assert rec.calls == []


def test_lifecycle_checks_happen_before_the_library(rec):
    ix = fx.IndexPQ(16, 2)
    with pytest.raises(AssertionError, match="not trained"):
        ix.add(X)
    with pytest.raises(AssertionError, match="not trained"):
        ix.search(X, 2)
    with pytest.raises(RuntimeError, match="fewer than the 256"):
        ix.train(np.zeros((200, 16), dtype=np.float32))
    with pytest.raises(AssertionError, match="dimension"):
        ix.train(np.zeros((300, 15), dtype=np.float32))
    with pytest.raises(AssertionError, match="4096 floats"):
        ix.pq.centroids = np.zeros(100, dtype=np.float32)
    assert [c[0] for c in rec.calls] == ["create"]
    ix.pq.centroids = np.zeros((2, 256, 8), dtype=np.float32)  # faiss's flat array, any shape that holds it
    assert ix.is_trained
    ix.add(X)
    assert rec.calls[1:] == [("set_centroids", ()), ("add", (3, 0, 0))]
    with pytest.raises(AssertionError, match="holds rows"):
        ix.train(np.zeros((300, 16), dtype=np.float32))
    with pytest.raises(AssertionError, match="holds rows"):
        ix.pq.centroids = np.zeros(2 * 256 * 8, dtype=np.float32)
    n = len(rec.calls)
    with pytest.raises(AssertionError):
        ix.search(X, 0)
    with pytest.raises(NotImplementedError, match="MAX_K"):
        ix.search(X, 1025)
    with pytest.raises(NotImplementedError, match="IndexPQ.search takes no selector"):
        ix.search(X, 2, params=fx.SearchParameters(sel=fx.IDSelectorRange(0, 3)))
    with pytest.raises(AssertionError, match="dimension"):
        ix.search(np.zeros((3, 5), dtype=np.float32), 2)
    assert len(rec.calls) == n  # none of them reached the library
    ix.search(X, 2, params=fx.SearchParameters())
    assert rec.calls[-1] == ("search", (3, 0, 0, 2, 0))
    ix.reset()
    assert ix.ntotal == 0 and ix.is_trained  # the centroids stay


def test_write_index_of_a_pq_index_is_not_offered(rec, tmp_path):
    with pytest.raises(NotImplementedError, match="IndexPQ"):
        fx.write_index(fx.IndexPQ(16, 2), str(tmp_path / "x.bin"))


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

    def remove_ids(self, rows):
        self.ntotal -= len(rows)
        return len(rows)


class _RecPq:
    code_size = 2

    def __init__(self, d, M, nbits, metric, device=0):
        self.args, self.calls = (d, M, nbits, metric, device), []

    def train(self, x):
        self.calls.append(("train", x))

    def add_from_index(self, x):
        self.calls.append(("add_from_index", x))

    def search(self, x, k):
        self.calls.append(("search", k))
        nq = np.asarray(x).shape[0]
        return (np.tile(np.arange(k, dtype=np.float32), (nq, 1)),
                np.tile(np.arange(k, dtype=np.int64)[::-1].copy(), (nq, 1)))


class _RecFx:
    IndexFlatL2 = _RecIndex
    IndexPQ = _RecPq
    ScalarQuantizer = fx.ScalarQuantizer
    SearchParameters = fx.SearchParameters
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


def test_store_builds_and_uses_the_pq_index(store):
    assert store.pq is None
    pq = store.build_pq(2)
    assert store.pq is pq and pq.args == (4, 2, 8, fx.METRIC_L2, 0)
    assert pq.calls == [("train", store.index), ("add_from_index", store.index)]  # the rows never leave the GPU
    D, ids = store.search(Q, 2, pq=True)
    assert pq.calls[-1] == ("search", 2) and ids == [101, 100]  # ids are row numbers: doc_ids keeps working
    assert store.index.calls == []
    D, ids = store.search(Q, 2)
    assert store.index.calls == [("search", 2, {})] and ids == [100, 101]  # the default: the call as before
    for kw in ({"allowed_ids": [100]}, {"nprobe": 2}, {"sq": True}):  # not offered together: swallowed to empty
        D, ids = store.search(Q, 2, pq=True, **kw)
        assert ids == [] and D.size == 0
    assert len(pq.calls) == 3


def test_store_search_with_pq_needs_a_built_index(store):
    D, ids = store.search(Q, 2, pq=True)
    assert ids == [] and D.size == 0 and store.index.calls == []


@pytest.mark.parametrize("mutate", ["add_vectors", "remove_vectors", "reset", "load_index"])
def test_every_mutating_call_drops_the_pq_index(store, mutate, tmp_path):
    store.build_pq(2)
    assert store.pq is not None
    if mutate == "add_vectors":
        store.add_vectors(np.zeros((1, 4), dtype=np.float32), [7])
    elif mutate == "remove_vectors":
        assert store.remove_vectors([101]) == 2
    elif mutate == "reset":
        store.reset()
    else:
        store.load_index(str(tmp_path / "other.bin"))
    assert store.pq is None
    assert store.search(Q, 2, pq=True)[1] == []

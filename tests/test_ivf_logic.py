"""Host logic of IndexIVFFlat on CPU: the Python layer of faiss.py against a
recording stand-in for the C library, and the store's build_ivf / search(nprobe=)
against recording stand-in indexes.  The kernels are checked in test_ivf_gpu.py."""
import ctypes
import importlib

import numpy as np
import pytest

from rag_faiss_embedding_amd import faiss as fx


class _RecLib:
    """The C calls of IndexIVFFlat, recorded; every call succeeds."""

    def __init__(self, d, qntotal):
        self.d, self.qntotal, self.ntotal, self.calls = d, qntotal, 0, []

    def fx_index_dim(self, h, out):
        out._obj.value = self.d
        return 0

    def fx_index_ntotal(self, h, out):
        out._obj.value = self.qntotal
        return 0

    def fx_index_free(self, h):
        pass

    def fx_ivf_create(self, q, d, nlist, dtype, metric, out):
        self.calls.append(("create", (d, nlist, dtype, metric)))
        out._obj.value = 0x2000
        return 0

    def fx_ivf_free(self, h):
        self.calls.append(("free", ()))

    def fx_ivf_set_stream(self, h, s):
        return 0

    def fx_ivf_ntotal(self, h, out):
        out._obj.value = self.ntotal
        return 0

    def fx_ivf_add(self, h, n, x, code, mem, ids, imem):
        self.calls.append(("add", (n, code, mem, ids is not None, imem)))
        self.ntotal += n
        return 0

    def fx_ivf_search(self, h, nq, x, code, mem, k, nprobe, D, I, omem):
        self.calls.append(("search", (nq, code, mem, k, nprobe, omem)))
        return 0

    def fx_ivf_reset(self, h):
        self.calls.append(("reset", ()))
        self.ntotal = 0
        return 0


def _quantizer(d=4, qntotal=8, cls=None):
    q = (cls or fx.IndexFlatL2).__new__(cls or fx.IndexFlatL2)
    q._lib = _RecLib(d, qntotal)
    q._h = ctypes.c_void_p(1)
    q.device = 0
    q.storage_dtype = "float32"
    return q


def _ivf(nlist=8, qntotal=8, **kw):
    q = _quantizer(qntotal=qntotal)
    return fx.IndexIVFFlat(q, 4, nlist, **kw), q._lib


X = np.zeros((3, 4), dtype=np.float32)


def test_constructor_checks_the_quantizer():
    ivf, rec = _ivf(metric=fx.METRIC_INNER_PRODUCT, dtype="bfloat16")
    assert rec.calls == [("create", (4, 8, 1, 0))]
    assert (ivf.d, ivf.nlist, ivf.nprobe, ivf.metric_type, ivf.ntotal) == (4, 8, 1, 0, 0)
    with pytest.raises(AssertionError):
        fx.IndexIVFFlat(_quantizer(d=5), 4, 8)
    with pytest.raises(AssertionError):
        fx.IndexIVFFlat(_quantizer(), 4, 8, device=1)
    with pytest.raises(AssertionError):
        fx.IndexIVFFlat(object(), 4, 8)
    with pytest.raises(ValueError):
        fx.IndexIVFFlat(_quantizer(), 4, 8, dtype="int8")


def test_is_trained_follows_the_quantizer():
    ivf, rec = _ivf(nlist=8, qntotal=0)
    assert not ivf.is_trained
    with pytest.raises(AssertionError, match="not trained"):
        ivf.add(X)
    with pytest.raises(AssertionError, match="not trained"):
        ivf.search(X, 2)
    assert [c[0] for c in rec.calls] == ["create"]
    rec.qntotal = 8
    assert ivf.is_trained
    ivf.train(X)  # a no-op on a trained index
    ivf.add(X)
    assert [c[0] for c in rec.calls] == ["create", "add"]


def test_nprobe_is_clamped_and_checked():
    ivf, rec = _ivf(nlist=8)
    ivf.search(X, 2)
    ivf.nprobe = 5
    ivf.search(X, 2)
    ivf.nprobe = 50
    ivf.search(X, 2)
    ivf.search(X, 2, params=fx.SearchParametersIVF(nprobe=3))
    ivf.search(X, 2, params=fx.SearchParametersIVF(nprobe=300))
    ivf.search(X, 2, params=fx.SearchParameters())  # no nprobe of its own: the attribute's
    assert [c[1][4] for c in rec.calls if c[0] == "search"] == [1, 5, 8, 3, 8, 8]
    assert all(c[1][:4] == (3, 0, 0, 2) and c[1][5] == 0 for c in rec.calls if c[0] == "search")
    n = len(rec.calls)
    ivf.nprobe = 0
    with pytest.raises(AssertionError, match="nprobe"):
        ivf.search(X, 2)
    with pytest.raises(AssertionError, match="nprobe"):
        ivf.search(X, 2, params=fx.SearchParametersIVF(nprobe=-1))
    ivf.nprobe = 1
    with pytest.raises(AssertionError):
        ivf.search(X, 0)
    with pytest.raises(NotImplementedError):
        ivf.search(X, 1025)
    with pytest.raises(NotImplementedError, match="selector"):
        ivf.search(X, 2, params=fx.SearchParametersIVF(sel=fx.IDSelectorRange(0, 3), nprobe=2))
    assert len(rec.calls) == n  # none of them reached the library


def test_add_and_add_with_ids_do_not_mix():
    ivf, rec = _ivf()
    ivf.add(X)
    ivf.add(X)
    with pytest.raises(AssertionError, match="add_with_ids not implemented"):
        ivf.add_with_ids(X, [1, 2, 3])
    ivf.reset()
    ivf.add_with_ids(X, np.array([-5, 1 << 40, -5]))
    with pytest.raises(AssertionError, match="add does not make sense"):
        ivf.add(X)
    with pytest.raises(AssertionError, match="2 ids for 3 rows"):
        ivf.add_with_ids(X, [1, 2])
    adds = [c[1] for c in rec.calls if c[0] == "add"]
    assert adds == [(3, 0, 0, False, 0), (3, 0, 0, False, 0), (3, 0, 0, True, 0)]
    assert ivf.ntotal == 3


def test_write_index_of_an_ivf_index_is_not_offered(tmp_path):
    ivf, _ = _ivf()
    with pytest.raises(NotImplementedError):
        fx.write_index(ivf, str(tmp_path / "x.bin"))


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


class _RecIvf:
    def __init__(self, quantizer, d, nlist, metric, dtype="float32", device=0):
        self.args, self.nprobe, self.calls = (d, nlist, metric, dtype, device), 1, []
        assert isinstance(quantizer, _RecIndex)

    def train(self, x):
        self.calls.append(("train", x))

    def add_from_index(self, x):
        self.calls.append(("add_from_index", x))

    def search(self, x, k, params=None):
        self.calls.append(("search", k, params.nprobe))
        nq = np.asarray(x).shape[0]
        return (np.tile(np.arange(k, dtype=np.float32), (nq, 1)),
                np.tile(np.arange(k, dtype=np.int64)[::-1].copy(), (nq, 1)))


class _RecFx:
    IndexFlatL2 = _RecIndex
    IndexIVFFlat = _RecIvf
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


def test_store_builds_and_uses_the_ivf(store):
    assert store.ivf is None
    ivf = store.build_ivf(3, nprobe=2)
    assert store.ivf is ivf and ivf.args == (4, 3, fx.METRIC_L2, "float32", 0) and ivf.nprobe == 2
    assert ivf.calls == [("train", store.index), ("add_from_index", store.index)]  # the rows never leave the GPU
    D, ids = store.search(Q, 2, nprobe=5)
    assert ivf.calls[-1] == ("search", 2, 5) and ids == [101, 100]  # ids are row numbers: doc_ids keeps working
    assert store.index.calls == []
    D, ids = store.search(Q, 2)
    assert store.index.calls == [("search", 2, {})] and ids == [100, 101]  # without nprobe: the call as before
    assert len(ivf.calls) == 3
    D, ids = store.search(Q, 2, allowed_ids=[100], nprobe=2)  # not offered together: swallowed to empty
    assert ids == [] and D.size == 0


def test_store_search_with_nprobe_needs_a_built_ivf(store):
    D, ids = store.search(Q, 2, nprobe=2)
    assert ids == [] and D.size == 0 and store.index.calls == []


@pytest.mark.parametrize("mutate", ["add_vectors", "remove_vectors", "reset", "load_index"])
def test_every_mutating_call_drops_the_ivf(store, mutate, tmp_path):
    store.build_ivf(3)
    assert store.ivf is not None
    if mutate == "add_vectors":
        store.add_vectors(np.zeros((1, 4), dtype=np.float32), [7])
    elif mutate == "remove_vectors":
        assert store.remove_vectors([101]) == 2
    elif mutate == "reset":
        store.reset()
    else:
        store.load_index(str(tmp_path / "other.bin"))
    assert store.ivf is None
    D, ids = store.search(Q, 2, nprobe=2)
    assert ids == []

"""Host logic of IndexScalarQuantizer on CPU: the Python layer of faiss.py
against a recording stand-in for the C library, and the store's build_sq /
search(sq=True) against recording stand-in indexes.  The kernels are checked in
test_sq_gpu.py."""
import importlib

import numpy as np
import pytest

from rag_faiss_embedding_amd import faiss as fx

SQ = fx.ScalarQuantizer


class _RecLib:
    """The C calls of IndexScalarQuantizer, recorded; every call succeeds."""

    def __init__(self):
        self.ntotal, self.trained, self.calls = 0, False, []

    def fx_sq_create(self, d, qtype, metric, device, out):
        self.calls.append(("create", (d, qtype, metric, device)))
        out._obj.value = 0x3000
        return 0

    def fx_sq_free(self, h):
        self.calls.append(("free", ()))

    def fx_sq_set_stream(self, h, s):
        return 0

    def fx_sq_ntotal(self, h, out):
        out._obj.value = self.ntotal
        return 0

    def fx_sq_is_trained(self, h, out):
        out._obj.value = int(self.trained)
        return 0

    def fx_sq_train(self, h, n, x, code, mem, more):
        self.calls.append(("train", (n, code, mem, more)))
        self.trained = not more
        return 0

    def fx_sq_set_trained(self, h, arr):
        self.calls.append(("set_trained", ()))
        self.trained = True
        return 0

    def fx_sq_add(self, h, n, x, code, mem):
        self.calls.append(("add", (n, code, mem)))
        self.ntotal += n
        return 0

    def fx_sq_search(self, h, nq, x, code, mem, k, D, I, omem):
        self.calls.append(("search", (nq, code, mem, k, omem)))
        return 0

    def fx_sq_reset(self, h):
        self.calls.append(("reset", ()))
        self.ntotal = 0
        return 0


@pytest.fixture()
def sq(monkeypatch):
    rec = _RecLib()
    monkeypatch.setattr(fx.IndexScalarQuantizer, "_lib", rec)
    return fx.IndexScalarQuantizer(4), rec


X = np.zeros((3, 4), dtype=np.float32)


def test_qtype_numbers_are_faiss_s():
    assert (SQ.QT_8bit, SQ.QT_4bit, SQ.QT_8bit_uniform, SQ.QT_4bit_uniform, SQ.QT_fp16, SQ.QT_8bit_direct, SQ.QT_6bit,
            SQ.QT_bf16, SQ.QT_8bit_direct_signed) == (0, 1, 2, 3, 4, 5, 6, 7, 8)


def test_other_qtypes_never_reach_the_library(monkeypatch):
    rec = _RecLib()
    monkeypatch.setattr(fx.IndexScalarQuantizer, "_lib", rec)
    for qt, name in ((SQ.QT_4bit, "QT_4bit"), (SQ.QT_6bit, "QT_6bit"), (SQ.QT_8bit_direct, "QT_8bit_direct"),
                     (SQ.QT_4bit_uniform, "QT_4bit_uniform"), (SQ.QT_8bit_direct_signed, "QT_8bit_direct_signed")):
        with pytest.raises(NotImplementedError, match=name):
            fx.IndexScalarQuantizer(4, qt)
    with pytest.raises(NotImplementedError, match='QT_fp16.*dtype="float16"'):
        fx.IndexScalarQuantizer(4, SQ.QT_fp16)
    with pytest.raises(NotImplementedError, match='QT_bf16.*dtype="bfloat16"'):
        fx.IndexScalarQuantizer(4, SQ.QT_bf16)
    assert rec.calls == []
    ix = fx.IndexScalarQuantizer(4, SQ.QT_8bit_uniform, fx.METRIC_INNER_PRODUCT)
    assert rec.calls == [("create", (4, 2, 0, 0))]
    assert (ix.d, ix.code_size, ix.metric_type, ix.ntotal, ix.is_trained) == (4, 4, 0, 0, False)


def test_lifecycle_checks_happen_before_the_library(sq):
    ix, rec = sq
    with pytest.raises(AssertionError, match="not trained"):
        ix.add(X)
    with pytest.raises(AssertionError, match="not trained"):
        ix.search(X, 2)
    assert [c[0] for c in rec.calls] == ["create"]
    ix.train(X)
    ix.add(X)
    assert rec.calls[1:] == [("train", (3, 0, 0, 0)), ("add", (3, 0, 0))]
    with pytest.raises(AssertionError, match="holds rows"):
        ix.train(X)
    with pytest.raises(AssertionError, match="holds rows"):
        ix.set_trained(np.zeros(8, dtype=np.float32))
    n = len(rec.calls)
    with pytest.raises(AssertionError):
        ix.search(X, 0)
    with pytest.raises(NotImplementedError):
        ix.search(X, 1025)
    with pytest.raises(NotImplementedError, match="selector"):
        ix.search(X, 2, params=fx.SearchParameters(sel=fx.IDSelectorRange(0, 3)))
    with pytest.raises(AssertionError, match="dimension"):
        ix.search(np.zeros((3, 5), dtype=np.float32), 2)
    assert len(rec.calls) == n  # none of them reached the library
    ix.search(X, 2, params=fx.SearchParameters())
    assert rec.calls[-1] == ("search", (3, 0, 0, 2, 0))
    ix.reset()
    assert ix.ntotal == 0 and ix.is_trained  # the training stays
    ix.set_trained(np.zeros(8, dtype=np.float32))
    with pytest.raises(AssertionError, match="8 floats"):
        ix.set_trained(np.zeros(7, dtype=np.float32))


def test_write_index_of_an_sq_index_is_not_offered(sq, tmp_path):
    with pytest.raises(NotImplementedError):
        fx.write_index(sq[0], str(tmp_path / "x.bin"))


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


class _RecSq:
    code_size = 4

    def __init__(self, d, qtype, metric, device=0):
        self.args, self.calls = (d, qtype, metric, device), []

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
    IndexScalarQuantizer = _RecSq
    ScalarQuantizer = SQ
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


def test_store_builds_and_uses_the_sq_index(store):
    assert store.sq is None
    sq = store.build_sq()
    assert store.sq is sq and sq.args == (4, SQ.QT_8bit, fx.METRIC_L2, 0)
    assert sq.calls == [("train", store.index), ("add_from_index", store.index)]  # the rows never leave the GPU
    D, ids = store.search(Q, 2, sq=True)
    assert sq.calls[-1] == ("search", 2) and ids == [101, 100]  # ids are row numbers: doc_ids keeps working
    assert store.index.calls == []
    D, ids = store.search(Q, 2)
    assert store.index.calls == [("search", 2, {})] and ids == [100, 101]  # the default: the call as before
    assert len(sq.calls) == 3
    D, ids = store.search(Q, 2, allowed_ids=[100], sq=True)  # not offered together: swallowed to empty
    assert ids == [] and D.size == 0


def test_store_search_with_sq_needs_a_built_index(store):
    D, ids = store.search(Q, 2, sq=True)
    assert ids == [] and D.size == 0 and store.index.calls == []


@pytest.mark.parametrize("mutate", ["add_vectors", "remove_vectors", "reset", "load_index"])
def test_every_mutating_call_drops_the_sq_index(store, mutate, tmp_path):
    store.build_sq(SQ.QT_8bit_uniform)
    assert store.sq is not None and store.sq.args[1] == 2
    if mutate == "add_vectors":
        store.add_vectors(np.zeros((1, 4), dtype=np.float32), [7])
    elif mutate == "remove_vectors":
        assert store.remove_vectors([101]) == 2
    elif mutate == "reset":
        store.reset()
    else:
        store.load_index(str(tmp_path / "other.bin"))
    assert store.sq is None
    D, ids = store.search(Q, 2, sq=True)
    assert ids == []

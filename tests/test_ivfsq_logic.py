"""Host logic of IndexIVFScalarQuantizer on CPU: the Python layer of faiss.py against a recording
stand-in for the C library, and the store's build_ivf(qtype=) against recording stand-in indexes.
The kernels are checked in test_ivfsq_gpu.py."""
import ctypes
import importlib

import numpy as np
import pytest

from rag_faiss_embedding_amd import _lib
from rag_faiss_embedding_amd import faiss as fx

SQ = fx.ScalarQuantizer


class _RecLib:
    """The C calls of IndexIVFScalarQuantizer, recorded; every call succeeds."""

    def __init__(self, d, qntotal):
        self.d, self.qntotal, self.ntotal, self.calls, self.trained = d, qntotal, 0, [], False
        self.lists = {0: (np.array([7, 9], dtype=np.int64), np.arange(2 * d, dtype=np.uint8).reshape(2, d))}

    def fx_index_dim(self, h, out):
        out._obj.value = self.d
        return 0

    def fx_index_ntotal(self, h, out):
        out._obj.value = self.qntotal
        return 0

    def fx_index_free(self, h):
        pass

    def fx_ivfsq_create(self, q, d, nlist, qtype, metric, by_residual, out):
        self.calls.append(("create", (d, nlist, qtype, metric, by_residual)))
        out._obj.value = 0x3000
        return 0

    def fx_ivfsq_free(self, h):
        self.calls.append(("free", ()))

    def fx_ivfsq_set_stream(self, h, s):
        return 0

    def fx_ivfsq_ntotal(self, h, out):
        out._obj.value = self.ntotal
        return 0

    def fx_ivfsq_is_trained(self, h, out):
        out._obj.value = 1 if self.trained else 0
        return 0

    def fx_ivfsq_train(self, h, n, x, code, mem, more):
        self.calls.append(("train", (n, code, mem, more)))
        self.trained = not more
        return 0

    def fx_ivfsq_get_trained(self, h, out):
        self.calls.append(("get_trained", ()))
        a = np.ctypeslib.as_array(ctypes.cast(out, ctypes.POINTER(ctypes.c_float)), shape=(2 * self.d,))
        a[:self.d], a[self.d:] = -1.0, 2.0
        return 0

    def fx_ivfsq_set_trained(self, h, arr):
        a = np.ctypeslib.as_array(ctypes.cast(arr, ctypes.POINTER(ctypes.c_float)), shape=(2 * self.d,))
        self.calls.append(("set_trained", tuple(a.tolist())))
        self.trained = True
        return 0

    def fx_ivfsq_add(self, h, n, x, code, mem, ids, imem):
        self.calls.append(("add", (n, code, mem, ids is not None, imem)))
        self.ntotal += n
        return 0

    def fx_ivfsq_search(self, h, nq, x, code, mem, k, nprobe, D, I, omem):
        self.calls.append(("search", (nq, code, mem, k, nprobe, omem)))
        return 0

    def fx_ivfsq_reset(self, h):
        self.calls.append(("reset", ()))
        self.ntotal = 0
        return 0

    def fx_ivfsq_list_codes(self, h, l, out, cap, n):
        ids, codes = self.lists.get(l, (np.zeros(0, np.int64), np.zeros((0, self.d), np.uint8)))
        n._obj.value = len(ids)
        if cap:
            ctypes.memmove(out, codes.ctypes.data, min(cap, len(ids)) * self.d)
        return 0

    def fx_ivfsq_list_ids(self, h, l, out, cap, n):
        ids, _ = self.lists.get(l, (np.zeros(0, np.int64), None))
        n._obj.value = len(ids)
        if cap:
            ctypes.memmove(out, ids.ctypes.data, min(cap, len(ids)) * 8)
        return 0

    def fx_ivfsq_last_plan(self, h, p, c, s, qb, g):
        p._obj.value, c._obj.value, s._obj.value, qb._obj.value, g._obj.value = 1, 2, 6, 37, 99
        return 0

    def fx_ivfsq_last_counts(self, h, a, b, c):
        a._obj.value, b._obj.value, c._obj.value = 3, 3, 0
        return 0


def _quantizer(d=4, qntotal=8, cls=None):
    q = (cls or fx.IndexFlatL2).__new__(cls or fx.IndexFlatL2)
    q._lib = _RecLib(d, qntotal)
    q._h = ctypes.c_void_p(1)
    q.device = 0
    q.storage_dtype = "float32"
    return q


def _ivfsq(nlist=8, qntotal=8, **kw):
    q = _quantizer(qntotal=qntotal)
    return fx.IndexIVFScalarQuantizer(q, 4, nlist, **kw), q._lib


X = np.zeros((3, 4), dtype=np.float32)


def test_constructor_checks_the_quantizer_and_the_qtype():
    ix, rec = _ivfsq(qtype=SQ.QT_8bit_uniform, metric=fx.METRIC_INNER_PRODUCT, by_residual=False)
    assert rec.calls == [("create", (4, 8, 2, 0, 0))]
    assert (ix.d, ix.nlist, ix.nprobe, ix.metric_type, ix.ntotal, ix.code_size) == (4, 8, 1, 0, 0, 4)
    assert ix.by_residual is False and ix.qtype == SQ.QT_8bit_uniform
    ix, rec = _ivfsq()
    assert rec.calls == [("create", (4, 8, 0, 1, 1))] and ix.by_residual is True  # faiss's defaults
    with pytest.raises(AssertionError):
        fx.IndexIVFScalarQuantizer(_quantizer(d=5), 4, 8)
    with pytest.raises(AssertionError):
        fx.IndexIVFScalarQuantizer(_quantizer(), 4, 8, device=1)
    with pytest.raises(AssertionError):
        fx.IndexIVFScalarQuantizer(object(), 4, 8)
    for qt in (SQ.QT_4bit, SQ.QT_fp16, SQ.QT_6bit, 77):
        with pytest.raises(NotImplementedError, match="not offered"):
            fx.IndexIVFScalarQuantizer(_quantizer(), 4, 8, qt)


def test_is_trained_needs_the_quantizer_and_the_tables():
    ix, rec = _ivfsq(nlist=8, qntotal=0)
    assert not ix.is_trained
    rec.qntotal = 8
    assert not ix.is_trained  # centroids alone are not enough
    with pytest.raises(AssertionError, match="not trained"):
        ix.add(X)
    with pytest.raises(AssertionError, match="not trained"):
        ix.search(X, 2)
    ix.train(X)  # the quantizer holds its centroids: only the tables are trained
    assert rec.calls[-1] == ("train", (3, 0, 0, 0)) and ix.is_trained
    n = len(rec.calls)
    ix.train(X)  # a no-op on a trained index
    assert len(rec.calls) == n
    ix.add(X)
    assert rec.calls[-1] == ("add", (3, 0, 0, False, 0)) and ix.ntotal == 3
    with pytest.raises(AssertionError, match="holds rows"):
        rec.trained = False
        ix.train(X)


def test_trained_round_trip_and_uniform_form():
    ix, rec = _ivfsq()
    t = ix.trained
    assert t.shape == (8,) and (t[:4] == -1).all() and (t[4:] == 2).all()
    ix.set_trained(t)
    assert rec.calls[-1] == ("set_trained", (-1.0,) * 4 + (2.0,) * 4) and ix.is_trained
    with pytest.raises(AssertionError):
        ix.set_trained(t[:3])
    ux, urec = _ivfsq(qtype=SQ.QT_8bit_uniform)
    assert ux.trained.tolist() == [-1.0, 2.0]
    ux.set_trained([0.5, 3.0])
    assert urec.calls[-1] == ("set_trained", (0.5,) * 4 + (3.0,) * 4)
    qx, _ = _ivfsq(qntotal=0)
    with pytest.raises(AssertionError, match="quantizer"):
        qx.set_trained(t)


def test_search_takes_nprobe_and_refuses_what_is_not_offered():
    ix, rec = _ivfsq()
    rec.trained = True
    ix.search(X, 2)
    ix.nprobe = 5
    ix.search(X, 2)
    ix.search(X, 2, params=fx.SearchParametersIVF(nprobe=100))  # clamped to nlist
    assert [c[1][4] for c in rec.calls if c[0] == "search"] == [1, 5, 8]
    with pytest.raises(NotImplementedError, match="IndexIVFScalarQuantizer.search takes no selector"):
        ix.search(X, 2, params=fx.SearchParametersIVF(sel=fx.IDSelectorRange(0, 2)))
    with pytest.raises(NotImplementedError, match="MAX_K"):
        ix.search(X, _lib.MAX_K + 1)
    with pytest.raises(AssertionError):
        ix.search(X, 0)
    with pytest.raises(AssertionError):
        ix.search(X, 2, params=fx.SearchParametersIVF(nprobe=0))
    with pytest.raises(NotImplementedError, match="IndexIVFScalarQuantizer"):
        fx.write_index(ix, "/nonexistent/x.bin")


def test_adds_keep_one_id_mode_and_reset_keeps_the_trainings():
    ix, rec = _ivfsq()
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
    with pytest.raises(AssertionError, match="ids for"):
        ix.reset()
        ix.add_with_ids(X, np.arange(2))


def test_list_accessors_and_readers():
    ix, rec = _ivfsq()
    assert ix.get_list_ids(0).tolist() == [7, 9]
    codes = ix.get_list_codes(0)
    assert codes.dtype == np.uint8 and codes.shape == (2, 4) and codes.tolist() == [[0, 1, 2, 3], [4, 5, 6, 7]]
    assert ix.get_list_codes(3).shape == (0, 4)
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
        assert isinstance(quantizer, _RecIndex)


class _RecFx:
    IndexFlatL2 = _RecIndex
    IndexIVFFlat = _RecIvf
    IndexIVFScalarQuantizer = _RecIvfSq
    ScalarQuantizer = SQ
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


def test_store_builds_the_8_bit_lists_with_a_qtype(store):
    ix = store.build_ivf(3, nprobe=2, qtype=SQ.QT_8bit)
    assert isinstance(ix, _RecIvfSq) and store.ivf is ix
    assert ix.args == (4, 3, SQ.QT_8bit, fx.METRIC_L2, 0) and ix.nprobe == 2
    assert ix.calls == [("train", store.index), ("add_from_index", store.index)]  # the rows never leave the GPU
    D, ids = store.search(Q, 2, nprobe=5)  # search(nprobe=) uses it unchanged
    assert ix.calls[-1] == ("search", 2, 5) and ids == [101, 100]
    D, ids = store.search(Q, 2)
    assert store.index.calls == [("search", 2, {})] and ids == [100, 101]
    D, ids = store.search(Q, 2, sq=True, nprobe=2)  # not offered together, as before: swallowed to empty
    assert ids == [] and D.size == 0
    store.add_vectors(np.zeros((1, 4), dtype=np.float32), [7])
    assert store.ivf is None


def test_store_without_a_qtype_builds_the_flat_lists_as_before(store):
    ix = store.build_ivf(3, nprobe=2)
    assert type(ix) is _RecIvf and ix.args == (4, 3, fx.METRIC_L2, "float32", 0)

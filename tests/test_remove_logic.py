"""CPU checks of the Python side of row removal: ``_FlatIndex.remove_ids``
over a recording stand-in for the C library, and the store / retrieval layers
(``FAISSVectorStore.remove_vectors``, ``RetrievalEngine.remove_documents``)
over a recording stand-in index, as tests/test_select_logic.py fakes them."""
import ctypes
import importlib

import numpy as np
import pytest

from rag_faiss_embedding_amd import faiss as fx


class _RecLib:
    """The C calls of ``remove_ids``, recorded; a removal takes ``gone`` rows."""

    def __init__(self, d, ntotal, gone):
        self.d, self.ntotal, self.gone, self.calls, self.freed = d, ntotal, gone, [], []

    def fx_index_dim(self, h, out):
        out._obj.value = self.d
        return 0

    def fx_index_ntotal(self, h, out):
        out._obj.value = self.ntotal
        return 0

    def fx_index_set_stream(self, h, s):
        return 0

    def fx_selector_create(self, h, kind, data, n, mem, invert, out):
        ids = None
        if kind == 1 and n:
            ids = np.ctypeslib.as_array(ctypes.cast(data, ctypes.POINTER(ctypes.c_int64)), shape=(n,)).tolist()
        self.calls.append(("create", (kind, n, mem, invert), ids))
        out._obj.value = 0x1000 + len(self.calls)
        return 0

    def fx_selector_free(self, h):
        self.freed.append(h.value)

    def fx_index_remove_ids(self, h, sel, out):
        self.calls.append(("remove", sel.value))
        out._obj.value = self.gone
        self.ntotal -= self.gone
        return 0

    def fx_index_search_sel(self, *a):
        self.calls.append(("search_sel", a[1].value))
        return 0

    def fx_index_free(self, h):
        pass


def _stand_in(d=4, ntotal=10, gone=2):
    ix = fx.IndexFlatL2.__new__(fx.IndexFlatL2)
    ix._lib = _RecLib(d, ntotal, gone)
    ix._h = ctypes.c_void_p(1)
    ix.device = 0
    return ix


def test_remove_ids_accepts_a_selector_a_list_and_an_array():
    ix = _stand_in(gone=2)
    assert ix.remove_ids(fx.IDSelectorRange(3, 5)) == 2
    assert ix.remove_ids([1, 7]) == 2
    assert ix.remove_ids(np.array([0, 2], dtype=np.int32)) == 2
    assert ix.remove_ids(fx.IDSelectorNot(fx.IDSelectorBatch([0, 1]))) == 2
    kinds = [c[1] for c in ix._lib.calls if c[0] == "create"]
    assert kinds == [(2, 2, 0, 0), (1, 2, 0, 0), (1, 2, 0, 0), (1, 2, 0, 1)]
    assert [c[2] for c in ix._lib.calls if c[0] == "create"][1:3] == [[1, 7], [0, 2]]
    # each removal got the handle created right before it
    for i in range(0, 8, 2):
        assert ix._lib.calls[i][0] == "create" and ix._lib.calls[i + 1] == ("remove", 0x1000 + i + 1)
    assert ix.ntotal == 2


def test_a_removal_invalidates_cached_selectors_even_when_ntotal_returns():
    ix = _stand_in(ntotal=10, gone=1)
    sel = fx.IDSelectorRange(0, 5)
    p = fx.SearchParameters(sel=sel)
    xq = np.zeros((1, 4), dtype=np.float32)
    ix.search(xq, 3, params=p)
    first = ix._lib.calls[-1][1]
    assert ix.remove_ids([9]) == 1
    ix._lib.ntotal = 10  # an add of as many rows: the key's ntotal is back, its counter is not
    ix.search(xq, 3, params=p)
    assert ix._lib.calls[-2][0] == "create" and ix._lib.calls[-1][1] != first
    assert first in ix._lib.freed
    # nothing removed: the cache stays
    ix._lib.gone = 0
    n_created = sum(c[0] == "create" for c in ix._lib.calls)
    assert ix.remove_ids(sel) == 0
    ix.search(xq, 3, params=p)
    assert sum(c[0] == "create" for c in ix._lib.calls) == n_created


# --------------------------------------------------------------------------
# store and retrieval layers over a recording stand-in index
# --------------------------------------------------------------------------
class _RecIndex:
    """Records what remove_ids is called with; removes the rows it is given."""

    metric_type = 1

    def __init__(self, d=4, dtype="float32", device=0):
        self.d, self.ntotal, self.removed = d, 0, []

    def add(self, x):
        self.ntotal += len(x)

    def remove_ids(self, x):
        rows = sorted(set(int(r) for r in np.asarray(x).reshape(-1) if 0 <= r < self.ntotal))
        self.removed.append(np.asarray(x).reshape(-1).tolist())
        self.ntotal -= len(rows)
        return len(rows)


class _RecFx:
    IndexFlatL2 = _RecIndex
    SearchParameters = fx.SearchParameters
    IDSelectorBatch = fx.IDSelectorBatch


@pytest.fixture()
def store(monkeypatch, tmp_path):
    fs = importlib.import_module("rag_faiss_embedding_amd.faiss_store")
    monkeypatch.setattr(fs, "_fx", _RecFx)
    monkeypatch.setattr(fs.FAISSVectorStore, "_instance", None)
    monkeypatch.setattr(fs.FAISSVectorStore, "_initialized", False)
    st = fs.FAISSVectorStore(dimension=4, index_path=str(tmp_path / "none.bin"))
    st.add_vectors(np.zeros((6, 4), dtype=np.float32), [100, 101, 102, 101, 104, 105])
    return st


def test_store_remove_vectors(store):
    assert store.remove_vectors([]) == 0 and store.remove_vectors([999, 7]) == 0  # nothing / unknown ids
    assert store.index.removed == [] and store.index.ntotal == 6
    assert store.remove_vectors([101, 999]) == 2  # an id that occurs twice removes both rows
    assert store.index.removed == [[1, 3]]
    assert store.doc_ids == [100, 102, 104, 105] and store.index.ntotal == 4
    assert store.remove_vectors({105, 100}) == 2
    assert store.index.removed[1] == [0, 3] and store.doc_ids == [102, 104]


def test_store_leaves_rows_beyond_doc_ids_alone(store):
    store.index.add(np.zeros((3, 4), dtype=np.float32))  # rows without ids (add_vectors does not check counts)
    assert store.index.ntotal == 9
    assert store.remove_vectors([105, 6, 7, 8]) == 1  # (6, 7, 8 are row numbers, not document ids)
    assert store.index.removed == [[5]] and store.index.ntotal == 8
    assert store.doc_ids == [100, 101, 102, 101, 104]
    # ids recorded for rows that never went in are no rows either
    store.doc_ids.extend([200, 201, 202, 203, 204])
    assert store.remove_vectors([204]) == 0 and store.doc_ids[-1] == 204
    assert store.remove_vectors([202, 100]) == 2 and store.index.removed[-1] == [0, 7]
    assert store.doc_ids == [101, 102, 101, 104, 200, 201, 203, 204]


def test_store_errors_propagate(store):
    def boom(x):
        raise RuntimeError("no")
    store.index.remove_ids = boom
    with pytest.raises(RuntimeError):
        store.remove_vectors([100])
    assert store.doc_ids == [100, 101, 102, 101, 104, 105]


def test_engine_remove_documents():
    from rag_faiss_embedding_amd import retrieval as R
    ix = _RecIndex()
    ix.add(np.zeros((7, 4), dtype=np.float32))
    doc_ids = [100, 101, 102, 101, 104]  # rows 5 and 6 carry no id
    eng = R.RetrievalEngine(None, ix, doc_ids, None)
    assert eng.remove_documents([]) == 0 and eng.remove_documents([5, 6, 999]) == 0 and ix.removed == []
    assert eng.remove_documents([101, 104, 999]) == 3
    assert ix.removed == [[1, 3, 4]] and ix.ntotal == 4
    assert eng.doc_ids == [100, 102]
    assert doc_ids == [100, 101, 102, 101, 104]  # the engine works on its own copy
    assert eng.remove_documents(iter([100])) == 1 and eng.doc_ids == [102] and ix.removed[1] == [0]

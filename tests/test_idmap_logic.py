"""CPU checks of the Python side of stable ids: ``IndexIDMap`` / ``IndexIDMap2``
over a recording stand-in index, and ``_FlatIndex.add_with_ids`` /
``rows_of_ids`` / ``get_ids`` / ``read_index`` over a recording stand-in for
the C library, as tests/test_remove_logic.py fakes them."""
import ctypes

import numpy as np
import pytest

from rag_faiss_embedding_amd import _lib
from rag_faiss_embedding_amd import faiss as fx


class _FakeFlat:
    """What the wrappers call on the flat index, recorded."""

    d, metric_type, is_trained = 8, fx.METRIC_L2, True

    def __init__(self, ntotal=0):
        self.ntotal, self.calls, self._resets = ntotal, [], 0
        self.labels = np.zeros(0, dtype=np.int64)

    def add_with_ids(self, x, ids):
        # (the real binding's length rule)
        assert len(ids) == len(x), f"add_with_ids: {len(ids)} ids for {len(x)} rows"
        self.calls.append(("add_with_ids", len(x)))
        self.labels = np.concatenate([self.labels, np.asarray(ids, dtype=np.int64)])
        self.ntotal += len(x)

    def search(self, x, k, *, params=None, D=None, I=None):
        self.calls.append(("search", k, params, D, I))
        return "D", "I"

    def range_search(self, x, radius, *, params=None):
        self.calls.append(("range_search", radius, params))
        return "lims", "D", "I"

    def remove_ids(self, x):
        self.calls.append(("remove_ids", x))
        self._resets += 1
        return 3

    def reset(self):
        self.calls.append(("reset",))
        self.ntotal = 0
        self._resets += 1

    def get_ids(self):
        return self.labels

    def rows_of_ids(self, ids):
        self.calls.append(("rows_of_ids", np.asarray(ids).tolist()))
        return np.array([int(np.flatnonzero(self.labels == v)[-1]) if (self.labels == v).any() else -1 for v in ids])

    def reconstruct_n(self, i0, n):
        self.calls.append(("reconstruct_n", i0, n))
        return np.full((n, self.d), float(i0), dtype=np.float32)


def test_wrapped_index_must_be_empty():
    with pytest.raises(AssertionError, match="empty"):
        fx.IndexIDMap(_FakeFlat(ntotal=4))
    with pytest.raises(AssertionError, match="empty"):
        fx.IndexIDMap2(_FakeFlat(ntotal=1))
    flat = _FakeFlat()
    assert fx.IndexIDMap2(flat).index is flat


def test_attributes_follow_the_wrapped_index():
    flat = _FakeFlat()
    idx = fx.IndexIDMap(flat)
    assert (idx.d, idx.ntotal, idx.metric_type, idx.is_trained) == (8, 0, fx.METRIC_L2, True)
    idx.add_with_ids(np.zeros((5, 8), dtype=np.float32), np.arange(5))
    assert idx.ntotal == 5 and idx.id_map.tolist() == [0, 1, 2, 3, 4]
    assert issubclass(fx.IndexIDMap2, fx.IndexIDMap)


def test_add_is_refused_and_lengths_must_match():
    idx = fx.IndexIDMap(_FakeFlat())
    with pytest.raises(RuntimeError, match="add_with_ids"):
        idx.add(np.zeros((2, 8), dtype=np.float32))
    with pytest.raises(AssertionError):
        idx.add_with_ids(np.zeros((2, 8), dtype=np.float32), [1, 2, 3])
    assert idx.ntotal == 0 and idx.index.calls == []


def test_calls_go_to_the_wrapped_index_and_bump_its_resets():
    flat = _FakeFlat()
    idx = fx.IndexIDMap2(flat)
    idx.add_with_ids(np.zeros((4, 8), dtype=np.float32), [10, -3, 10, 1 << 40])
    params = fx.SearchParameters(sel=fx.IDSelectorRange(0, 11))
    assert idx.search("x", 3, params=params, D="d", I="i") == ("D", "I")
    assert idx.range_search("x", 0.5) == ("lims", "D", "I")
    assert flat.calls[1:] == [("search", 3, params, "d", "i"), ("range_search", 0.5, None)]
    assert idx.remove_ids([10]) == 3 and flat._resets == 1
    idx.reset()
    assert flat._resets == 2 and idx.ntotal == 0 and idx.id_map.size == 0


def test_reconstruct_takes_the_last_row_of_a_label():
    flat = _FakeFlat()
    idx = fx.IndexIDMap2(flat)
    idx.add_with_ids(np.zeros((4, 8), dtype=np.float32), [10, -3, 10, 1 << 40])
    assert idx.reconstruct(10).tolist() == [2.0] * 8  # rows 0 and 2 carry 10: the last one
    assert idx.reconstruct(-3).tolist() == [1.0] * 8
    assert ("rows_of_ids", [10]) in flat.calls and ("reconstruct_n", 2, 1) in flat.calls
    with pytest.raises(RuntimeError, match="not found"):
        idx.reconstruct(11)
    assert not hasattr(fx.IndexIDMap(_FakeFlat()), "reconstruct")


# ---- the thin bindings over a recording stand-in for the C library ------------
class _RecLib:
    def __init__(self, d=4, ntotal=0, has_ids=0):
        self.d, self.ntotal, self.has_ids, self.calls = d, ntotal, has_ids, []

    def fx_index_dim(self, h, out):
        out._obj.value = self.d
        return 0

    def fx_index_ntotal(self, h, out):
        out._obj.value = self.ntotal
        return 0

    def fx_index_set_stream(self, h, s):
        return 0

    def fx_index_has_ids(self, h, out):
        out._obj.value = self.has_ids
        return 0

    def fx_index_add_with_ids(self, h, n, x, x_dtype, x_mem, ids, ids_mem):
        got = np.ctypeslib.as_array(ctypes.cast(ids, ctypes.POINTER(ctypes.c_int64)), shape=(n,)).tolist()
        self.calls.append(("add_with_ids", n, x_dtype, x_mem, got, ids_mem))
        self.ntotal += n
        return 0

    def fx_index_get_ids(self, h, i0, n, out, out_mem):
        self.calls.append(("get_ids", i0, n, out_mem))
        np.ctypeslib.as_array(ctypes.cast(out, ctypes.POINTER(ctypes.c_int64)), shape=(n,))[:] = np.arange(i0, i0 + n) * 2
        return 0

    def fx_index_rows_of_ids(self, h, ids, n, ids_mem, rows, rows_mem):
        got = np.ctypeslib.as_array(ctypes.cast(ids, ctypes.POINTER(ctypes.c_int64)), shape=(n,))
        self.calls.append(("rows_of_ids", got.tolist(), ids_mem, rows_mem))
        np.ctypeslib.as_array(ctypes.cast(rows, ctypes.POINTER(ctypes.c_int64)), shape=(n,))[:] = got // 2
        return 0

    def fx_index_write(self, h, path):
        self.calls.append(("write", h.value, path))
        return 0

    def fx_index_free(self, h):
        pass


def _stand_in(**kw):
    ix = fx.IndexFlatL2.__new__(fx.IndexFlatL2)
    ix._lib = _RecLib(**kw)
    ix._h = ctypes.c_void_p(1)
    ix.device = 0
    return ix


def test_flat_add_with_ids_binds_rows_and_int64_ids():
    ix = _stand_in()
    ix.add_with_ids(np.ones((3, 4)), np.array([7, -2, 1 << 41], dtype=np.int64))
    ix.add_with_ids(np.ones((2, 4), dtype=np.float32), [5, 5])  # a list; duplicates are legal
    assert ix._lib.calls == [("add_with_ids", 3, _lib.F32, _lib.MEM_HOST, [7, -2, 1 << 41], _lib.MEM_HOST),
                             ("add_with_ids", 2, _lib.F32, _lib.MEM_HOST, [5, 5], _lib.MEM_HOST)]
    with pytest.raises(AssertionError, match="ids for"):
        ix.add_with_ids(np.ones((3, 4)), [1, 2])
    with pytest.raises(AssertionError, match="dimension"):
        ix.add_with_ids(np.ones((2, 5)), [1, 2])
    assert len(ix._lib.calls) == 2


def test_flat_get_ids_and_rows_of_ids():
    ix = _stand_in(ntotal=6, has_ids=1)
    assert ix.has_ids is True
    assert ix.get_ids().tolist() == [0, 2, 4, 6, 8, 10]
    assert ix.get_ids(2, 3).tolist() == [4, 6, 8]
    assert ix.rows_of_ids([8, 8, 2]).tolist() == [4, 4, 1]
    assert ix._lib.calls == [("get_ids", 0, 6, _lib.MEM_HOST), ("get_ids", 2, 3, _lib.MEM_HOST),
                             ("rows_of_ids", [8, 8, 2], _lib.MEM_HOST, _lib.MEM_HOST)]


def test_wrapper_over_the_bindings_and_write_index():
    ix = _stand_in()
    idx = fx.IndexIDMap2(ix)
    idx.add_with_ids(np.ones((2, 4)), [9, 8])
    assert idx.ntotal == 2 and idx.id_map.tolist() == [0, 2]
    fx.write_index(idx, "/x/labelled.index")  # the wrapper writes its flat index's handle
    fx.write_index(ix, "/x/flat.index")
    assert ix._lib.calls[-2:] == [("write", 1, b"/x/labelled.index"), ("write", 1, b"/x/flat.index")]


def test_read_index_wraps_a_labelled_file(monkeypatch):
    class _ReadLib(_RecLib):
        def fx_index_read(self, path, dtype, device, out):
            out._obj.value = 0x55
            return 0

    for has, kind in ((1, fx.IndexIDMap2), (0, fx.IndexFlatL2)):
        so = _ReadLib(ntotal=3, has_ids=has)
        monkeypatch.setattr(fx, "lib", so)
        monkeypatch.setattr(fx._FlatIndex, "_lib", so)
        back = fx.read_index("/x/any.index")
        assert type(back) is kind and back.ntotal == 3
        flat = back.index if has else back
        assert isinstance(flat, fx.IndexFlatL2) and flat._h.value == 0x55
        flat._h = ctypes.c_void_p()  # (nothing to free)

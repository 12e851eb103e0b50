"""CPU checks of the Python side of the read-back calls: ``_FlatIndex``'s
bindings over a recording stand-in for the C library (as
tests/test_select_logic.py fakes it), ``IndexIDMap`` / ``IndexIDMap2`` over a
recording stand-in index, and the MMR re-ranking of retrieval.py against a
numpy restatement written here.  The kernels are checked in
test_reconstruct_gpu.py."""
import ctypes

import numpy as np
import pytest

from rag_faiss_embedding_amd import _lib
from rag_faiss_embedding_amd import faiss as fx
from rag_faiss_embedding_amd import retrieval


def _addr(p):
    return p.value if isinstance(p, ctypes.c_void_p) else p


# ---- the thin bindings over a recording stand-in for the C library ------------
class _RecLib:
    def __init__(self, d=4, ntotal=10):
        self.d, self.ntotal, self.calls = d, ntotal, []

    def fx_index_dim(self, h, out):
        out._obj.value = self.d
        return 0

    def fx_index_ntotal(self, h, out):
        out._obj.value = self.ntotal
        return 0

    def fx_index_set_stream(self, h, s):
        return 0

    def fx_index_free(self, h):
        pass

    def fx_selector_create(self, h, kind, data, n, mem, invert, out):
        out._obj.value = 0x2000
        return 0

    def fx_selector_free(self, h):
        pass

    def fx_index_reconstruct_batch(self, h, n, keys, keys_mem, out, out_dtype, out_mem):
        got = np.ctypeslib.as_array(ctypes.cast(keys, ctypes.POINTER(ctypes.c_int64)), shape=(n,))
        self.calls.append(("reconstruct_batch", n, got.tolist(), keys_mem, out_dtype, out_mem))
        o = np.ctypeslib.as_array(ctypes.cast(out, ctypes.POINTER(ctypes.c_float)), shape=(n, self.d))
        o[:] = got[:, None].astype(np.float32) + np.arange(self.d, dtype=np.float32) / 8
        return 0

    def fx_index_search_and_reconstruct(self, h, sel, nq, q, q_dtype, q_mem, k, D, I, R, r_dtype, out_mem):
        qv = np.ctypeslib.as_array(ctypes.cast(q, ctypes.POINTER(ctypes.c_float)), shape=(nq, self.d))
        self.calls.append(("search_and_reconstruct", _addr(sel), nq, qv.copy(), q_dtype, q_mem, k, r_dtype, out_mem))
        np.ctypeslib.as_array(ctypes.cast(D, ctypes.POINTER(ctypes.c_float)), shape=(nq, k))[:] = np.arange(k)
        np.ctypeslib.as_array(ctypes.cast(I, ctypes.POINTER(ctypes.c_int64)), shape=(nq, k))[:] = np.arange(k) + 100
        np.ctypeslib.as_array(ctypes.cast(R, ctypes.POINTER(ctypes.c_float)), shape=(nq, k, self.d))[:] = 0.5
        return 0

    def fx_index_compute_distance_subset(self, h, nq, q, q_dtype, q_mem, k, keys, keys_mem, D, out_mem):
        got = np.ctypeslib.as_array(ctypes.cast(keys, ctypes.POINTER(ctypes.c_int64)), shape=(nq, k))
        self.calls.append(("compute_distance_subset", nq, q_dtype, q_mem, k, got.tolist(), keys_mem, out_mem))
        np.ctypeslib.as_array(ctypes.cast(D, ctypes.POINTER(ctypes.c_float)), shape=(nq, k))[:] = got * 2.0
        return 0


def _stand_in(**kw):
    ix = fx.IndexFlatL2.__new__(fx.IndexFlatL2)
    ix._lib = _RecLib(**kw)
    ix._h = ctypes.c_void_p(1)
    ix.device = 0
    ix.storage_dtype = "float32"
    return ix


def test_reconstruct_batch_passes_host_keys_and_fp32_out():
    ix = _stand_in()
    out = ix.reconstruct_batch([3, 0, 3, 9])
    assert out.dtype == np.float32 and out.shape == (4, 4)
    assert out[:, 0].tolist() == [3.0, 0.0, 3.0, 9.0] and out[0].tolist() == [3.0, 3.125, 3.25, 3.375]
    assert ix.reconstruct(7).tolist() == [7.0, 7.125, 7.25, 7.375]
    assert ix.reconstruct_batch(np.array([5], dtype=np.int32), dtype="storage").dtype == np.float32
    assert ix._lib.calls == [
        ("reconstruct_batch", 4, [3, 0, 3, 9], _lib.MEM_HOST, _lib.F32, _lib.MEM_HOST),
        ("reconstruct_batch", 1, [7], _lib.MEM_HOST, _lib.F32, _lib.MEM_HOST),
        ("reconstruct_batch", 1, [5], _lib.MEM_HOST, _lib.F32, _lib.MEM_HOST)]
    assert ix.reconstruct_batch([]).shape == (0, 4)
    with pytest.raises(ValueError):
        ix.reconstruct_batch([1], dtype="float16")


def test_storage_dtype_of_a_16_bit_index():
    ix = _stand_in()
    ix.storage_dtype = "float16"
    assert ix._out_dtype("storage", False) == (_lib.F16, np.dtype("float16"))
    assert ix._out_dtype(None, False) == (_lib.F32, np.dtype("float32"))
    ix.storage_dtype = "bfloat16"
    with pytest.raises(TypeError, match="bfloat16"):
        ix.reconstruct_batch([1], dtype="storage")  # numpy has none: device keys only
    assert ix._lib.calls == []


def test_search_and_reconstruct_binds_queries_results_and_selector():
    ix = _stand_in()
    xq = np.arange(8, dtype=np.float64).reshape(2, 4)  # converted to fp32, as search does
    D, I, R = ix.search_and_reconstruct(xq, 3)
    assert (D.shape, I.shape, R.shape) == ((2, 3), (2, 3), (2, 3, 4))
    assert (D.dtype, I.dtype, R.dtype) == (np.float32, np.int64, np.float32)
    assert D[1].tolist() == [0, 1, 2] and I[0].tolist() == [100, 101, 102] and (R == 0.5).all()
    D, I, R = ix.search_and_reconstruct(xq, 2, params=fx.SearchParameters(sel=fx.IDSelectorRange(1, 5)))
    a, b = ix._lib.calls
    assert a[0] == "search_and_reconstruct" and a[1] is None and a[2] == 2 and a[4:] == (_lib.F32, _lib.MEM_HOST, 3,
                                                                                      _lib.F32, _lib.MEM_HOST)
    np.testing.assert_array_equal(a[3], xq.astype(np.float32))
    assert b[1] == 0x2000 and b[6] == 2
    with pytest.raises(AssertionError, match="positive"):
        ix.search_and_reconstruct(xq, 0)
    with pytest.raises(AssertionError, match="dimension"):
        ix.search_and_reconstruct(np.zeros((2, 5)), 3)
    assert len(ix._lib.calls) == 2


def test_compute_distance_subset_binds_the_label_matrix():
    ix = _stand_in()
    xq = np.zeros((2, 4), dtype=np.float32)
    D = ix.compute_distance_subset(xq, [[4, -1, 7], [0, 0, 1 << 40]])
    assert D.dtype == np.float32 and D.tolist() == [[8.0, -2.0, 14.0], [0.0, 0.0, float(2 << 40)]]
    assert ix._lib.calls == [("compute_distance_subset", 2, _lib.F32, _lib.MEM_HOST, 3, [[4, -1, 7], [0, 0, 1 << 40]],
                              _lib.MEM_HOST, _lib.MEM_HOST)]
    with pytest.raises(AssertionError, match="nq, k"):
        ix.compute_distance_subset(xq, [[1, 2, 3]])
    assert ix.compute_distance_subset(xq, np.zeros((2, 0), dtype=np.int64)).shape == (2, 0)
    assert len(ix._lib.calls) == 1


# ---- the wrappers over a recording stand-in index ------------------------------
class _FakeFlat:
    d, metric_type, is_trained, ntotal = 4, fx.METRIC_L2, True, 0

    def __init__(self, known=()):
        self.known, self.calls = set(known), []

    def reconstruct_batch(self, keys, dtype=None):
        keys = np.asarray(keys, dtype=np.int64)
        self.calls.append(("reconstruct_batch", keys.tolist(), dtype))
        out = np.full((keys.size, self.d), np.nan, dtype=np.float32)  # the library's row for an unknown label
        for i, key in enumerate(keys.tolist()):
            if key in self.known:
                out[i] = key
        return out

    def search_and_reconstruct(self, x, k, *, params=None, dtype=None):
        self.calls.append(("search_and_reconstruct", k, params, dtype))
        return "D", "I", "R"

    def compute_distance_subset(self, x, labels):
        self.calls.append(("compute_distance_subset", labels))
        return "D"


def test_idmap_forwards_the_new_calls():
    flat = _FakeFlat(known=[5])
    idx = fx.IndexIDMap(flat)
    params = fx.SearchParameters(sel=fx.IDSelectorRange(0, 9))
    assert idx.search_and_reconstruct("x", 4, params=params) == ("D", "I", "R")
    assert idx.compute_distance_subset("x", "L") == "D"
    assert flat.calls == [("search_and_reconstruct", 4, params, None), ("compute_distance_subset", "L")]
    assert not hasattr(idx, "reconstruct_batch")  # IndexIDMap2's, as reconstruct


def test_idmap2_reconstruct_is_one_batch_call_and_raises_on_a_nan_row():
    flat = _FakeFlat(known=[5, -3])
    idx = fx.IndexIDMap2(flat)
    assert idx.reconstruct(5).tolist() == [5.0] * 4
    assert idx.reconstruct(-3).tolist() == [-3.0] * 4
    assert flat.calls == [("reconstruct_batch", [5], None), ("reconstruct_batch", [-3], None)]
    with pytest.raises(RuntimeError, match="key 11 not found"):
        idx.reconstruct(11)  # an all-NaN row: the library's answer for an unknown label
    got = idx.reconstruct_batch([5, 11, -3], dtype="storage")
    assert np.isnan(got[1]).all() and got[0, 0] == 5 and got[2, 0] == -3  # the batch form does not raise
    assert flat.calls[-1] == ("reconstruct_batch", [5, 11, -3], "storage")


# ---- MMR re-ranking -------------------------------------------------------------
def mmr_restated(sim_q, vecs, k, lam, l2):
    """The rule, restated: start from rank 0; then always the unpicked candidate
    with the largest lam s(q, c) - (1 - lam) max_p s(c, p), the earlier rank on
    a tie."""
    n = len(sim_q)
    vecs = vecs.astype(np.float64)
    s = -((vecs[:, None, :] - vecs[None, :, :]) ** 2).sum(2) if l2 else vecs @ vecs.T
    picked = [0] if n else []
    while len(picked) < min(k, n):
        best, best_v = -1, -np.inf
        for c in range(n):
            if c in picked:
                continue
            v = lam * float(sim_q[c]) - (1 - lam) * max(s[c, p] for p in picked)
            if v > best_v:
                best, best_v = c, v
        picked.append(best)
    return picked


@pytest.mark.parametrize("l2", [True, False])
@pytest.mark.parametrize("lam", [0.0, 0.3, 0.7, 1.0])
def test_mmr_pick_equals_the_restatement(lam, l2):
    rng = np.random.default_rng(5)
    # integer vectors: every similarity is exact, so both forms see the same ties
    vecs = rng.integers(-3, 4, size=(12, 6)).astype(np.float32)
    q = rng.integers(-3, 4, size=6).astype(np.float32)
    sim = -((vecs - q) ** 2).sum(1) if l2 else vecs @ q
    order = np.argsort(-sim, kind="stable")  # candidates come ranked
    vecs, sim = vecs[order], sim[order]
    for k in (1, 5, 12, 20):
        assert retrieval.mmr_pick(sim, vecs, k, lam, l2) == mmr_restated(sim, vecs, k, lam, l2)
    if lam == 1.0:
        assert retrieval.mmr_pick(sim, vecs, 12, lam, l2) == list(range(12))  # the plain ranking
    assert retrieval.mmr_pick(sim[:0], vecs[:0], 3, lam, l2) == []


def test_lambda_zero_never_takes_a_twin_before_a_third():
    a = np.array([1.0, 0.0, 0.0], dtype=np.float32)
    vecs = np.stack([a, a, np.array([0.9, 0.1, 0.0], dtype=np.float32), np.array([0.0, 1.0, 0.0], dtype=np.float32)])
    q = a
    for l2 in (True, False):
        sim = -((vecs - q) ** 2).sum(1) if l2 else vecs @ q
        assert (np.diff(sim) <= 0).all()  # ranked; rank 1 is rank 0's twin
        picks = retrieval.mmr_pick(sim, vecs, 3, 0.0, l2)
        assert picks[0] == 0 and 1 not in picks, picks
        assert retrieval.mmr_pick(sim, vecs, 4, 0.0, l2)[-1] == 1  # ... taken only when nothing else is left
        assert retrieval.mmr_pick(sim, vecs, 4, 1.0, l2) == [0, 1, 2, 3]


class _Index:
    """search / search_and_reconstruct over a small numpy corpus, recorded."""
    metric_type = 1

    def __init__(self, xb):
        self.xb, self.calls = xb, []

    def _rank(self, xq, k):
        D = ((xq[:, None, :] - self.xb[None, :, :]) ** 2).sum(2).astype(np.float32)
        I = np.argsort(D, axis=1, kind="stable")[:, :k]
        Dk = np.take_along_axis(D, I, 1)
        pad = k - I.shape[1]
        if pad > 0:
            I = np.pad(I, ((0, 0), (0, pad)), constant_values=-1)
            Dk = np.pad(Dk, ((0, 0), (0, pad)), constant_values=np.finfo(np.float32).max)
        return Dk, I.astype(np.int64)

    def search(self, xq, k, **kw):
        self.calls.append(("search", k, kw))
        return self._rank(xq, k)

    def search_and_reconstruct(self, xq, k, *, params=None):
        self.calls.append(("search_and_reconstruct", k, params))
        D, I = self._rank(xq, k)
        R = np.where((I >= 0)[:, :, None], self.xb[np.maximum(I, 0)], np.nan).astype(np.float32)
        return D, I, R


class _Store:
    def fetch_many(self, ids):
        return {int(i): {"id": int(i)} for i in ids}


def test_diversity_goes_through_search_and_reconstruct_and_none_does_not():
    rng = np.random.default_rng(9)
    xb = rng.integers(-4, 5, size=(9, 5)).astype(np.float32)
    xb[1] = xb[0]  # a near-duplicate pair
    xq = (xb[[0, 4]] + 0.25).astype(np.float32)
    doc_ids = list(range(100, 109))
    ix = _Index(xb)
    plain = retrieval.search_similar_documents(ix, doc_ids, _Store(), xq, k=3)
    assert [c[0] for c in ix.calls] == ["search"] and ix.calls[0][1:] == (3, {})
    # lambda = 1 is the plain ranking; the default fetch is 4k (here past ntotal: padded slots are skipped)
    one = retrieval.search_similar_documents(ix, doc_ids, _Store(), xq, k=3, diversity=1.0)
    assert ix.calls[-1] == ("search_and_reconstruct", 12, None) and one == plain
    div = retrieval.search_similar_documents(ix, doc_ids, _Store(), xq, k=3, diversity=0.0, fetch_k=6)
    assert ix.calls[-1] == ("search_and_reconstruct", 6, None)
    D, I = ix._rank(xq, 6)
    for qi in range(2):
        picks = mmr_restated(-D[qi].astype(np.float64), xb[I[qi]], 3, 0.0, True)
        assert [d["id"] for d in div[qi]] == [doc_ids[I[qi][p]] for p in picks]
        assert [d["distance"] for d in div[qi]] == [float(D[qi][p]) for p in picks]
    assert {100, 101} - {d["id"] for d in div[0]}  # the twins are not both taken
    with pytest.raises(ValueError):
        retrieval._diverse_search(ix, xq, 3, None, 1.5, None)

    class _Vec:
        def generate_embeddings(self, texts):
            return xq[:len(texts)]

    eng = retrieval.RetrievalEngine(_Vec(), ix, doc_ids, _Store())
    n = len(ix.calls)
    assert eng.search(["a", "b"], k=3) == plain and ix.calls[n][0] == "search"
    assert eng.search(["a", "b"], k=3, diversity=0.0, fetch_k=6) == div
    assert ix.calls[-1] == ("search_and_reconstruct", 6, None)

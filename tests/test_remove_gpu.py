"""GPU checks of ``index.remove_ids`` (fx_remove.hip through the C ABI and the
Python surface): the in-place compaction of the flat index.

Conventions are tests/test_select_gpu.py's: the same values re-cut to (n, d)
rows and (nq, d) queries, n = 3100 (25 tiles, 28 rows in the last) and n = 300,
nq = 130; float32 d = 384, bfloat16 d = 768, float16 d = 64, bfloat16 d = 320;
L2 and IP.

With Y = reconstruct_n(0, n) taken before the removal and ``keep`` the boolean
complement of the removed set, every case checks (``check_removed``):

1. the return value == (~keep).sum() and ntotal == keep.sum();
2. reconstruct_n(0, ntotal) is byte-equal to Y[keep];
3. search(xq, 10): ids equal the CPU oracle on Y[keep] (oracle.cpu.knn_exact
   for L2, oracle.flat_l2.knn_inner_product for IP), distances within
   assert_parity's 1e-5 max(1, |D|);
4. search(xq, 10) is identical to a fresh index built by add(Y[keep]): ids
   equal and D.tobytes() equal (the returned distance is the exact fp64
   recomputation over the stored row; the scan image cannot enter).
"""
import ctypes
import json
import shutil

import numpy as np
import pytest

from oracle import cpu as C
from oracle import flat_l2 as F
from tests._data import gaussian_small
from tests.test_gpu_parity import assert_parity

pytestmark = pytest.mark.gpu

WIDTHS = [("float32", 384), ("bfloat16", 768), ("float16", 64), ("bfloat16", 320)]
NMAX, NSMALL, QMAX = 3100, 300, 130
FLT_MAX = F.FLT_MAX
CASES = [(m, dt, d) for m in ("L2", "IP") for dt, d in WIDTHS]
CASE_IDS = ["-".join(map(str, p)) for p in CASES]


@pytest.fixture(scope="module")
def fx():
    from rag_faiss_embedding_amd import _lib, faiss
    if _lib.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    return faiss


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def values():
    xb, xq = gaussian_small()
    v = np.concatenate([xb.ravel(), xq.ravel()])
    v = np.concatenate([v, -v[::-1]])
    assert v.size >= (NMAX + QMAX) * 768
    v.setflags(write=False)
    return v


def _cut(values, d, n):
    xb = values[:NMAX * d].reshape(NMAX, d)[:n]
    xq = values[NMAX * d:(NMAX + QMAX) * d].reshape(QMAX, d)
    return xb, xq


def row_bytes(dtype, d):
    return (d * (4 if dtype == "float32" else 2) + 127) // 128 * 128


def _cls(fx_mod, metric):
    return fx_mod.IndexFlatL2 if metric == "L2" else fx_mod.IndexFlatIP


def _build(fx_mod, values, metric, dtype, d, n):
    """(index of the n rows, its stored rows as fp32, the queries)."""
    xb, xq = _cut(values, d, n)
    ix = _cls(fx_mod, metric)(d, dtype=dtype)
    ix.add(xb)
    Y = ix.reconstruct_n(0, n)
    Y.setflags(write=False)
    return ix, Y, xq


def oracle(metric, xq, rows, k):
    """(D, I) of the k nearest of `rows`, padded as faiss pads past len(rows)."""
    nq = len(xq)
    D = np.full((nq, k), FLT_MAX if metric == "L2" else -FLT_MAX, dtype=np.float32)
    I = np.full((nq, k), -1, dtype=np.int64)
    kk = min(k, len(rows))
    if kk:
        knn = C.knn_exact if metric == "L2" else F.knn_inner_product
        D[:, :kk], I[:, :kk] = knn(xq, np.ascontiguousarray(rows), kk)
    return D, I


def check_removed(fx_mod, metric, dtype, ix, Y, keep, xq, n_removed):
    """Checks 1-4 of the module docstring on an index that held Y and had ~keep removed."""
    assert n_removed == int((~keep).sum())
    assert ix.ntotal == int(keep.sum())
    kept = np.ascontiguousarray(Y[keep])
    assert ix.reconstruct_n(0, ix.ntotal).tobytes() == kept.tobytes()
    D, I = ix.search(xq, 10)
    assert_parity(D, I, *oracle(metric, xq, kept, 10))
    fresh = _cls(fx_mod, metric)(Y.shape[1], dtype=dtype)
    if len(kept):
        fresh.add(kept)
    Df, If = fresh.search(xq, 10)
    np.testing.assert_array_equal(I, If)
    assert D.tobytes() == Df.tobytes()


# --------------------------------------------------------------------------
# removal patterns, as boolean "removed" masks over the n rows, and what
# remove_ids is called with
# --------------------------------------------------------------------------
def third(n):
    m = np.zeros(n, dtype=bool)
    m[::3] = True
    return m


def block(n, lo, hi):
    m = np.zeros(n, dtype=bool)
    m[lo:hi] = True
    return m


PATTERNS = {
    "block": lambda fx_mod, n: (block(n, 900, 2000), fx_mod.IDSelectorRange(900, 2000)),      # not tile-aligned
    "last": lambda fx_mod, n: (block(n, n - 1, n), [n - 1]),                                   # nothing moves
    "last28": lambda fx_mod, n: (block(n, n - 28, n), np.arange(n - 28, n)),                   # the partial tile goes
    "keep100": lambda fx_mod, n: (~block(n, 1000, 1100), fx_mod.IDSelectorNot(fx_mod.IDSelectorRange(1000, 1100))),
}
MOVING = {
    "third": lambda fx_mod, n: (third(n), fx_mod.IDSelectorBatch(np.arange(0, n, 3))),         # every tile shifts
    "row0": lambda fx_mod, n: (block(n, 0, 1), np.array([0])),                                 # everything moves by one
}


@pytest.mark.parametrize("pattern", sorted(PATTERNS))
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_patterns(fx, values, case, pattern):
    metric, dtype, d = case
    ix, Y, xq = _build(fx, values, metric, dtype, d, NMAX)
    gone, arg = PATTERNS[pattern](fx, NMAX)
    check_removed(fx, metric, dtype, ix, Y, ~gone, xq, ix.remove_ids(arg))


@pytest.mark.parametrize("stage", ["default", "128rows", "1row"])
@pytest.mark.parametrize("pattern", sorted(MOVING))
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_moving_patterns_in_three_staging_sizes(fx, values, case, pattern, stage):
    """Every third row and row 0 with the default staging buffer (one staged
    chunk), with 128 rows of staging (many chunks, staged and direct) and, on
    n = 300, with one row (one row per chunk): the same bytes every time."""
    metric, dtype, d = case
    n = NSMALL if stage == "1row" else NMAX
    ix, Y, xq = _build(fx, values, metric, dtype, d, n)
    if stage != "default":
        ix.set_option("remove_stage", (128 if stage == "128rows" else 1) * row_bytes(dtype, d))
    gone, arg = MOVING[pattern](fx, n)
    check_removed(fx, metric, dtype, ix, Y, ~gone, xq, ix.remove_ids(arg))
    # the plan took the path the setting is there to force
    st = ix.last_remove_stats()
    above = n - int(gone.sum())  # kept rows above the first removed one (row 0 in both patterns)
    assert st["first"] == 0 and st["direct_rows"] + st["staged_rows"] == above
    if stage == "default":
        assert st["chunks"] == 1 and st["direct_rows"] == 0
    elif stage == "128rows":
        assert st["chunks"] > 5 and st["staged_rows"] > 0 and (pattern == "row0") == (st["direct_rows"] == 0)
    else:
        assert st["chunks"] >= 100 if pattern == "row0" else st["chunks"] > 5


@pytest.mark.parametrize("metric,dtype,d,row_b", [("L2", "float16", 64, 128), ("IP", "bfloat16", 128, 256)])
def test_many_chunks_at_1024_row_boundaries(fx, values, metric, dtype, d, row_b):
    """The plan of a production-sized removal in small: 24,000 rows with a
    staging buffer of 2048 rows, so chunks are cut at 1024-row boundaries from
    the device's coarse prefix (not at single rows, as the 128-row and one-row
    settings above cut them).  One row in ten scattered plus a block: the
    small shift below the block gives staged chunks, the large one above it
    direct chunks."""
    n = 24_000
    assert values.size >= (n + QMAX) * d
    xb = values[:n * d].reshape(n, d)
    xq = values[-QMAX * d:].reshape(QMAX, d)
    ix = _cls(fx, metric)(d, dtype=dtype)
    ix.add(xb)
    Y = ix.reconstruct_n(0, n)
    ix.set_option("remove_stage", 2048 * row_b)
    gone = np.zeros(n, dtype=bool)
    gone[np.random.default_rng(5).permutation(n)[:n // 10]] = True
    gone[9000:12500] = True
    first = int(np.flatnonzero(gone)[0])
    check_removed(fx, metric, dtype, ix, Y, ~gone, xq, ix.remove_ids(np.flatnonzero(gone)))
    st = ix.last_remove_stats()
    assert st["first"] == first
    assert st["direct_rows"] + st["staged_rows"] == int((~gone)[first:].sum())
    assert st["staged_rows"] >= 2048 and st["direct_rows"] >= 2048 and st["chunks"] >= 6


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_all_rows(fx, values, case):
    """Everything removed: an empty index that pads and takes rows again."""
    metric, dtype, d = case
    ix, Y, xq = _build(fx, values, metric, dtype, d, NMAX)
    assert ix.remove_ids(fx.IDSelectorRange(0, NMAX)) == NMAX
    assert ix.ntotal == 0
    D, I = ix.search(xq, 10)
    assert (I == -1).all() and (D == (FLT_MAX if metric == "L2" else -FLT_MAX)).all()
    ix.add(Y[:200])
    assert ix.reconstruct_n(0, 200).tobytes() == Y[:200].tobytes()
    D, I = ix.search(xq, 10)
    assert_parity(D, I, *oracle(metric, xq, Y[:200], 10))


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_no_rows(fx, values, case):
    """Ids outside the index: 0 removed, nothing changes, and a C selector
    created before the call still searches."""
    from rag_faiss_embedding_amd import _lib
    metric, dtype, d = case
    ix, Y, xq = _build(fx, values, metric, dtype, d, NMAX)
    want = ix.search(xq, 10)
    h = ctypes.c_void_p()
    rng = np.array([0, 10], dtype=np.int64)
    assert _lib.lib.fx_selector_create(ix._h, 2, rng.ctypes.data_as(ctypes.c_void_p), 2, 0, 0, ctypes.byref(h)) == 0
    assert ix.remove_ids([NMAX, NMAX + 7, 10 ** 9, -5]) == 0
    assert ix.remove_ids(fx.IDSelectorRange(NMAX, NMAX + 100)) == 0
    assert ix.ntotal == NMAX and ix.reconstruct_n(0, NMAX).tobytes() == Y.tobytes()
    D, I = ix.search(xq, 10)
    np.testing.assert_array_equal(I, want[1])
    assert D.tobytes() == want[0].tobytes()
    Dh, Ih = np.empty((1, 5), dtype=np.float32), np.empty((1, 5), dtype=np.int64)
    args = (1, xq.ctypes.data, _lib.F32, _lib.MEM_HOST, 5, Dh.ctypes.data, Ih.ctypes.data, _lib.MEM_HOST)
    assert _lib.lib.fx_index_search_sel(ix._h, h, *args) == 0 and set(Ih[0]) <= set(range(10))
    _lib.lib.fx_selector_free(h)


def test_remove_stage_option_range(fx, values):
    ix, _, _ = _build(fx, values, "L2", "float32", 384, NSMALL)
    for bad in (-1, 1, 1535, (1 << 32) + 1):
        with pytest.raises(RuntimeError):
            ix.set_option("remove_stage", bad)
    for good in (0, 1536, 1 << 32):
        ix.set_option("remove_stage", good)


@pytest.mark.parametrize("case", [CASES[0], CASES[1], CASES[6]], ids=[CASE_IDS[0], CASE_IDS[1], CASE_IDS[6]])
def test_repeated_removal_and_file_round_trip(fx, values, case, tmp_path):
    """Remove, add the removed rows back, remove a different set; the oracle
    after each step; then write_index / read_index."""
    metric, dtype, d = case
    ix, Y, xq = _build(fx, values, metric, dtype, d, NMAX)
    gone = third(NMAX)
    check_removed(fx, metric, dtype, ix, Y, ~gone, xq, ix.remove_ids(np.flatnonzero(gone)))
    ix.add(Y[gone])
    Y2 = np.concatenate([Y[~gone], Y[gone]])
    assert ix.ntotal == NMAX and ix.reconstruct_n(0, NMAX).tobytes() == Y2.tobytes()
    D, I = ix.search(xq, 10)
    assert_parity(D, I, *oracle(metric, xq, Y2, 10))
    gone2 = block(NMAX, 5, 1500) | block(NMAX, 2900, 3000)
    check_removed(fx, metric, dtype, ix, Y2, ~gone2, xq, ix.remove_ids(np.flatnonzero(gone2)))
    if metric == "L2":  # (the IxF2 file is an L2 index: read_index)
        path = tmp_path / "ix.bin"
        fx.write_index(ix, str(path))
        back = fx.read_index(str(path), dtype=dtype)
        assert back.ntotal == ix.ntotal
        assert back.reconstruct_n(0, back.ntotal).tobytes() == np.ascontiguousarray(Y2[~gone2]).tobytes()
        Db, Ib = back.search(xq, 10)
        np.testing.assert_array_equal(Ib, ix.search(xq, 10)[1])


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_range_search_after_removal(fx, values, case):
    """range_search (the plain MFMA filter over the stored rows) after a
    removal, preceded by a top-k search so that an image exists and is rebuilt:
    membership equals the oracle's on Y[keep] at a radius from its 10th distance."""
    metric, dtype, d = case
    ix, Y, xq = _build(fx, values, metric, dtype, d, NMAX)
    ix.search(xq, 10)
    gone = third(NMAX) | block(NMAX, 100, 300)
    assert ix.remove_ids(np.flatnonzero(gone)) == int(gone.sum())
    kept = np.ascontiguousarray(Y[~gone])
    Dk, _ = oracle(metric, xq, kept, 10)
    y64 = kept.astype(np.float64)
    if metric == "L2":  # difference form: no cancellation
        K = np.stack([((q.astype(np.float64) - y64) ** 2).sum(1) for q in xq])
    else:
        K = xq.astype(np.float64) @ y64.T
    # the radius: from the oracle's 10th distances (their median), moved to the middle of the widest gap
    # among the 100 keys around it, so that membership does not hang on the last bit of a distance
    s = np.sort(K.ravel())
    at = int(np.searchsorted(s, float(np.median(Dk[:, 9]))))
    w = s[max(0, at - 50):at + 50]
    g = int(np.argmax(np.diff(w)))
    radius = np.float32(0.5 * (w[g] + w[g + 1]))
    assert w[g + 1] - w[g] >= 1e-5 * abs(float(radius)) and w[g] < float(radius) < w[g + 1]
    member = K < float(radius) if metric == "L2" else K > float(radius)
    lims, D, I = ix.range_search(xq, float(radius))
    np.testing.assert_array_equal(lims, np.concatenate([[0], np.cumsum(member.sum(1))]).astype(np.uint64))
    qi, ri = np.nonzero(member)
    np.testing.assert_array_equal(I, ri)
    assert (np.abs(D.astype(np.float64) - K[qi, ri]) <= 1e-5 * np.maximum(1.0, np.abs(K[qi, ri]))).all()
    assert member.sum() > 0


def test_filtered_search_after_removal(fx, values):
    """A Python IDSelectorRange used before the removal is rebuilt and selects
    by the new ids."""
    ix, Y, xq = _build(fx, values, "L2", "bfloat16", 768, NMAX)
    p = fx.SearchParameters(sel=fx.IDSelectorRange(500, 700))
    D, I = ix.search(xq, 10, params=p)
    assert ((I >= 500) & (I < 700)).all()
    assert ix.remove_ids(fx.IDSelectorRange(0, 400)) == 400
    kept = Y[400:]
    D, I = ix.search(xq, 10, params=p)
    Dr, Ir = oracle("L2", xq, kept[500:700], 10)
    assert_parity(D, I, Dr, Ir + 500)
    # also after an add restores the old ntotal
    ix.add(Y[:400])
    Y2 = np.concatenate([kept, Y[:400]])
    D, I = ix.search(xq, 10, params=p)
    Dr, Ir = oracle("L2", xq, Y2[500:700], 10)
    assert_parity(D, I, Dr, Ir + 500)


def test_stale_c_handles(fx, values):
    """C selectors from before a removal are stale, the one passed in included,
    also once an add restores the old ntotal."""
    from rag_faiss_embedding_amd import _lib
    d = 64
    ix, Y, xq = _build(fx, values, "L2", "float16", d, NMAX)
    lib = _lib.lib

    def make(lo, hi):
        h = ctypes.c_void_p()
        rng = np.array([lo, hi], dtype=np.int64)
        assert lib.fx_selector_create(ix._h, 2, rng.ctypes.data_as(ctypes.c_void_p), 2, 0, 0, ctypes.byref(h)) == 0
        return h

    before, used = make(0, 10), make(100, 150)
    other = fx.IndexFlatL2(d, dtype="float16")
    other.add(Y)
    n = ctypes.c_int64(-1)
    assert lib.fx_index_remove_ids(other._h, used, ctypes.byref(n)) == -1 and "another index" in _lib.last_error()
    assert other.ntotal == NMAX
    assert lib.fx_index_remove_ids(ix._h, used, ctypes.byref(n)) == 0 and n.value == 50
    assert ix.ntotal == NMAX - 50
    Dh, Ih = np.empty((1, 5), dtype=np.float32), np.empty((1, 5), dtype=np.int64)
    args = (1, xq.ctypes.data, _lib.F32, _lib.MEM_HOST, 5, Dh.ctypes.data, Ih.ctypes.data, _lib.MEM_HOST)
    for h in (before, used):
        assert lib.fx_index_search_sel(ix._h, h, *args) == -1 and "stale" in _lib.last_error()
        assert lib.fx_index_remove_ids(ix._h, h, ctypes.byref(n)) == -1 and "stale" in _lib.last_error()
    ix.add(Y[100:150])
    assert ix.ntotal == NMAX
    for h in (before, used):
        assert lib.fx_index_search_sel(ix._h, h, *args) == -1 and "stale" in _lib.last_error()
        assert lib.fx_index_remove_ids(ix._h, h, ctypes.byref(n)) == -1 and "stale" in _lib.last_error()
        lib.fx_selector_free(h)
    assert ix.ntotal == NMAX
    Y2 = np.concatenate([Y[:100], Y[150:], Y[100:150]])
    assert ix.reconstruct_n(0, NMAX).tobytes() == Y2.tobytes()


def test_search_graph_is_dropped(fx, values):
    """A captured one-query search, then remove row 0 and add one row (the old
    ntotal again): the next search equals a fresh index's."""
    d = 384
    ix, Y, xq = _build(fx, values, "L2", "float32", d, NMAX)
    ix.set_option("search_graph", 1)
    ix.search(xq[:1], 10)
    ix.search(xq[:1], 10)  # captured by the first, replayed by the second
    assert ix.remove_ids([0]) == 1
    ix.add(Y[:1] * 0.5)
    Y2 = np.concatenate([Y[1:], Y[:1] * 0.5])
    fresh = fx.IndexFlatL2(d)
    fresh.add(Y2)
    for _ in range(2):
        D, I = ix.search(xq[:1], 10)
        Df, If = fresh.search(xq[:1], 10)
        np.testing.assert_array_equal(I, If)
        assert D.tobytes() == Df.tobytes()
    assert_parity(D, I, *oracle("L2", xq[:1], Y2, 10))


@pytest.mark.parametrize("case", [CASES[1], CASES[4]], ids=[CASE_IDS[1], CASE_IDS[4]])
def test_device_ids(fx, values, torch_cuda, case):
    """remove_ids with an int64 device tensor equals the host-array call."""
    metric, dtype, d = case
    ids = np.flatnonzero(third(NMAX) | block(NMAX, 2000, 2100))
    a, Y, xq = _build(fx, values, metric, dtype, d, NMAX)
    b, _, _ = _build(fx, values, metric, dtype, d, NMAX)
    na = a.remove_ids(torch_cuda.from_numpy(ids).cuda())
    nb = b.remove_ids(ids)
    assert na == nb == len(ids)
    assert a.reconstruct_n(0, a.ntotal).tobytes() == b.reconstruct_n(0, b.ntotal).tobytes()
    keep = np.ones(NMAX, dtype=bool)
    keep[ids] = False
    check_removed(fx, metric, dtype, a, Y, keep, xq, na)


def test_outlier_and_the_recomputed_maximum(fx, values):
    """A removed outlier leaves no trace in the certification bound: add one row
    of 1e3 x a corpus row to a bf16 d = 768 L2 index, remove it, and the search is
    byte-equal to the one before with no exact fallback and the same number
    of re-scanned queries.

    last_fallbacks() of the untouched index was measured first: 3 freshly built
    indexes, 12 searches each, gave 0 re-scanned and 0 exact-fallback queries
    every time (spread 0), so equality is asserted."""
    ix, Y, xq = _build(fx, values, "L2", "bfloat16", 768, NMAX)
    D0, I0 = ix.search(xq, 10)
    f0 = ix.last_fallbacks()
    ix.add(Y[7:8] * 1e3)
    assert ix.ntotal == NMAX + 1
    assert ix.remove_ids([NMAX]) == 1
    D, I = ix.search(xq, 10)
    np.testing.assert_array_equal(I, I0)
    assert D.tobytes() == D0.tobytes()
    print(f"fallbacks before {f0}, after {ix.last_fallbacks()}, exact {ix.last_exact_fallbacks()}")
    assert ix.last_exact_fallbacks() == 0
    assert ix.last_fallbacks() == f0


def test_store_remove_vectors_on_the_shipped_index(fx, golden_dir, tmp_path, monkeypatch):
    """FAISSVectorStore.remove_vectors on the shipped 23-row index: two
    documents go, searches return the rest as the oracle ranks them, and
    save_index / load_index round-trip the 21 rows and their ids."""
    from rag_faiss_embedding_amd import _mapping, faiss_store
    (tmp_path / "data").mkdir()
    shutil.copy(golden_dir / "shipped_index.bin", tmp_path / "data" / "faiss_index.bin")
    ids = json.loads((golden_dir / "shipped_ids.json").read_text())["mapping_ids"]
    (tmp_path / "data" / "faiss_index.bin.mapping").write_bytes(_mapping.dumps_ids(ids))
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(faiss_store.FAISSVectorStore, "_instance", None)
    monkeypatch.setattr(faiss_store.FAISSVectorStore, "_initialized", False)
    store = faiss_store.FAISSVectorStore()
    assert store.index.ntotal == 23 and store.doc_ids == ids
    xb = store.index.reconstruct_n(0, 23)
    gone = {ids[3], ids[17]}
    keep = np.array([doc not in gone for doc in ids])
    n_gone = int((~keep).sum())
    assert store.remove_vectors(list(gone) + [10 ** 9]) == n_gone
    left = [doc for doc in ids if doc not in gone]
    assert store.index.ntotal == 23 - n_gone and store.doc_ids == left
    assert store.remove_vectors([10 ** 9]) == 0 and store.remove_vectors([]) == 0
    kept = np.ascontiguousarray(xb[keep])
    for qi in (0, 3, 17, 20):
        for k in (3, 5, 23):
            D, found = store.search(xb[qi], k)
            Dr, Ir = C.knn_exact(xb[qi:qi + 1], kept, min(k, len(kept)))
            assert found == [left[r] for r in Ir[0]]
            assert not set(found) & gone
            np.testing.assert_allclose(D, Dr[0], rtol=1e-5, atol=1e-5)
    store.save_index()
    store.reset()
    assert store.index.ntotal == 0 and store.doc_ids == []
    store.load_index()
    assert store.index.ntotal == 23 - n_gone and store.doc_ids == left
    assert store.index.reconstruct_n(0, 23 - n_gone).tobytes() == kept.tobytes()

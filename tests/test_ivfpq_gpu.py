"""GPU checks of IndexIVFPQ (fx_ivfpq.hip through the C ABI and the Python layer) against the numpy
reference of tests/_ivfpq_ref.py and the scan model of tests/test_ivfpq_model.py.

As in tests/test_ivfsq_gpu.py most tests skip k-means: the coarse centroids are given, the rows are
``centroid + small noise`` with prescribed per-list counts, and the codebook is sampled from the
rows' residuals, so the shapes hit the list scan's edges.  Every list's codes must be bitwise the
reference's in insertion order, fx_ivfpq_residuals bitwise the reference's, ids equal to the
reference's, distances within 1e-5 * max(1, |D_ref|).  The exact list scan repairs every query the
refine cannot certify, so a broken gather scan would show only as flagged queries: at k = 1 and k =
10 ``last_fallbacks()`` must lie in the model's range of uncertified queries (E scaled by 1 -+ 1e-5
and the merged list's last key moved by the accumulation term)."""
import numpy as np
import pytest

from tests import _ivf_ref as IV
from tests import _ivfpq_ref as R
from tests import _kmeans_ref as kref
from tests.test_ivfpq_model import FUSED_SHAPES, ScanModel, edge_model, groups_corpus, long_corpus, plan_chunks

pytestmark = pytest.mark.gpu

L2, IP = R.METRIC_L2, R.METRIC_INNER_PRODUCT


@pytest.fixture(scope="module")
def fx():
    from rag_faiss_embedding_amd import _lib, faiss
    if _lib.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    return faiss


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def make_index(mod, centroids, M, metric, by_residual=True, cents=None):
    nlist, d = centroids.shape
    q = (mod.IndexFlatL2 if metric == L2 else mod.IndexFlatIP)(d)
    q.add(centroids)
    ix = mod.IndexIVFPQ(q, d, nlist, M, 8, metric, by_residual)
    if cents is not None:
        ix.pq.centroids = cents
    return ix


def check(ix, got, want, what):
    D, I = got
    Dr, Ir = want
    assert ix.last_dropped_candidates() == 0, f"{what}: dropped candidates"
    bad = np.flatnonzero((I != Ir).any(1))
    assert bad.size == 0, f"{what}: ids differ for queries {bad[:5]}: {I[bad[0]]} vs {Ir[bad[0]]}"
    err = np.abs(D.astype(np.float64) - Dr.astype(np.float64))
    assert (err <= 1e-5 * np.maximum(1.0, np.abs(Dr))).all(), f"{what}: distances off by {err.max()}"


def check_flags(ix, m, nprobe, k, what):
    plan = ix.last_ivf_plan()
    C = plan["chunks"]
    assert C == plan_chunks(m.nq, min(nprobe, m.nlist), m.max_list_rows()), plan
    lo, hi = m.flagged_range(nprobe, C, k)
    got = ix.last_fallbacks()
    print(f"{what}: {got} of {m.nq} queries flagged (model: {lo} .. {hi}), chunks {C}")
    assert lo <= got <= hi, f"{what}: {got} flagged, the model has {lo} .. {hi}"


def check_payload(ix, ref, lists, ids, what):
    assert (ix.pq.centroids.view(np.uint32) == ref.cents.reshape(-1).view(np.uint32)).all(), f"{what}: centroids"
    sizes = np.bincount(lists, minlength=ix.nlist)
    assert (ix.list_sizes() == sizes).all(), f"{what}: list sizes"
    for l in range(ix.nlist):
        assert (ix.get_list_ids(l) == ids[lists == l]).all(), f"{what}: list {l}: ids / insertion order"
        assert (ix.get_list_codes(l) == ref.list_codes(l)).all(), f"{what}: list {l}: codes"


def check_residuals(ix, torch, xb, lists, c, by_residual):
    want = R.residuals(xb, lists, c, by_residual)
    got = ix._residuals(xb).cpu().numpy()
    assert (got.view(np.uint32) == want.view(np.uint32)).all(), "residuals from host rows"
    got = ix._residuals(torch.from_numpy(np.array(xb)).to("cuda:0")).cpu().numpy()
    assert (got.view(np.uint32) == want.view(np.uint32)).all(), "residuals from device rows"


EDGE = [(d, M, m, br) for d, M in FUSED_SHAPES for m in (L2, IP) for br in (True, False)]


@pytest.mark.parametrize("d,M,metric,by_residual", EDGE,
                         ids=[f"d{d}-M{M}-{'L2' if m == L2 else 'IP'}-{'res' if br else 'plain'}" for d, M, m, br in EDGE])
def test_list_edges(fx, torch, d, M, metric, by_residual):
    c, xb, lists, xq = IV.edge_corpus(d, "float32")
    assert (IV.assign(xb, c, metric) == lists).all(), "the corpus does not realise the prescribed lists"
    m = edge_model(d, M, metric, by_residual)
    ix = make_index(fx, c, M, metric, by_residual)
    assert not ix.is_trained and ix.code_size == M and ix.by_residual == by_residual and ix.pq.dsub == d // M
    with pytest.raises(AssertionError, match="not trained"):
        ix.search(xq, 1)
    ix.pq.centroids = m.cents
    assert ix.is_trained and ix.ntotal == 0
    check_residuals(ix, torch, xb, lists, c, by_residual)
    ix.add(xb)
    ids = np.arange(xb.shape[0], dtype=np.int64)
    assert ix.ntotal == xb.shape[0]
    check_payload(ix, m.ref, lists, ids, "edge")
    full = m.ref.ranking(xq, metric)
    for nprobe in (1, 3, 12):
        ix.nprobe = nprobe
        for k in (1, 10, 32):
            what = f"d={d} M={M} nprobe={nprobe} k={k}"
            want = m.ref.search(xq, ids, k, nprobe, metric, full=full)
            check(ix, ix.search(xq, k), want, what)
            assert ix.last_ivf_plan()["path"] == "fused", what
            if k <= 10:
                check_flags(ix, m, nprobe, k, what)
    ix.nprobe = 3
    want = m.ref.search(xq, ids, 33, 3, metric, full=full)
    check(ix, ix.search(xq, 33), want, "k=33")
    assert ix.last_ivf_plan()["path"] == "exact"


@pytest.mark.parametrize("metric", [L2, IP], ids=["L2", "IP"])
@pytest.mark.parametrize("by_residual", [True, False], ids=["res", "plain"])
def test_dsub_4_takes_the_exact_path(fx, metric, by_residual):
    d, M = 20, 5
    c, xb, lists, xq = IV.edge_corpus(d, "float32")
    cents = R.codebook(xb, lists, c, M, by_residual)
    ref = R.Model(xb, lists, c, cents, by_residual)
    ix = make_index(fx, c, M, metric, by_residual, cents)
    ix.add(xb)
    ids = np.arange(xb.shape[0], dtype=np.int64)
    check_payload(ix, ref, lists, ids, "dsub 4")
    full = ref.ranking(xq, metric)
    for nprobe in (1, 3, 12):
        ix.nprobe = nprobe
        for k in (1, 10, 33):
            check(ix, ix.search(xq, k), ref.search(xq, ids, k, nprobe, metric, full=full), f"dsub 4 nprobe={nprobe} k={k}")
            assert ix.last_ivf_plan()["path"] == "exact"


def test_more_than_one_pair_group_per_list(fx):
    c, xb, lists, xq = groups_corpus()
    m = ScanModel(c, xb, lists, xq, L2, 48)
    ix = make_index(fx, c, 48, L2, True, m.cents)
    ix.add(xb)
    ix.nprobe = 2
    want = m.ref.search(xq, np.arange(xb.shape[0]), 10, 2, L2)
    check(ix, ix.search(xq, 10), want, "pair groups")
    check_flags(ix, m, 2, 10, "pair groups")


@pytest.mark.parametrize("nq", [1, 5])
def test_chunked_long_list_at_small_nq(fx, nq):
    c, xb, lists, xq = long_corpus(nq)
    m = ScanModel(c, xb, lists, xq, L2, 48)
    ix = make_index(fx, c, 48, L2, True, m.cents)
    ix.add(xb)
    want = m.ref.search(xq, np.arange(xb.shape[0]), 10, 1, L2)
    check(ix, ix.search(xq, 10), want, f"chunked nq={nq}")
    plan = ix.last_ivf_plan()
    assert plan["chunks"] > 1 and plan["slots"] == plan["chunks"], plan
    check_flags(ix, m, 1, 10, f"chunked nq={nq}")


def test_two_batches_reset_and_arbitrary_ids(fx):
    d, M = 384, 48
    c, xb, lists, xq = IV.edge_corpus(d, "float32")
    n = xb.shape[0]
    ids = np.arange(n, dtype=np.int64)
    cents = R.codebook(xb, lists, c, M)
    ix = make_index(fx, c, M, L2, True, cents)
    ix.nprobe = 3
    cut = 1000
    first = R.Model(xb[:cut], lists[:cut], c, cents)
    ix.add(xb[:cut])
    check(ix, ix.search(xq, 10), first.search(xq, ids[:cut], 10, 3, L2), "first add")
    check_payload(ix, first, lists[:cut], ids[:cut], "first add")
    ix.add(xb[cut:])
    whole = R.Model(xb, lists, c, cents)
    check(ix, ix.search(xq, 10), whole.search(xq, ids, 10, 3, L2), "second add")
    check_payload(ix, whole, lists, ids, "second add")
    with pytest.raises(AssertionError):
        ix.add_with_ids(xb[:3], ids[:3])
    with pytest.raises(AssertionError):
        ix.pq.centroids = cents  # the index holds rows
    ix.reset()
    assert ix.ntotal == 0 and ix.is_trained and ix.quantizer.ntotal == len(IV.EDGE_SIZES)
    assert (ix.list_sizes() == 0).all() and (ix.pq.centroids == cents.reshape(-1)).all()
    D, I = ix.search(xq, 3)
    assert (I == -1).all() and (D == R.FLT_MAX).all()
    weird = ids * 3 - 7  # negative ids
    weird[5:10] = (1 << 40) + np.arange(5)  # above 2^32
    weird[20:30] = 12345  # duplicates
    ix.add_with_ids(xb[:cut], weird[:cut])
    check(ix, ix.search(xq, 10), first.search(xq, weird[:cut], 10, 3, L2), "add_with_ids")
    check_payload(ix, first, lists[:cut], weird[:cut], "add_with_ids")
    with pytest.raises(AssertionError):
        ix.add(xb[:3])
    with pytest.raises(NotImplementedError):
        fx.write_index(ix, "/nonexistent/ivfpq.bin")


@pytest.mark.stream_ordered
def test_device_tensors_in_and_out(fx, torch):
    d, M = 384, 48
    c, xb, lists, xq = IV.edge_corpus(d, "float32")
    cents = R.codebook(xb, lists, c, M)
    ref = R.Model(xb, lists, c, cents)
    ix = make_index(fx, c, M, L2, True, cents)
    ix.add(torch.from_numpy(np.array(xb)).to("cuda:0"))
    ix.nprobe = 3
    outs = []
    tq = torch.from_numpy(np.array(xq)).to("cuda:0")
    for k in (10, 40):
        D, I = ix.search(tq, k)
        assert D.is_cuda and I.is_cuda and D.dtype == torch.float32 and I.dtype == torch.int64
        outs.append((k, D, I))
    for k, D, I in outs:
        want = ref.search(xq, np.arange(xb.shape[0]), k, 3, L2)
        check(ix, (D.cpu().numpy(), I.cpu().numpy()), want, f"device k={k}")
        Dh, Ih = ix.search(xq, k)
        assert (Ih == I.cpu().numpy()).all() and (Dh == D.cpu().numpy()).all()


def test_end_to_end_train_with_kmeans(fx, torch):
    x, _ = kref.blobs(2000, 64, 8, 1, 0)
    x = np.array(x)
    d, nlist, M = 64, 8, 8
    ix = fx.IndexIVFPQ(fx.IndexFlatL2(d), d, nlist, M, pq_niter=4)
    assert not ix.is_trained
    with pytest.raises(AssertionError):
        ix.add(x[:5])
    with pytest.raises(RuntimeError, match="fewer than"):
        fx.IndexIVFPQ(fx.IndexFlatL2(d), d, 2, M).train(x[:100])
    ix.train(x)
    assert ix.is_trained and ix.quantizer.ntotal == nlist
    got = ix.pq.centroids.copy()
    ix.train(x)  # a no-op on a trained index
    assert (ix.pq.centroids == got).all()
    c = ix.quantizer.reconstruct_n(0, nlist)  # the centroids as stored
    lists = IV.assign(x, c, L2)
    # the codebook equals M direct Kmeans runs on the slices of the residuals
    res = R.residuals(x, lists, c)
    dsub = d // M
    for m in range(M):
        km = fx.Kmeans(dsub, 256, niter=4, seed=1234)
        km.train(np.ascontiguousarray(res[:, m * dsub:(m + 1) * dsub]))
        assert (got.reshape(M, 256, dsub)[m].view(np.uint32) == np.asarray(km.centroids).view(np.uint32)).all(), m
    ix.add(x)
    ref = R.Model(x, lists, c, got.reshape(M, 256, dsub))
    ids = np.arange(x.shape[0], dtype=np.int64)
    check_payload(ix, ref, lists, ids, "k-means")
    xq = x[::97] + np.float32(0.01)
    check(ix, ix.search(xq, 10, params=fx.SearchParametersIVF(nprobe=4)), ref.search(xq, ids, 10, 4, L2), "end to end")
    with pytest.raises(NotImplementedError):
        ix.search(xq, 10, params=fx.SearchParametersIVF(sel=fx.IDSelectorRange(0, 5)))
    with pytest.raises(NotImplementedError):
        ix.search(xq, 1025)
    with pytest.raises(NotImplementedError):
        fx.IndexIVFPQ(fx.IndexFlatL2(d), d, nlist, M, 4)
    with pytest.raises(ValueError):
        fx.IndexIVFPQ(fx.IndexFlatL2(d), d, nlist, 7)


def test_forced_fallback_equals_unforced(fx, diag_fx, monkeypatch):
    d, M = 384, 48
    c, xb, lists, xq = IV.edge_corpus(d, "float32")
    cents = R.codebook(xb, lists, c, M)
    res = []
    for force in (None, "1"):
        if force:
            monkeypatch.setenv("FX_FORCE_FALLBACK", force)  # (read when the index is created)
        ix = make_index(diag_fx, c, M, L2, True, cents)
        monkeypatch.delenv("FX_FORCE_FALLBACK", raising=False)
        ix.add(xb)
        ix.nprobe = 3
        D, I = ix.search(xq, 10)
        assert ix.last_dropped_candidates() == 0
        res.append((D, I, ix.last_fallbacks()))
    (D0, I0, f0), (D1, I1, f1) = res
    assert f0 == 0 and f1 == xq.shape[0]
    assert (I0 == I1).all() and (D0.view(np.uint32) == D1.view(np.uint32)).all()


def test_store_consumer(fx, monkeypatch):
    from rag_faiss_embedding_amd import faiss_store
    x, _ = kref.blobs(2000, 64, 16, 7, 0)
    x = np.array(x)
    monkeypatch.setattr(faiss_store.FAISSVectorStore, "_instance", None)
    monkeypatch.setattr(faiss_store.FAISSVectorStore, "_initialized", False)
    store = faiss_store.FAISSVectorStore(dimension=64, index_path="/nonexistent/none.bin")
    doc_ids = [5000 + 3 * i for i in range(x.shape[0])]
    store.add_vectors(x, doc_ids)
    with pytest.raises(ValueError):
        store.build_ivf(8, qtype=fx.ScalarQuantizer.QT_8bit, pq_m=8)
    ix = store.build_ivf(8, pq_m=8)
    assert store.ivf is ix and isinstance(ix, fx.IndexIVFPQ)
    assert ix.ntotal == 2000 and ix.nprobe == 8 and ix.by_residual and ix.code_size == 8
    for q in (x[3] + np.float32(0.02), x[1500] * np.float32(0.9)):
        for nprobe in (2, 8):
            Ds, ids = store.search(q, 5, nprobe=nprobe)
            D, I = ix.search(q.reshape(1, -1), 5, params=fx.SearchParametersIVF(nprobe=nprobe))
            assert ids == [doc_ids[r] for r in I[0]] and (np.asarray(Ds, dtype=np.float32) == D[0]).all()
            assert ix.last_dropped_candidates() == 0
    store.add_vectors(x[:1], [1])
    assert store.ivf is None

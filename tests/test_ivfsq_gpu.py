"""GPU checks of IndexIVFScalarQuantizer (fx_ivfsq.hip through the C ABI and the Python layer) against
the numpy reference of tests/_ivfsq_ref.py and the scan model of tests/test_ivfsq_model.py.

As in tests/test_ivf_gpu.py most tests skip k-means: the centroids are given and the rows are
``centroid + small noise`` with prescribed per-list counts, so the shapes hit the list scan's edges.
The tables must be bitwise the reference's, every list's codes bitwise the reference's in insertion
order, ids equal to the reference's, distances within 1e-5 * max(1, |D_ref|).  The exact list scan
repairs every query the refine cannot certify, so a broken int8 scan would show only as flagged
queries: at k = 1 and k = 10 ``last_fallbacks()`` must be the model's count of uncertified queries
(the model's E is the device's fp64 formula summed in another order, so the count is taken with E
scaled by 1 -+ 1e-5 and both must agree with the device where they agree with each other)."""
import numpy as np
import pytest

from tests import _ivf_ref as IV
from tests import _ivfsq_ref as R
from tests import _kmeans_ref as kref
from tests.test_ivfsq_model import ScanModel, edge_model, groups_corpus, long_corpus, plan_chunks

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


def make_index(mod, centroids, metric, qtype=R.QT_8bit, by_residual=True):
    nlist, d = centroids.shape
    q = (mod.IndexFlatL2 if metric == L2 else mod.IndexFlatIP)(d)
    q.add(centroids)
    return mod.IndexIVFScalarQuantizer(q, d, nlist, qtype, metric, by_residual)


def full_trained(ix):
    t = ix.trained
    if t.size == 2:
        t = np.concatenate([np.full(ix.d, t[0], np.float32), np.full(ix.d, t[1], np.float32)])
    return t


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
    assert (full_trained(ix).view(np.uint32) == ref.trained.view(np.uint32)).all(), f"{what}: trained"
    sizes = np.bincount(lists, minlength=ix.nlist)
    assert (ix.list_sizes() == sizes).all(), f"{what}: list sizes"
    for l in range(ix.nlist):
        assert (ix.get_list_ids(l) == ids[lists == l]).all(), f"{what}: list {l}: ids / insertion order"
        assert (ix.get_list_codes(l) == ref.list_codes(l)).all(), f"{what}: list {l}: codes"


EDGE = [(d, m, br, R.QT_8bit) for d in (20, 384, 1100) for m in (L2, IP) for br in (True, False)]
EDGE += [(384, m, True, R.QT_8bit_uniform) for m in (L2, IP)]


@pytest.mark.parametrize("d,metric,by_residual,qtype", EDGE,
                         ids=[f"d{d}-{'L2' if m == L2 else 'IP'}-{'res' if br else 'plain'}-qt{qt}"
                              for d, m, br, qt in EDGE])
def test_list_edges(fx, d, metric, by_residual, qtype):
    c, xb, lists, xq = IV.edge_corpus(d, "float32")
    assert (IV.assign(xb, c, metric) == lists).all(), "the corpus does not realise the prescribed lists"
    m = edge_model(d, metric, by_residual, qtype)
    ix = make_index(fx, c, metric, qtype, by_residual)
    assert not ix.is_trained and ix.code_size == d and ix.by_residual == by_residual
    with pytest.raises(AssertionError, match="not trained"):
        ix.search(xq, 1)
    ix.train(xb)
    assert ix.is_trained and ix.ntotal == 0
    ix.add(xb)
    ids = np.arange(xb.shape[0], dtype=np.int64)
    assert ix.ntotal == xb.shape[0]
    check_payload(ix, m.ref, lists, ids, "edge")
    full = m.ref.ranking(xq, metric)
    for nprobe in (1, 3, 12, 50):
        ix.nprobe = nprobe
        for k in (1, 10, 32, 100):
            what = f"d={d} nprobe={nprobe} k={k}"
            want = m.ref.search(xq, ids, k, nprobe, metric, full=full)
            check(ix, ix.search(xq, k), want, what)
            assert ix.last_ivf_plan()["path"] == ("fused" if k <= 32 else "exact"), what
            if k <= 10:
                check_flags(ix, m, nprobe, k, what)


def test_more_than_one_pair_group_per_list(fx):
    c, xb, lists, xq = groups_corpus()
    m = ScanModel(c, xb, lists, xq, L2)
    ix = make_index(fx, c, L2)
    ix.train(xb)
    ix.add(xb)
    ix.nprobe = 2
    want = m.ref.search(xq, np.arange(xb.shape[0]), 10, 2, L2)
    check(ix, ix.search(xq, 10), want, "pair groups")
    check_flags(ix, m, 2, 10, "pair groups")


@pytest.mark.parametrize("nq", [1, 5])
def test_chunked_long_list_at_small_nq(fx, nq):
    c, xb, lists, xq = long_corpus(nq)
    m = ScanModel(c, xb, lists, xq, L2)
    ix = make_index(fx, c, L2)
    ix.train(xb)
    ix.add(xb)
    want = m.ref.search(xq, np.arange(xb.shape[0]), 10, 1, L2)
    check(ix, ix.search(xq, 10), want, f"chunked nq={nq}")
    plan = ix.last_ivf_plan()
    assert plan["chunks"] > 1 and plan["slots"] == plan["chunks"], plan
    check_flags(ix, m, 1, 10, f"chunked nq={nq}")


def test_two_batches_reset_and_arbitrary_ids(fx):
    d = 384
    c, xb, lists, xq = IV.edge_corpus(d, "float32")
    n = xb.shape[0]
    ids = np.arange(n, dtype=np.int64)
    ix = make_index(fx, c, L2)
    ix.nprobe = 3
    ix.train(xb)  # the tables of the whole corpus, then the rows in two batches
    trained = full_trained(ix)
    cut = 1000
    first = R.Model(xb[:cut], lists[:cut], c, train=(xb, lists))
    ix.add(xb[:cut])
    check(ix, ix.search(xq, 10), first.search(xq, ids[:cut], 10, 3, L2), "first add")
    check_payload(ix, first, lists[:cut], ids[:cut], "first add")
    ix.add(xb[cut:])
    whole = R.Model(xb, lists, c)
    check(ix, ix.search(xq, 10), whole.search(xq, ids, 10, 3, L2), "second add")
    check_payload(ix, whole, lists, ids, "second add")
    with pytest.raises(AssertionError):
        ix.add_with_ids(xb[:3], ids[:3])
    ix.reset()
    assert ix.ntotal == 0 and ix.is_trained and ix.quantizer.ntotal == len(IV.EDGE_SIZES)
    assert (ix.list_sizes() == 0).all() and (full_trained(ix) == trained).all()
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
    # a training kept with numpy makes a second index that encodes alike
    ix2 = make_index(fx, c, L2)
    ix2.set_trained(trained)
    assert ix2.is_trained
    ix2.add(xb[:cut])
    check_payload(ix2, first, lists[:cut], ids[:cut], "set_trained")
    with pytest.raises(NotImplementedError):
        fx.write_index(ix2, "/nonexistent/ivfsq.bin")


@pytest.mark.stream_ordered
def test_device_tensors_in_and_out(fx, torch):
    d = 384
    c, xb, lists, xq = IV.edge_corpus(d, "float32")
    ref = R.Model(xb, lists, c)
    ix = make_index(fx, c, L2)
    tb = torch.from_numpy(np.array(xb)).to("cuda:0")
    ix.train(tb)
    ix.add(tb)
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


def test_end_to_end_train_with_kmeans(fx):
    x, _ = kref.blobs(2000, 100, 8, 1, 0)
    x = np.array(x)
    d, nlist = 100, 8
    ix = fx.IndexIVFScalarQuantizer(fx.IndexFlatL2(d), d, nlist)
    assert not ix.is_trained
    with pytest.raises(AssertionError):
        ix.add(x[:5])
    ix.train(x)
    assert ix.is_trained and ix.quantizer.ntotal == nlist
    ix.train(x)  # a no-op on a trained index
    ix.add(x)
    c = ix.quantizer.reconstruct_n(0, nlist)  # the centroids as stored
    lists = IV.assign(x, c, L2)
    ref = R.Model(x, lists, c)
    ids = np.arange(x.shape[0], dtype=np.int64)
    check_payload(ix, ref, lists, ids, "k-means")  # every row lies in the list the quantizer assigns it to
    ix.nprobe = 4
    xq = x[::97] + np.float32(0.01)
    check(ix, ix.search(xq, 10, params=fx.SearchParametersIVF(nprobe=4)), ref.search(xq, ids, 10, 4, L2), "end to end")
    with pytest.raises(NotImplementedError):
        ix.search(xq, 10, params=fx.SearchParametersIVF(sel=fx.IDSelectorRange(0, 5)))
    with pytest.raises(NotImplementedError):
        ix.search(xq, 1025)
    with pytest.raises(NotImplementedError):
        fx.IndexIVFScalarQuantizer(fx.IndexFlatL2(d), d, nlist, fx.ScalarQuantizer.QT_4bit)


def test_forced_fallback_equals_unforced(fx, diag_fx, monkeypatch):
    d = 384
    c, xb, lists, xq = IV.edge_corpus(d, "float32")
    res = []
    for force in (None, "1"):
        if force:
            monkeypatch.setenv("FX_FORCE_FALLBACK", force)  # (read when the index is created)
        ix = make_index(diag_fx, c, L2)
        monkeypatch.delenv("FX_FORCE_FALLBACK", raising=False)
        ix.train(xb)
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
    x, _ = kref.blobs(2000, 100, 16, 7, 0)
    x = np.array(x)
    monkeypatch.setattr(faiss_store.FAISSVectorStore, "_instance", None)
    monkeypatch.setattr(faiss_store.FAISSVectorStore, "_initialized", False)
    store = faiss_store.FAISSVectorStore(dimension=100, index_path="/nonexistent/none.bin")
    doc_ids = [5000 + 3 * i for i in range(x.shape[0])]
    store.add_vectors(x, doc_ids)
    ix = store.build_ivf(8, qtype=fx.ScalarQuantizer.QT_8bit)
    assert store.ivf is ix and isinstance(ix, fx.IndexIVFScalarQuantizer)
    assert ix.ntotal == 2000 and ix.nprobe == 8 and ix.by_residual
    for q in (x[3] + np.float32(0.02), x[1500] * np.float32(0.9)):
        for nprobe in (2, 8):
            Ds, ids = store.search(q, 5, nprobe=nprobe)
            D, I = ix.search(q.reshape(1, -1), 5, params=fx.SearchParametersIVF(nprobe=nprobe))
            assert ids == [doc_ids[r] for r in I[0]] and (np.asarray(Ds, dtype=np.float32) == D[0]).all()
            assert ix.last_dropped_candidates() == 0
    store.build_sq()
    D, ids = store.search(x[0], 5, sq=True, nprobe=2)  # not offered together, as before: swallowed to empty
    assert ids == [] and D.size == 0
    store.add_vectors(x[:1], [1])
    assert store.ivf is None
    assert store.search(x[0], 5, nprobe=2)[1] == []

"""GPU checks of IndexIVFFlat (fx_ivf.hip through the C ABI and the Python
layer) against the numpy reference of tests/_ivf_ref.py.

Most tests skip training: the centroids are given (well-separated points added
to the quantizer) and the rows are ``centroid + small noise`` with prescribed
per-list counts, so the shapes hit the list scan's edges.  Ids must equal the
reference exactly -- the coarse search is bit-exact and the ranking rule
(distance, list, insertion order) is the reference's -- and distances agree
within 1e-5 * max(1, |D_ref|).  The conftest fixture that checks the candidate
lists only wraps the flat index's search, so every search here asserts
``last_dropped_candidates() == 0`` itself.  The exact list scan repairs every
query the refine cannot certify, so the tests of the fused path also assert
``last_fallbacks() == 0`` at k = 1 and k = 10: the MFMA scan and the refine
must have served those results themselves (k = 32 leaves the refine no room
and is flagged by design)."""
import numpy as np
import pytest

from tests import _ivf_ref as ref
from tests import _kmeans_ref as kref

pytestmark = pytest.mark.gpu

L2, IP = ref.METRIC_L2, ref.METRIC_INNER_PRODUCT
DTYPES = ["float32", "bfloat16", "float16"]


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


def quantizer(mod, d, metric, centroids, dtype="float32"):
    q = (mod.IndexFlatL2 if metric == L2 else mod.IndexFlatIP)(d, dtype=dtype)
    q.add(centroids)
    return q


def make_ivf(fx, centroids, metric, dtype, mod=None):
    nlist, d = centroids.shape
    q = quantizer(mod or fx, d, metric, centroids)
    return fx.IndexIVFFlat(q, d, nlist, metric, dtype=dtype)


def check(ivf, got, want, what):
    D, I = got
    Dr, Ir = want
    assert ivf.last_dropped_candidates() == 0, f"{what}: dropped candidates"
    bad = np.flatnonzero((I != Ir).any(1))
    assert bad.size == 0, f"{what}: ids differ for queries {bad[:5]}: {I[bad[0]]} vs {Ir[bad[0]]}"
    err = np.abs(D.astype(np.float64) - Dr.astype(np.float64))
    assert (err <= 1e-5 * np.maximum(1.0, np.abs(Dr))).all(), f"{what}: distances off by {err.max()}"


@pytest.mark.parametrize("metric", [L2, IP], ids=["L2", "IP"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [20, 384, 768])
def test_list_edges(fx, d, dtype, metric):
    c, xb, lists, xq = ref.edge_corpus(d, dtype)
    assert (ref.assign(xb, c, metric) == lists).all(), "the corpus does not realise the prescribed lists"
    ivf = make_ivf(fx, c, metric, dtype)
    assert ivf.is_trained and ivf.ntotal == 0
    ivf.add(xb)
    ids = np.arange(xb.shape[0], dtype=np.int64)
    assert ivf.ntotal == xb.shape[0]
    assert (ivf.list_sizes() == np.array(ref.EDGE_SIZES)).all()
    for l in range(len(ref.EDGE_SIZES)):
        assert (ivf.get_list_ids(l) == np.flatnonzero(lists == l)).all(), f"list {l}: ids / insertion order"
    full = ref.ranking(xq, xb, lists, metric)
    for nprobe in (1, 3, 12, 50):
        ivf.nprobe = nprobe
        for k in (1, 10, 32):
            want = ref.search(xq, xb, ids, lists, c, k, nprobe, metric, full=full)
            check(ivf, ivf.search(xq, k), want, f"d={d} {dtype} nprobe={nprobe} k={k}")
            assert ivf.last_ivf_plan()["path"] == "fused"
            if k <= 10:  # the MFMA scan + refine serve these themselves: nothing falls to the exact list scan
                assert ivf.last_fallbacks() == 0, f"d={d} {dtype} nprobe={nprobe} k={k}: flagged queries"


def test_more_than_one_query_group_per_list(fx):
    d, dtype = 384, "bfloat16"
    c, xb, lists, _ = ref.edge_corpus(d, dtype)
    r = np.random.default_rng(5)
    ql = np.concatenate([np.full(300, 11), r.integers(0, 11, 20)])  # 300 queries nearest to the 1000-row list
    r.shuffle(ql)
    xq = kref.round_to(c[ql] + 0.1 * r.standard_normal((ql.size, d)).astype(np.float32), dtype)
    assert (ref.assign(xq, c, L2) == ql).all()
    ivf = make_ivf(fx, c, L2, dtype)
    ivf.add(xb)
    ivf.nprobe = 2
    want = ref.search(xq, xb, np.arange(xb.shape[0]), lists, c, 10, 2, L2)
    check(ivf, ivf.search(xq, 10), want, "query groups")
    assert ivf.last_fallbacks() == 0


@pytest.mark.parametrize("nq", [1, 5])
def test_chunked_long_list_at_small_nq(fx, nq):
    d, dtype = 384, "bfloat16"
    sizes = (20000, 3, 0, 130, 1, 64, 7, 256)
    c, xb, lists, xq = ref.edge_corpus(d, dtype, sizes=sizes, seed=3, nq=5)
    r = np.random.default_rng(8)
    xq = kref.round_to(c[np.zeros(nq, dtype=int)] + 0.1 * r.standard_normal((nq, d)).astype(np.float32), dtype)
    ivf = make_ivf(fx, c, L2, dtype)
    ivf.add(xb)
    want = ref.search(xq, xb, np.arange(xb.shape[0]), lists, c, 10, 1, L2)
    check(ivf, ivf.search(xq, 10), want, f"chunked nq={nq}")
    assert ivf.last_fallbacks() == 0
    plan = ivf.last_ivf_plan()
    assert plan["chunks"] > 1 and plan["slots"] == plan["chunks"], plan


@pytest.mark.parametrize("metric", [L2, IP], ids=["L2", "IP"])
def test_exact_path_big_k(fx, metric):
    d, dtype = 384, "float16"
    c, xb, lists, xq = ref.edge_corpus(d, dtype)
    ivf = make_ivf(fx, c, metric, dtype)
    ivf.add(xb)
    ivf.nprobe = 3
    full = ref.ranking(xq, xb, lists, metric)
    for k in (33, 100, 1024):
        want = ref.search(xq, xb, np.arange(xb.shape[0]), lists, c, k, 3, metric, full=full)
        check(ivf, ivf.search(xq, k), want, f"exact k={k}")
        assert ivf.last_ivf_plan()["path"] == "exact"
    assert (want[1] == -1).any(), "k = 1024 should pad for some query"
    with pytest.raises(NotImplementedError):
        ivf.search(xq, 1025)


def test_forced_fallback_equals_unforced(fx, diag_fx):
    d, dtype = 384, "bfloat16"
    c, xb, lists, xq = ref.edge_corpus(d, dtype)
    ivf = make_ivf(fx, c, L2, dtype, mod=diag_fx)
    ivf.add(xb)
    ivf.nprobe = 3
    D0, I0 = ivf.search(xq, 10)
    assert ivf.last_dropped_candidates() == 0
    plain = ivf.last_fallbacks()
    ivf.quantizer.set_option("force_fallback", 1)
    D1, I1 = ivf.search(xq, 10)
    assert ivf.last_dropped_candidates() == 0
    assert ivf.last_fallbacks() == xq.shape[0] and plain == 0
    assert (I0 == I1).all() and (D0.view(np.uint32) == D1.view(np.uint32)).all()


@pytest.mark.parametrize("metric", [L2, IP], ids=["L2", "IP"])
def test_nprobe_nlist_equals_flat_index(fx, metric):
    n, d, nlist, k = 5000, 384, 16, 10
    r = np.random.default_rng(21)
    xb = r.standard_normal((n, d)).astype(np.float32)
    xq = r.standard_normal((64, d)).astype(np.float32)
    flat = (fx.IndexFlatL2 if metric == L2 else fx.IndexFlatIP)(d)
    flat.add(xb)
    Df, If = flat.search(xq, k + 1)
    assert (Df[:, 1:] != Df[:, :-1]).all(), "the flat result has tied distances in its top 11"
    ivf = make_ivf(fx, np.ascontiguousarray(xb[:nlist]), metric, "float32")
    ivf.add(xb)
    ivf.nprobe = nlist
    D, I = ivf.search(xq, k)
    assert ivf.last_dropped_candidates() == 0
    assert (I == If[:, :k]).all()
    assert (D.view(np.uint32) == Df[:, :k].view(np.uint32)).all()


def test_ties_order_by_distance_list_insertion(fx):
    d, nlist = 20, 6
    c = np.zeros((nlist, d), dtype=np.float32)
    c[np.arange(nlist), np.arange(nlist)] = 8.0  # integer-grid centroids 8 e_l
    r = np.random.default_rng(2)
    base = []
    for l in range(nlist):  # integer-grid rows: 8 e_l + e_j, which tie within and across lists
        for j in range(nlist, nlist + 5):
            v = c[l].copy()
            v[j] += 1.0
            base.append(v)
    base = np.array(base, dtype=np.float32)
    base = base[r.permutation(base.shape[0])]
    xb = np.repeat(base, 2, axis=0)  # every row twice, interleaved
    lists = ref.assign(xb, c, L2)
    xq = np.zeros((4, d), dtype=np.float32)
    xq[1, 0] = 4.0
    xq[1, 1] = 4.0  # equidistant from lists 0 and 1
    xq[2, 2] = 8.0
    xq[3, :nlist] = 1.0
    ivf = make_ivf(fx, c, L2, "float32")
    ivf.add(xb)
    for nprobe in (2, nlist):
        ivf.nprobe = nprobe
        for k in (5, 32):
            want = ref.search(xq, xb, np.arange(xb.shape[0]), lists, c, k, nprobe, L2)
            check(ivf, ivf.search(xq, k), want, f"ties nprobe={nprobe} k={k}")


def test_incremental_adds_reset_and_arbitrary_ids(fx):
    d, dtype = 384, "float32"
    c, xb, lists, xq = ref.edge_corpus(d, dtype)
    n = xb.shape[0]
    ivf = make_ivf(fx, c, L2, dtype)
    ivf.nprobe = 3
    ids = np.arange(n, dtype=np.int64)
    cut = 1000
    ivf.add(xb[:cut])
    check(ivf, ivf.search(xq, 10), ref.search(xq, xb[:cut], ids[:cut], lists[:cut], c, 10, 3, L2), "first add")
    ivf.add(xb[cut:])
    check(ivf, ivf.search(xq, 10), ref.search(xq, xb, ids, lists, c, 10, 3, L2), "second add")
    with pytest.raises(AssertionError):
        ivf.add_with_ids(xb[:3], ids[:3])
    ivf.reset()
    assert ivf.ntotal == 0 and ivf.is_trained and (ivf.list_sizes() == 0).all()
    D, I = ivf.search(xq, 3)
    assert (I == -1).all() and (D == ref.FLT_MAX).all()
    weird = ids * 3 - 7  # negative ids
    weird[5:10] = (1 << 40) + np.arange(5)  # above 2^32
    weird[20:30] = 12345  # duplicates
    ivf.add_with_ids(xb[:cut], weird[:cut])
    check(ivf, ivf.search(xq, 10), ref.search(xq, xb[:cut], weird[:cut], lists[:cut], c, 10, 3, L2), "add_with_ids")
    with pytest.raises(AssertionError):
        ivf.add(xb[:3])


@pytest.mark.stream_ordered
def test_device_tensors_in_and_out(fx, torch):
    d, dtype = 384, "bfloat16"
    c, xb, lists, xq = ref.edge_corpus(d, dtype)
    ivf = make_ivf(fx, c, L2, dtype)
    ivf.add(torch.from_numpy(np.array(xb)).to("cuda:0").bfloat16())
    ivf.nprobe = 3
    outs = []
    tq = torch.from_numpy(np.array(xq)).to("cuda:0")
    for k in (10, 40):
        D, I = ivf.search(tq, k)
        assert D.is_cuda and I.is_cuda and D.dtype == torch.float32 and I.dtype == torch.int64
        outs.append((k, D, I))
    for k, D, I in outs:
        want = ref.search(xq, xb, np.arange(xb.shape[0]), lists, c, k, 3, L2)
        check(ivf, (D.cpu().numpy(), I.cpu().numpy()), want, f"device k={k}")
        Dh, Ih = ivf.search(xq, k)
        assert (Ih == I.cpu().numpy()).all() and (Dh == D.cpu().numpy()).all()


def test_end_to_end_train_add_search(fx, tmp_path):
    x, _ = kref.blobs(3001, 100, 16, 1, 0)
    x = np.array(x)
    d, nlist = 100, 16
    ivf = fx.IndexIVFFlat(fx.IndexFlatL2(d), d, nlist)
    assert not ivf.is_trained
    with pytest.raises(AssertionError):
        ivf.add(x[:5])
    ivf.train(x)
    assert ivf.is_trained
    ivf.train(x)  # a no-op on a trained index
    assert ivf.quantizer.ntotal == nlist
    ivf.add(x)
    ivf.nprobe = 4
    xq = x[::97] + np.float32(0.01)
    c = ivf.quantizer.reconstruct_n(0, nlist)  # the centroids as stored
    lists = ref.assign(x, c, L2)
    want = ref.search(xq, x, np.arange(x.shape[0]), lists, c, 10, 4, L2)
    got = ivf.search(xq, 10)
    check(ivf, got, want, "end to end")
    # the training persists through the quantizer's file
    path = str(tmp_path / "quantizer.ixf2")
    fx.write_index(ivf.quantizer, path)
    ivf2 = fx.IndexIVFFlat(fx.read_index(path), d, nlist)
    assert ivf2.is_trained
    ivf2.add(x)
    ivf2.nprobe = 4
    D2, I2 = ivf2.search(xq, 10, params=fx.SearchParametersIVF(nprobe=4))
    assert ivf2.last_dropped_candidates() == 0
    assert (I2 == got[1]).all() and (D2 == got[0]).all()
    with pytest.raises(NotImplementedError):
        fx.write_index(ivf, path)


def test_store_consumer(fx, monkeypatch):
    from rag_faiss_embedding_amd import faiss_store
    x, _ = kref.blobs(2000, 100, 16, 7, 0)
    x = np.array(x)
    monkeypatch.setattr(faiss_store.FAISSVectorStore, "_instance", None)
    monkeypatch.setattr(faiss_store.FAISSVectorStore, "_initialized", False)
    store = faiss_store.FAISSVectorStore(dimension=100, index_path="/nonexistent/none.bin")
    doc_ids = [5000 + 3 * i for i in range(x.shape[0])]
    store.add_vectors(x, doc_ids)
    ivf = store.build_ivf(8)
    assert store.ivf is ivf and ivf.ntotal == 2000 and ivf.nprobe == 8
    c = ivf.quantizer.reconstruct_n(0, 8)
    lists = ref.assign(x, c, L2)
    for q in (x[3] + np.float32(0.02), x[1500] * np.float32(0.9)):
        D8, ids8 = store.search(q, 5, nprobe=8)  # every list probed: the flat search
        Df, idsf = store.search(q, 5)
        assert ids8 == idsf and (D8 == Df).all() and len(ids8) == 5
        D2, ids2 = store.search(q, 5, nprobe=2)
        Dr, Ir = ref.search(q.reshape(1, -1), x, np.arange(2000), lists, c, 5, 2, L2)
        assert ids2 == [doc_ids[r] for r in Ir[0]] and np.allclose(D2, Dr[0], rtol=1e-5, atol=0)
        assert ivf.last_dropped_candidates() == 0
    store.add_vectors(x[:1], [1])
    assert store.ivf is None
    assert store.search(x[0], 5, nprobe=2)[1] == []

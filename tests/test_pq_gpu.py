"""GPU checks of IndexPQ (fx_pq.hip through the C ABI and the Python layer)
against the numpy reference of tests/_pq_ref.py: the codec bitwise, training as
M direct k-means runs, every search with ids equal to the reference, distances
within 1e-5 * max(1, |D_ref|) and no dropped candidate.  The exact scan repairs
every query the refine cannot certify, so the fused-path tests also assert
``last_fallbacks() == 0`` wherever the model counts none: the gather scan and the
refine must have served those results themselves.  Codebooks are injected with
``pq.centroids = ...`` unless the test is about training."""
import numpy as np
import pytest

from tests import _pq_ref as R

pytestmark = pytest.mark.gpu

L2, IP = R.L2, R.IP
SHAPES = {16: 2, 64: 8, 96: 6}  # d -> M (dsub 8, 8, 16)


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


def check(ix, got, want, what):
    D, I = got
    Dr, Ir = want
    assert ix.last_dropped_candidates() == 0, f"{what}: dropped candidates"
    bad = np.flatnonzero((I != Ir).any(1))
    assert bad.size == 0, f"{what}: ids differ for queries {bad[:5]}: {I[bad[0]]} vs {Ir[bad[0]]}"
    err = np.abs(D.astype(np.float64) - Dr.astype(np.float64))
    assert (err <= 1e-5 * np.maximum(1.0, np.abs(Dr))).all(), f"{what}: distances off by {err.max()}"


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def built(fx, xb, M, metric=L2, mod=None, cents=None):
    """(index, centroids, decoded reference rows): centroids injected, xb added."""
    cents = R.sampled_centroids(xb, M) if cents is None else cents
    ix = (mod or fx).IndexPQ(xb.shape[1], M, 8, metric)
    ix.pq.centroids = cents
    ix.add(xb)
    return ix, cents, R.decode(R.encode(xb, cents), cents)


# ---------------------------------------------------------------------------
# codec
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["float32", "bfloat16", "float16"])
@pytest.mark.parametrize("d", sorted(SHAPES))
def test_codec_is_bitwise_the_reference(fx, torch, d, dt):
    M = SHAPES[d]
    r = np.random.default_rng(d)
    x = r.standard_normal((700, d)).astype(np.float32)
    tt = torch.from_numpy(x).to("cuda:0").to(getattr(torch, dt))
    x = tt.float().cpu().numpy()  # the values the device sees
    extra = (50.0 * x[:50]).astype(np.float32)  # rows far outside the codebook's range
    te = torch.from_numpy(extra).to("cuda:0").to(getattr(torch, dt))
    extra = te.float().cpu().numpy()
    cents = R.sampled_centroids(x, M)
    cents[:, 200] = cents[:, 5]  # two identical centroids per sub-quantizer: the lowest j wins
    ix = fx.IndexPQ(d, M)
    assert not ix.is_trained and ix.code_size == M and ix.pq.dsub == d // M
    ix.pq.centroids = cents
    assert ix.is_trained and (bits(ix.pq.centroids) == bits(cents.reshape(-1))).all()
    allx, allt = np.concatenate([x, extra]), torch.cat([tt, te])
    codes = R.encode(allx, cents)
    assert codes.shape == (750, M) and (codes == 5).any() and not (codes == 200).any()
    dev_codes = ix.sa_encode(allt)
    assert dev_codes.dtype == torch.uint8 and (dev_codes.cpu().numpy() == codes).all()
    assert (ix.sa_encode(allx) == codes).all()  # numpy in, numpy out
    dec = R.decode(codes, cents)
    assert (bits(ix.sa_decode(codes)) == bits(dec)).all()
    assert (bits(ix.sa_decode(dev_codes).cpu().numpy()) == bits(dec)).all()
    ix.add(allt)
    assert ix.ntotal == 750
    assert (ix.codes == codes).all() and (ix.get_codes(700, 50) == codes[700:]).all()
    assert (bits(ix.reconstruct_n(0, 750)) == bits(dec)).all()
    assert (bits(ix.reconstruct_n(700, 50)) == bits(dec[700:])).all()
    keys = np.array([749, 0, 3, 3, 128], dtype=np.int64)
    assert (bits(ix.reconstruct_batch(keys)) == bits(dec[keys])).all()
    assert (bits(ix.reconstruct(127)) == bits(dec[127])).all()
    dk = ix.reconstruct_batch(torch.tensor([5, 750, -1], device="cuda:0"))
    assert (bits(dk[0].cpu().numpy()) == bits(dec[5])).all() and bool(dk[1:].isnan().all())
    with pytest.raises(RuntimeError):
        ix.reconstruct_batch(np.array([750]))


def test_non_finite_centroids_are_refused(fx):
    ix = fx.IndexPQ(16, 2)
    cents = np.zeros((2, 256, 8), dtype=np.float32)
    cents[1, 7, 3] = np.inf
    with pytest.raises(RuntimeError, match="non-finite"):
        ix.pq.centroids = cents
    assert not ix.is_trained


# ---------------------------------------------------------------------------
# training
# ---------------------------------------------------------------------------
def test_training_is_m_direct_kmeans_runs(fx):
    r = np.random.default_rng(3)
    x = r.standard_normal((1000, 64)).astype(np.float32)
    ix = fx.IndexPQ(64, 8, niter=4, seed=77)
    ix.train(x)
    assert ix.is_trained
    got = ix.pq.centroids
    want = []
    for m in range(8):
        km = fx.Kmeans(8, 256, niter=4, seed=77)
        km.train(np.ascontiguousarray(x[:, 8 * m:8 * m + 8]))
        want.append(km.centroids)
    assert (bits(got) == bits(np.stack(want).reshape(-1))).all()
    again = fx.IndexPQ(64, 8, niter=4, seed=77)
    again.train(x)
    assert (bits(again.pq.centroids) == bits(got)).all()
    with pytest.raises(RuntimeError, match="fewer than"):
        fx.IndexPQ(64, 8).train(x[:200])
    # the trained index serves a search
    ix.add(x)
    dec = R.decode(R.encode(x, got.reshape(8, 256, 8)), got.reshape(8, 256, 8))
    check(ix, ix.search(x[:20], 5), R.search(x[:20], dec, 5), "trained")


# ---------------------------------------------------------------------------
# search
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [L2, IP], ids=["L2", "IP"])
@pytest.mark.parametrize("d", sorted(SHAPES) + [776])
def test_search_equals_the_reference(fx, torch, d, metric):
    """1300 + d rows (uneven splits, a ragged last tile), 150 queries (two query tiles); d = 776 = 97 *
    8 is a K that is no multiple of the 32-dimension stage."""
    M = SHAPES.get(d, 97)
    n = 1300 + d
    xb, xq = R.clustered(d, n, 150, seed=d)
    ix, cents, dec = built(fx, xb, M, metric)
    want = R.search(xq, dec, 100, metric)  # the top-k of any smaller k is its prefix
    xh, xl, shift, eps = R.prep(xq, metric, cents)
    codes = R.encode(xb, cents)
    keys = R.keys64(xh, xl, *R.image_rows(codes, cents), R.row_norms(codes, cents), metric).astype(np.float32)
    for k in (1, 10, 32):
        check(ix, ix.search(xq, k), (want[0][:, :k], want[1][:, :k]), f"d={d} k={k}")
        plan = ix.last_pq_plan()
        assert plan["path"] == "fused" and plan["qtiles"] == 2
        model = R.uncertified(keys, xq, dec, metric, shift, eps, k, plan["splits"])
        print(f"d={d} metric={metric} k={k}: {ix.last_fallbacks()} flagged, the model counts {model}")
        if model == 0:
            assert ix.last_fallbacks() == 0
    for k in (33, 100):
        check(ix, ix.search(xq, k), (want[0][:, :k], want[1][:, :k]), f"d={d} exact k={k}")
        assert ix.last_pq_plan()["path"] == "exact"
    check(ix, ix.search(xq[:1], 10), (want[0][:1, :10], want[1][:1, :10]), f"d={d} nq=1")
    # device tensors in and out
    tq = torch.from_numpy(xq).to("cuda:0")
    for k in (10, 33):
        D, I = ix.search(tq, k)
        assert D.is_cuda and I.dtype == torch.int64
        check(ix, (D.cpu().numpy(), I.cpu().numpy()), (want[0][:, :k], want[1][:, :k]), f"d={d} device k={k}")
    Dp, Ip = np.empty((150, 10), np.float32), np.empty((150, 10), np.int64)
    assert ix.search(xq, 10, D=Dp, I=Ip)[1] is Ip
    check(ix, (Dp, Ip), (want[0][:, :10], want[1][:, :10]), f"d={d} D= I=")
    with pytest.raises(NotImplementedError):
        ix.search(xq, 1025)


def test_lifecycle(fx):
    d, M = 64, 8
    xb, xq = R.clustered(d, 1500, 20, seed=5)
    cents = R.sampled_centroids(xb, M)
    ix = fx.IndexPQ(d, M)
    with pytest.raises(AssertionError):
        ix.search(xq, 3)
    from rag_faiss_embedding_amd import _lib
    assert _lib.lib.fx_pq_add(ix._h, 20, xq.ctypes.data, 0, 0) == -1 and "not trained" in _lib.last_error()
    ix.pq.centroids = cents
    D, I = ix.search(xq, 3)  # an empty index
    assert (I == -1).all() and (D == np.float32(3.4028234663852886e38)).all()
    dec = R.decode(R.encode(xb, cents), cents)
    ix.add(xb[:1000])
    check(ix, ix.search(xq, 10), R.search(xq, dec[:1000], 10), "first add")
    ix.add(xb[1000:])
    check(ix, ix.search(xq, 10), R.search(xq, dec, 10), "second add")
    assert _lib.lib.fx_pq_set_centroids(ix._h, cents.ctypes.data) == -1 and "holds" in _lib.last_error()
    ix.reset()
    assert ix.ntotal == 0 and ix.is_trained
    ix.add(xb[1000:])
    check(ix, ix.search(xq, 10), R.search(xq, dec[1000:], 10), "after reset")
    check(ix, ix.search(xq, 40), R.search(xq, dec[1000:], 40), "after reset, exact")


@pytest.mark.parametrize("metric", [L2, IP], ids=["L2", "IP"])
def test_rows_with_equal_codes_rank_by_row(fx, metric):
    """40 distinct codes each 50 times: k = 10 cuts through a block of exact ties."""
    d, M = 64, 8
    base, xq = R.clustered(d, 40, 12, seed=9, ncentres=40, spread=1.0)
    cents = R.sampled_centroids(base, M)
    xb = np.tile(base, (50, 1))  # row r repeats row r % 40
    ix, _, dec = built(fx, xb, M, metric, cents=cents)
    codes = ix.codes
    assert (codes == np.tile(codes[:40], (50, 1))).all()
    for k in (10, 32):
        want = R.search(xq, dec, k, metric)
        D, I = ix.search(xq, k)
        check(ix, (D, I), want, f"ties k={k}")
        first = I[:, 0]
        same = (codes[first][:, None, :] == codes[None, :, :]).all(2)  # the rows sharing the winner's code
        for q in range(len(xq)):
            assert (I[q, :10] == np.flatnonzero(same[q])[:10]).all() and (D[q, :10] == D[q, 0]).all()


def test_dsub_4_takes_the_exact_path(fx):
    xb, xq = R.clustered(32, 1400, 40, seed=4)
    ix, cents, dec = built(fx, xb, 8)
    assert ix.pq.dsub == 4
    for k in (1, 10, 33):
        check(ix, ix.search(xq, k), R.search(xq, dec, k), f"dsub=4 k={k}")
        assert ix.last_pq_plan()["path"] == "exact"
        assert ix.last_fallbacks() == 0


def test_forced_fallback_equals_unforced(fx, diag_fx, monkeypatch):
    xb, xq = R.clustered(64, 3000, 70, seed=12)
    cents = R.sampled_centroids(xb, 8)
    ix, _, dec = built(fx, xb, 8, mod=diag_fx, cents=cents)
    D0, I0 = ix.search(xq, 10)
    check(ix, (D0, I0), R.search(xq, dec, 10), "unforced")
    assert ix.last_pq_plan()["path"] == "fused"
    plain = ix.last_fallbacks()
    monkeypatch.setenv("FX_FORCE_FALLBACK", "1")  # (read when the index is created)
    forced, _, _ = built(fx, xb, 8, mod=diag_fx, cents=cents)
    monkeypatch.delenv("FX_FORCE_FALLBACK")
    D1, I1 = forced.search(xq, 10)
    assert forced.last_dropped_candidates() == 0
    assert forced.last_fallbacks() == xq.shape[0] and forced.last_exact_fallbacks() == xq.shape[0]
    print(f"unforced: {plain} of {len(xq)} queries flagged")
    assert (I0 == I1).all()
    assert (np.abs(D0.astype(np.float64) - D1) <= 1e-5 * np.maximum(1.0, np.abs(D0))).all()


def test_store_consumer(fx, monkeypatch):
    from rag_faiss_embedding_amd import faiss_store
    x, _ = R.clustered(64, 2000, 1, seed=13)
    monkeypatch.setattr(faiss_store.FAISSVectorStore, "_instance", None)
    monkeypatch.setattr(faiss_store.FAISSVectorStore, "_initialized", False)
    store = faiss_store.FAISSVectorStore(dimension=64, index_path="/nonexistent/none.bin")
    doc_ids = [5000 + 3 * i for i in range(x.shape[0])]
    store.add_vectors(x, doc_ids)
    pq = store.build_pq(8)
    assert store.pq is pq and pq.ntotal == 2000 and pq.code_size == 8
    direct = fx.IndexPQ(64, 8)
    direct.train(store.index)
    direct.add_from_index(store.index)
    assert (bits(direct.pq.centroids) == bits(pq.pq.centroids)).all() and (direct.codes == pq.codes).all()
    cents = pq.pq.centroids.reshape(8, 256, 8)
    dec = R.decode(R.encode(x, cents), cents)
    for q in (x[3] + np.float32(0.02), x[1500] * np.float32(0.9)):
        D, ids = store.search(q, 5, pq=True)
        Dd, Id = direct.search(q.reshape(1, -1), 5)
        assert ids == [doc_ids[i] for i in Id[0]] and (bits(D) == bits(Dd[0])).all()
        Dr, Ir = R.search(q.reshape(1, -1), dec, 5)
        assert ids == [doc_ids[i] for i in Ir[0]] and np.allclose(D, Dr[0], rtol=1e-5, atol=0)
        assert pq.last_dropped_candidates() == 0
    store.add_vectors(x[:1], [1])
    assert store.pq is None
    assert store.search(x[0], 5, pq=True)[1] == []

"""GPU checks of IndexScalarQuantizer (fx_sq.hip through the C ABI and the
Python layer) against the numpy reference of tests/_sq_ref.py: the codec
bitwise, every search with ids equal to the reference, distances within 1e-5 *
max(1, |D_ref|) and no dropped candidate.  The exact scan repairs every query
the refine cannot certify, so the fused-path test also asserts
``last_fallbacks() == 0``: the int8 MFMA scan and the refine must have served
those results themselves."""
import numpy as np
import pytest

from tests import _sq_ref as R

pytestmark = pytest.mark.gpu

L2, IP = 1, 0
FLT_MAX = np.float32(3.4028234663852886e38)


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


def built(fx, xb, metric=L2, qtype=R.QT_8bit, train=None, mod=None):
    """(index, decoded reference rows): trained on `train` (default xb), xb added."""
    ix = (mod or fx).IndexScalarQuantizer(xb.shape[1], qtype, metric)
    ix.train(xb if train is None else train)
    ix.add(xb)
    tr = R.train(xb if train is None else train, qtype)
    return ix, R.decode(R.encode(xb, tr), tr)


# ---------------------------------------------------------------------------
# codec
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("qtype", [R.QT_8bit, R.QT_8bit_uniform], ids=["8bit", "uniform"])
@pytest.mark.parametrize("dt", ["float32", "bfloat16", "float16"])
@pytest.mark.parametrize("d", [20, 100, 384])
def test_codec_is_bitwise_the_reference(fx, torch, d, dt, qtype):
    r = np.random.default_rng(d)
    x = r.standard_normal((700, d)).astype(np.float32)
    x[:, 3] = 0.25  # a constant dimension: vdiff = 0
    tt = torch.from_numpy(x).to("cuda:0").to(getattr(torch, dt))
    x = tt.float().cpu().numpy()  # the values the device sees
    extra = (3.0 * x[:50]).astype(np.float32)  # rows outside the trained range: clamped
    te = torch.from_numpy(extra).to("cuda:0").to(getattr(torch, dt))
    extra = te.float().cpu().numpy()
    ix = fx.IndexScalarQuantizer(d, qtype)
    assert not ix.is_trained and ix.code_size == d
    ix.train(tt)
    assert ix.is_trained
    tr = R.train(x, qtype)
    got = ix.trained
    want = tr if qtype == R.QT_8bit else np.array([tr[0], tr[d]], dtype=np.float32)
    assert got.shape == want.shape and (got == want).all()
    if qtype == R.QT_8bit:
        assert tr[d + 3] == 0
    allx, allt = np.concatenate([x, extra]), torch.cat([tt, te])
    codes = R.encode(allx, tr)
    assert (codes[:, 3] == 0).all() or qtype == R.QT_8bit_uniform
    assert codes.min() == 0 and codes.max() == 255
    dev_codes = ix.sa_encode(allt)
    assert dev_codes.dtype == torch.uint8 and (dev_codes.cpu().numpy() == codes).all()
    assert (ix.sa_encode(allx) == codes).all()  # numpy in, numpy out
    dec = R.decode(codes, tr)
    assert (bits(ix.sa_decode(codes)) == bits(dec)).all()
    assert (bits(ix.sa_decode(dev_codes).cpu().numpy()) == bits(dec)).all()
    ix.add(allt)
    assert ix.ntotal == 750
    assert (bits(ix.reconstruct_n(0, 750)) == bits(dec)).all()
    assert (bits(ix.reconstruct_n(700, 50)) == bits(dec[700:])).all()
    keys = np.array([749, 0, 3, 3, 128], dtype=np.int64)
    assert (bits(ix.reconstruct_batch(keys)) == bits(dec[keys])).all()
    assert (bits(ix.reconstruct(127)) == bits(dec[127])).all()
    dk = ix.reconstruct_batch(torch.tensor([5, 750, -1], device="cuda:0"))
    assert (bits(dk[0].cpu().numpy()) == bits(dec[5])).all() and bool(dk[1:].isnan().all())
    with pytest.raises(RuntimeError):
        ix.reconstruct_batch(np.array([750]))
    # the training kept with numpy makes a second index that returns identical codes
    ix2 = fx.IndexScalarQuantizer(d, qtype)
    ix2.set_trained(got)
    assert ix2.is_trained and (ix2.trained == got).all()
    assert (ix2.sa_encode(allx) == codes).all()
    ix2.add(allx)
    assert (bits(ix2.reconstruct_n()) == bits(dec)).all()


def test_non_finite_training_data_fails(fx):
    x = np.zeros((10, 20), dtype=np.float32)
    x[4, 7] = np.inf
    ix = fx.IndexScalarQuantizer(20)
    with pytest.raises(RuntimeError, match="non-finite"):
        ix.train(x)
    assert not ix.is_trained
    ix.train(np.nan_to_num(x, posinf=1.0))
    assert ix.is_trained


# ---------------------------------------------------------------------------
# search
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [L2, IP], ids=["L2", "IP"])
@pytest.mark.parametrize("d", [20, 100, 384, 768, 1100])
def test_edges(fx, d, metric):
    """The smallest shapes that cross a tile edge on rows, on queries and in the
    padded k dimension.  (d = 1100 is past the width from which an accumulator can pass its
    exact fp32 range, but these standard normal rows stay 36 times short of 2^24; the corner case
    of tests/test_sq_scan_parity.py gets there.)"""
    r = np.random.default_rng(100 + d)
    xall = r.standard_normal((1000, d)).astype(np.float32)
    xq = r.standard_normal((300, d)).astype(np.float32)
    tr = R.train(xall)
    ix = fx.IndexScalarQuantizer(d, R.QT_8bit, metric)
    ix.train(xall)
    for ntotal in (1, 127, 128, 129, 1000):
        ix.reset()
        ix.add(xall[:ntotal])
        assert ix.ntotal == ntotal
        dec = R.decode(R.encode(xall[:ntotal], tr), tr)
        Dr, Ir = R.search(xq, dec, 32, metric)  # the top-k of any smaller k is its prefix
        if ntotal < 32:
            assert (Ir[:, ntotal:] == -1).all() and (np.abs(Dr[:, ntotal:]) == FLT_MAX).all()
        for nq in (1, 37, 129, 300):
            for k in (1, 10, 32):
                got = ix.search(xq[:nq], k)
                check(ix, got, (Dr[:nq, :k], Ir[:nq, :k]), f"d={d} ntotal={ntotal} nq={nq} k={k}")
                assert ix.last_sq_plan()["path"] == "fused"
                if ntotal == 1000:
                    # reported only: the data is unclustered, and which queries may be flagged is the
                    # model's to say (flag parity, tests/test_sq_scan_parity.py)
                    print(f"d={d} {'L2' if metric == L2 else 'IP'} ntotal=1000 nq={nq} k={k}: "
                          f"{ix.last_fallbacks()} queries flagged")


@pytest.fixture(scope="module")
def corpus01():
    return R.clustered(0.1)


def test_splits_and_passes(fx, corpus01):
    xb, xq = corpus01
    more = xq[:44] + xq[1:45]
    xq300 = np.concatenate([xq, more / np.linalg.norm(more, axis=1, keepdims=True)]).astype(np.float32)
    ix, dec = built(fx, xb)
    want = R.search(xq300, dec, 10)
    check(ix, ix.search(xq300[:1], 10), (want[0][:1], want[1][:1]), "nq=1")
    plan = ix.last_sq_plan()
    assert plan["splits"] > 1 and plan["grid"] == plan["splits"], plan
    check(ix, ix.search(xq300, 10), want, "nq=300")
    assert ix.last_sq_plan()["qtiles"] == 3


@pytest.mark.parametrize("spread", [0.1, 0.02])
def test_fused_path_serves_itself(fx, corpus01, spread):
    xb, xq = corpus01 if spread == 0.1 else R.clustered(0.02)
    ix, dec = built(fx, xb)
    want = R.search(xq, dec, 10)
    for k in (1, 10):
        check(ix, ix.search(xq, k), (want[0][:, :k], want[1][:, :k]), f"spread {spread} k={k}")
        assert ix.last_sq_plan()["path"] == "fused"
        print(f"spread {spread} k={k}: {ix.last_fallbacks()} of {len(xq)} queries flagged")
        if spread == 0.1:
            assert ix.last_fallbacks() == 0, f"k={k}: flagged queries"


@pytest.mark.parametrize("metric", [L2, IP], ids=["L2", "IP"])
def test_exact_path_big_k(fx, metric):
    r = np.random.default_rng(7)
    xb = r.standard_normal((1000, 100)).astype(np.float32)
    xq = r.standard_normal((37, 100)).astype(np.float32)
    ix, dec = built(fx, xb, metric)
    for k in (33, 100, 1024):
        want = R.search(xq, dec, k, metric)
        check(ix, ix.search(xq, k), want, f"exact k={k}")
        assert ix.last_sq_plan()["path"] == "exact"
    assert (want[1][:, 1000:] == -1).all(), "k = 1024 pads"
    with pytest.raises(NotImplementedError):
        ix.search(xq, 1025)


def test_forced_fallback_equals_unforced(fx, diag_fx, monkeypatch):
    r = np.random.default_rng(9)
    xb = r.standard_normal((3000, 384)).astype(np.float32)
    xq = r.standard_normal((70, 384)).astype(np.float32)
    ix, dec = built(fx, xb, mod=diag_fx)
    D0, I0 = ix.search(xq, 10)
    check(ix, (D0, I0), R.search(xq, dec, 10), "unforced")
    plain = ix.last_fallbacks()
    monkeypatch.setenv("FX_FORCE_FALLBACK", "1")  # (read when the index is created)
    forced, _ = built(fx, xb, mod=diag_fx)
    monkeypatch.delenv("FX_FORCE_FALLBACK")
    D1, I1 = forced.search(xq, 10)
    assert forced.last_dropped_candidates() == 0
    assert forced.last_fallbacks() == xq.shape[0] and forced.last_exact_fallbacks() == xq.shape[0] and plain == 0
    assert (I0 == I1).all() and (bits(D0) == bits(D1)).all()


def test_ties_order_by_distance_then_row(fx):
    d = 20
    r = np.random.default_rng(2)
    base = r.integers(-3, 4, size=(40, d)).astype(np.float32)  # integer-grid rows
    base = np.unique(base, axis=0)
    base = base[r.permutation(base.shape[0])]
    xb = np.repeat(base, 2, axis=0)  # every row twice: equal codes, equal distances
    xq = r.integers(-3, 4, size=(6, d)).astype(np.float32)
    for metric in (L2, IP):
        ix, dec = built(fx, xb, metric)
        for k in (5, 32):
            want = R.search(xq, dec, k, metric)
            assert (want[0][:, 0] == want[0][:, 1]).all()
            check(ix, ix.search(xq, k), want, f"ties metric={metric} k={k}")


def test_equals_the_flat_index_on_decoded_rows(fx):
    n, d, k = 5000, 384, 10
    r = np.random.default_rng(21)
    xb = r.standard_normal((n, d)).astype(np.float32)
    xq = r.standard_normal((64, d)).astype(np.float32)
    ix, _ = built(fx, xb)
    flat = fx.IndexFlatL2(d)
    flat.add(ix.reconstruct_n(0, n))
    Df, If = flat.search(xq, k + 1)
    assert (Df[:, 1:] != Df[:, :-1]).all(), "the flat result has tied distances in its top 11"
    D, I = ix.search(xq, k)
    assert ix.last_dropped_candidates() == 0
    assert (I == If[:, :k]).all()
    assert (bits(D) == bits(Df[:, :k])).all()


def test_lifecycle(fx):
    r = np.random.default_rng(5)
    xb = r.standard_normal((1500, 100)).astype(np.float32)
    xq = r.standard_normal((20, 100)).astype(np.float32)
    ix = fx.IndexScalarQuantizer(100)
    with pytest.raises(AssertionError):
        ix.search(xq, 3)
    with pytest.raises(AssertionError):
        ix.add(xb)
    # the library itself refuses too
    from rag_faiss_embedding_amd import _lib
    D, I = np.empty((20, 3), np.float32), np.empty((20, 3), np.int64)
    assert _lib.lib.fx_sq_search(ix._h, 20, xq.ctypes.data, 0, 0, 3, D.ctypes.data, I.ctypes.data, 0) == -1
    assert "not trained" in _lib.last_error()
    assert _lib.lib.fx_sq_add(ix._h, 20, xq.ctypes.data, 0, 0) == -1
    ix.train(xb)
    tr = R.train(xb)
    D, I = ix.search(xq, 3)  # an empty index
    assert (I == -1).all() and (D == FLT_MAX).all()
    cut = 1000
    ix.add(xb[:cut])
    dec = R.decode(R.encode(xb, tr), tr)
    check(ix, ix.search(xq, 10), R.search(xq, dec[:cut], 10), "first add")
    ix.add(xb[cut:])
    check(ix, ix.search(xq, 10), R.search(xq, dec, 10), "second add")
    with pytest.raises(AssertionError):
        ix.train(xb)
    assert _lib.lib.fx_sq_train(ix._h, 20, xq.ctypes.data, 0, 0, 0) == -1 and "holds" in _lib.last_error()
    ix.reset()
    assert ix.ntotal == 0 and ix.is_trained and (ix.trained == tr).all()
    ix.add(xb[cut:])
    check(ix, ix.search(xq, 10), R.search(xq, dec[cut:], 10), "after reset")


@pytest.mark.stream_ordered
def test_device_tensors_in_and_out(fx, torch):
    r = np.random.default_rng(11)
    xb = r.standard_normal((3000, 384)).astype(np.float32)
    xq = r.standard_normal((150, 384)).astype(np.float32)
    ix = fx.IndexScalarQuantizer(384)
    tb = torch.from_numpy(xb).to("cuda:0")
    ix.train(tb)
    ix.add(tb)
    tr = R.train(xb)
    dec = R.decode(R.encode(xb, tr), tr)
    tq = torch.from_numpy(xq).to("cuda:0")
    outs = []
    for k in (10, 40):
        D, I = ix.search(tq, k)
        assert D.is_cuda and I.is_cuda and D.dtype == torch.float32 and I.dtype == torch.int64
        outs.append((k, D, I))
    for k, D, I in outs:
        check(ix, (D.cpu().numpy(), I.cpu().numpy()), R.search(xq, dec, k), f"device k={k}")
        Dh, Ih = ix.search(xq, k)
        assert (Ih == I.cpu().numpy()).all() and (bits(Dh) == bits(D.cpu().numpy())).all()


def test_store_consumer(fx, monkeypatch):
    from rag_faiss_embedding_amd import faiss_store
    r = np.random.default_rng(13)
    x = r.standard_normal((2000, 100)).astype(np.float32)
    monkeypatch.setattr(faiss_store.FAISSVectorStore, "_instance", None)
    monkeypatch.setattr(faiss_store.FAISSVectorStore, "_initialized", False)
    store = faiss_store.FAISSVectorStore(dimension=100, index_path="/nonexistent/none.bin")
    doc_ids = [5000 + 3 * i for i in range(x.shape[0])]
    store.add_vectors(x, doc_ids)
    sq = store.build_sq()
    assert store.sq is sq and sq.ntotal == 2000
    tr = R.train(x)
    assert (sq.trained == tr).all()
    dec = R.decode(R.encode(x, tr), tr)
    for q in (x[3] + np.float32(0.02), x[1500] * np.float32(0.9)):
        D, ids = store.search(q, 5, sq=True)
        Dr, Ir = R.search(q.reshape(1, -1), dec, 5)
        assert ids == [doc_ids[i] for i in Ir[0]] and np.allclose(D, Dr[0], rtol=1e-5, atol=0)
        assert sq.last_dropped_candidates() == 0
    store.add_vectors(x[:1], [1])
    assert store.sq is None
    assert store.search(x[0], 5, sq=True)[1] == []

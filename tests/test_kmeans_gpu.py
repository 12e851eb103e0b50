"""GPU checks of Kmeans (fx_kmeans.hip through the C ABI and the Python layers)
against the numpy reference step of tests/_kmeans_ref.py.

Every comparison first asserts, on the reference alone, that no point's
nearest and second-nearest centroid are closer than 5e-7 relative (more than
four fp32 ulps): rounding cannot decide an assignment, so assignments, counts
and repairs must be identical, centroids agree within one fp32 rounding of two
fp64 sums that differ by summation order, and objectives within 1e-6.

The multi-iteration test checks the identity of every point's assignment: it
does not use the allowance for points whose reference gap is below 1e-5.  (The
issue's cap on such points, 0.1 % of n, does not hold on the reference for
the 1000 x 20 and 2500 x 768 shapes: in the iteration after a repair the two
halves of a split cluster are nearly equidistant, 11 and 8 points.)"""
import ctypes

import numpy as np
import pytest

from tests import _kmeans_ref as ref

pytestmark = pytest.mark.gpu

DTYPES = ["float32", "bfloat16", "float16"]
SHAPE_IDS = ["3001x100", "3001x100-far2", "4097x384", "1000x20-far1", "2500x768-far3"]
NITER = 5


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


def dev(torch, x, dtype="float32"):
    return torch.from_numpy(np.array(x, dtype=np.float32)).to("cuda:0").to(getattr(torch, dtype))


def kmeans(fx, shape, **kw):
    _, d, k, _, _ = shape
    # (every row trains: no subsampling at n > 256 k, no warning below 39 k)
    return fx.Kmeans(d, k, min_points_per_centroid=1, max_points_per_centroid=1 << 20, **kw)


@pytest.fixture(scope="module")
def ref_runs():
    """(shape, dtype) -> the reference's NITER steps from the initial centroids, computed once."""
    cache = {}

    def get(shape, dtype):
        if (shape, dtype) not in cache:
            x, init = ref.case(shape, dtype)
            c, steps = np.array(init), []
            for _ in range(NITER):
                steps.append(ref.lloyd_step(x, c))
                c = steps[-1]["centroids"]
            cache[shape, dtype] = steps
        return cache[shape, dtype]
    return get


def check_step(km, s, x, what):
    assert (km.counts == s["counts"]).all(), f"{what}: counts differ"
    assert km.iteration_stats[-1]["nsplit"] == s["nsplit"], f"{what}: nsplit"
    err = np.abs(km.centroids.astype(np.float64) - s["centroids"].astype(np.float64))
    tol = ref.centroid_tol(s["centroids"].astype(np.float64), x)
    print(f"{what}: max centroid error / tolerance {float((err / tol).max()):.3g}, "
          f"obj {km.obj[-1]!r} vs {s['obj']!r}, nsplit {s['nsplit']}")
    assert (err <= tol).all(), f"{what}: centroids off by up to {float((err / tol).max()):.3g} x the tolerance"
    assert abs(km.obj[-1] - s["obj"]) <= 1e-6 * abs(s["obj"]), f"{what}: obj {km.obj[-1]} vs {s['obj']}"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", ref.SHAPES, ids=SHAPE_IDS)
def test_stepwise_parity(fx, torch, shape, dtype):
    """One library step and one reference step from the same centroids, 5 times."""
    x, init = ref.case(shape, dtype)
    xt = dev(torch, x, dtype)
    c_prev = np.array(init)
    ix = fx.IndexFlatL2(shape[1])
    ix.add(c_prev)
    a_lib = ix.search(xt, 1)[1].reshape(-1).cpu().numpy()  # the assignment under the initial centroids
    for it in range(NITER):
        s = ref.lloyd_step(x, c_prev)
        assert s["gap"].min() >= ref.MIN_GAP, f"iteration {it}: reference gap {s['gap'].min():.3g}: change the seed"
        assert (a_lib == s["assign"]).all(), f"iteration {it}: {(a_lib != s['assign']).sum()} assignments differ"
        km = kmeans(fx, shape, niter=1)
        km.train(xt, init_centroids=c_prev)
        check_step(km, s, x, f"iteration {it}")
        a_lib = km.assign(xt)[1].cpu().numpy()
        c_prev = km.centroids
    assert km.index.ntotal == shape[2] and km.index.metric_type == fx.METRIC_L2


@pytest.mark.parametrize("shape,dtype", [(s, "float32") for s in ref.SHAPES] +
                         [(ref.SHAPES[1], "bfloat16"), (ref.SHAPES[1], "float16"), (ref.SHAPES[4], "bfloat16")],
                         ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v[:3])))
def test_multi_iteration_parity(fx, torch, ref_runs, shape, dtype):
    x, init = ref.case(shape, dtype)
    steps = ref_runs(shape, dtype)
    for it, s in enumerate(steps):
        assert s["gap"].min() >= ref.MIN_GAP, f"iteration {it}: reference gap {s['gap'].min():.3g}: change the seed"
    xt = dev(torch, x, dtype)
    km = kmeans(fx, shape, niter=NITER)
    final = km.train(xt, init_centroids=init)
    assert km.obj.shape == (NITER,) and final == km.obj[-1] and len(km.iteration_stats) == NITER
    assert [st["nsplit"] for st in km.iteration_stats] == [s["nsplit"] for s in steps]
    for it, s in enumerate(steps):
        assert abs(km.obj[it] - s["obj"]) <= 1e-6 * abs(s["obj"]), f"iteration {it}: obj {km.obj[it]} vs {s['obj']}"
    check_step(km, steps[-1], x, "after 5 iterations")
    # the assignment under the final centroids: every point
    a_ref, _, gap = ref.assign(x, steps[-1]["centroids"])
    assert gap.min() >= ref.MIN_GAP
    D, I = km.assign(xt)
    assert D.dim() == 1 and I.dim() == 1
    assert (I.cpu().numpy() == a_ref).all()


@pytest.mark.parametrize("shape,dtype", [(ref.SHAPES[1], d) for d in DTYPES] + [(ref.SHAPES[4], "bfloat16")],
                         ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v[:3])))
def test_determinism_and_chunking(fx, torch, shape, dtype):
    x, init = ref.case(shape, dtype)
    xt = dev(torch, x, dtype)

    def run(chunk):
        km = kmeans(fx, shape, niter=3)
        km.kmeans_chunk = chunk
        km.train(xt, init_centroids=init)
        return km
    a, b = run(0), run(0)
    assert a.centroids.tobytes() == b.centroids.tobytes() and a.obj.tobytes() == b.obj.tobytes()
    chunk = shape[0] // 3 - 1  # at least 3 chunks (4: the last one short)
    c, d = run(chunk), run(chunk)
    assert c.centroids.tobytes() == d.centroids.tobytes() and c.obj.tobytes() == d.obj.tobytes()
    assert (c.counts == a.counts).all()
    assert [s["nsplit"] for s in c.iteration_stats] == [s["nsplit"] for s in a.iteration_stats]
    err = np.abs(c.centroids.astype(np.float64) - a.centroids.astype(np.float64))
    assert (err <= ref.centroid_tol(a.centroids.astype(np.float64), x)).all()
    assert np.abs(c.obj - a.obj).max() <= 1e-6 * np.abs(a.obj).max()


class Abi:
    """The update ABI on a k-row fp32 centroid index, over torch buffers."""

    def __init__(self, fx, torch, k, d):
        from rag_faiss_embedding_amd import _lib
        self.lib, self._lib, self.torch = _lib.lib, _lib, torch
        self.ix = fx.IndexFlatL2(d)
        self.ix.add(np.zeros((k, d), dtype=np.float32))
        self.ix._bind_stream(True)
        self.sums = torch.full((k, d), float("nan"), dtype=torch.float64, device="cuda:0")
        self.counts = torch.full((k,), -7, dtype=torch.int64, device="cuda:0")
        self.obj = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda:0")

    def update(self, x, assign, dist=None, accumulate=0, host=False):
        p = lambda a: None if a is None else ctypes.c_void_p(a.data_ptr())  # noqa: E731
        code = {self.torch.float32: 0, self.torch.bfloat16: 1, self.torch.float16: 2}[x.dtype]
        xp, mem = p(x), self._lib.MEM_DEVICE
        if host:
            xh = x.float().cpu().numpy()
            xp, mem, code = ctypes.c_void_p(xh.ctypes.data), self._lib.MEM_HOST, 0
        return self.lib.fx_kmeans_update(self.ix._h, x.shape[0], xp, code, mem, p(assign), p(dist), p(self.sums),
                                         p(self.counts), p(self.obj), accumulate)

    def status(self):
        bad = ctypes.c_int64(-1)
        return self.lib.fx_kmeans_status(self.ix._h, ctypes.byref(bad)), bad.value


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_row_in_one_cluster(fx, torch, dtype):
    """1000 rows of 20 (40- and 80-B rows: element loads for the 16-bit ones)
    in cluster 1 of 3: 8 member blocks folded in order."""
    x, _ = ref.case(ref.SHAPES[3], dtype)
    xt = dev(torch, x, dtype)
    abi = Abi(fx, torch, 3, 20)
    assign = torch.ones(1000, dtype=torch.int64, device="cuda:0")
    dist = torch.arange(1000, dtype=torch.float32, device="cuda:0")
    assert abi.update(xt, assign, dist) == 0
    assert abi.status() == (0, 0)
    assert abi.counts.tolist() == [0, 1000, 0]
    sums = abi.sums.cpu().numpy()
    want = x.astype(np.float64).sum(0)
    assert (sums[0] == 0).all() and (sums[2] == 0).all()
    assert np.abs(sums[1] - want).max() <= 1e-12 * np.abs(x).sum(0).max()
    assert abi.obj.item() == 999 * 1000 / 2
    # a second chunk accumulates
    assert abi.update(xt, assign * 2, dist, accumulate=1) == 0
    assert abi.counts.tolist() == [0, 1000, 1000] and abi.obj.item() == 999 * 1000
    assert (abi.sums[2] == abi.sums[1]).all()


@pytest.mark.parametrize("dtype,d", [("float32", 384), ("bfloat16", 384), ("float16", 100), ("float32", 2052)])
def test_one_row_per_cluster(fx, torch, dtype, d):
    """Sums of one row are the row, bit for bit (d = 2052 fp32: more 16-B slices than a workgroup has lanes)."""
    k = 130
    r = np.random.default_rng(11)
    x = ref.round_to(r.standard_normal((k, d)).astype(np.float32), dtype)
    perm = r.permutation(k)
    abi = Abi(fx, torch, k, d)
    assert abi.update(dev(torch, x, dtype), torch.from_numpy(perm).to("cuda:0")) == 0
    assert abi.status() == (0, 0)
    assert (abi.counts == 1).all() and abi.obj.item() == 0
    sums = abi.sums.cpu().numpy()
    assert (sums[perm] == x.astype(np.float64)).all()


@pytest.mark.parametrize("host", [False, True], ids=["device-x", "host-x"])
def test_invalid_assignments_are_an_integrity_error(fx, torch, host):
    """Argument validation: an assignment of -1 (a padded search's) or k names
    no cluster; it is counted, the call fails with FX_E_INTEGRITY, and the
    valid rows are summed as if the entry were not there."""
    x, _ = ref.case(ref.SHAPES[3])
    k = 3
    a = np.random.default_rng(5).integers(0, k, 1000)
    a[17], a[900] = -1, k
    abi = Abi(fx, torch, k, 20)
    rc = abi.update(dev(torch, x), torch.from_numpy(a).to("cuda:0"), host=host)
    if host:
        assert rc == -6 and "outside [0, 3)" in abi._lib.last_error()
        assert abi.status() == (0, 0)  # (read and reset by the failed call)
    else:
        assert rc == 0
        assert abi.status() == (-6, 2)
        assert abi.status() == (0, 0)
    sums, counts = abi.sums.cpu().numpy(), abi.counts.cpu().numpy()
    assert np.isfinite(sums).all()
    valid = (a >= 0) & (a < k)
    assert (counts == np.bincount(a[valid], minlength=k)).all() and counts.sum() == 998
    for c in range(k):
        want = x[valid & (a == c)].astype(np.float64).sum(0)
        assert np.abs(sums[c] - want).max() <= 1e-12 * np.abs(x).sum(0).max()


def test_abi_codes_on_a_live_index(fx, torch):
    abi = Abi(fx, torch, 3, 20)
    x = torch.zeros((4, 20), device="cuda:0")
    a = torch.zeros(4, dtype=torch.int64, device="cuda:0")
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    lib, h = abi.lib, abi.ix._h
    assert lib.fx_kmeans_step(h, 0, None, 0, 1, None, None, p(abi.sums), p(abi.counts), p(abi.obj), 0) == 0  # n == 0
    assert torch.isnan(abi.sums).all()                                                                       # ... changes nothing
    assert lib.fx_kmeans_step(h, 4, None, 0, 1, None, None, p(abi.sums), p(abi.counts), p(abi.obj), 0) == -1
    empty = fx.IndexFlatL2(20)
    assert lib.fx_kmeans_step(empty._h, 4, p(x), 0, 1, None, None, p(abi.sums), p(abi.counts), p(abi.obj), 0) == -1
    assert "empty" in abi._lib.last_error()
    off = fx.IndexFlatL2(20)
    off.add(np.zeros((3, 20), dtype=np.float32))
    off.set_id_offset(5)
    assert lib.fx_kmeans_update(off._h, 4, p(x), 0, 1, p(a), None, p(abi.sums), p(abi.counts), p(abi.obj), 0) == -4
    lab = fx.IndexIDMap(fx.IndexFlatL2(20))
    lab.add_with_ids(np.zeros((3, 20), dtype=np.float32), np.arange(3) + 10)
    cent = torch.zeros((3, 20), device="cuda:0")
    ns = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    assert lib.fx_kmeans_finish(lab.index._h, p(abi.sums), p(abi.counts), 0, p(cent), p(ns)) == -4
    with pytest.raises(RuntimeError):
        abi.ix.set_option("kmeans_chunk", -1)
    abi.ix.set_option("kmeans_chunk", 1 << 30)


@pytest.mark.parametrize("dtype", DTYPES)
def test_spherical(fx, torch, dtype):
    x, _ = ref.case(ref.SHAPES[0])
    x = ref.round_to(x / np.linalg.norm(x.astype(np.float64), axis=1, keepdims=True).astype(np.float32), dtype)
    xt = dev(torch, x, dtype)
    km = kmeans(fx, ref.SHAPES[0], niter=4, spherical=True, seed=3)
    km.train(xt)
    assert km.index.metric_type == fx.METRIC_INNER_PRODUCT
    norms = np.linalg.norm(km.centroids.astype(np.float64), axis=1)
    assert np.abs(norms - 1).max() <= 1e-6
    a_ref, d_ref, gap = ref.assign(x, km.centroids, spherical=True)
    assert gap.min() >= ref.MIN_GAP, f"reference gap {gap.min():.3g}: change the seed"
    D, I = km.assign(xt)
    assert (I.cpu().numpy() == a_ref).all()
    # the objective is the sum of the inner products of the last iteration's assignment: it grows
    assert km.obj[-1] >= km.obj[0] and km.obj[-1] <= shape_n(ref.SHAPES[0]) * (1 + 1e-2)
    # the initial centroids are the seeded rows of the training set
    km0 = kmeans(fx, ref.SHAPES[0], niter=0, spherical=True, seed=3)
    km0.train(xt)
    assert (km0.centroids == x[km0._init_rows(x.shape[0])]).all()


def shape_n(shape):
    return shape[0]


def test_index_as_training_set_and_store_cluster(fx, torch, monkeypatch):
    from rag_faiss_embedding_amd import faiss_store
    shape = ref.SHAPES[2]
    x, init = ref.case(shape, "bfloat16")
    xt = dev(torch, x, "bfloat16")
    ix = fx.IndexFlatL2(shape[1], dtype="bfloat16")
    ix.add(xt)
    a, b = kmeans(fx, shape, niter=3), kmeans(fx, shape, niter=3)
    a.train(ix)
    b.train(xt)
    assert a.centroids.tobytes() == b.centroids.tobytes() and a.obj.tobytes() == b.obj.tobytes()
    Da, Ia = a.assign(ix)
    Db, Ib = b.assign(xt)
    assert isinstance(Ia, np.ndarray) and Ia.shape == (shape[0],)
    assert (Ia == Ib.cpu().numpy()).all() and (Da == Db.cpu().numpy()).all()
    # chunked gather (3 chunks) against the chunked tensor path: the same bits
    a.kmeans_chunk = b.kmeans_chunk = 1500
    a.train(ix, init_centroids=init)
    b.train(xt, init_centroids=init)
    assert a.centroids.tobytes() == b.centroids.tobytes() and a.obj.tobytes() == b.obj.tobytes()
    assert (a.assign(ix)[1] == b.assign(xt)[1].cpu().numpy()).all()
    # an IndexIDMap around the same rows trains the same
    lab = fx.IndexIDMap(fx.IndexFlatL2(shape[1], dtype="bfloat16"))
    lab.add_with_ids(xt, torch.arange(shape[0], device="cuda:0") * 3 - 5)
    c = kmeans(fx, shape, niter=3)
    c.kmeans_chunk = 1500
    c.train(lab, init_centroids=init)
    assert c.centroids.tobytes() == a.centroids.tobytes()
    # the store's consumer
    monkeypatch.setattr(faiss_store.FAISSVectorStore, "_instance", None)
    monkeypatch.setattr(faiss_store.FAISSVectorStore, "_initialized", False)
    store = faiss_store.FAISSVectorStore(dimension=shape[1], index_path="/nonexistent/none.bin", dtype="bfloat16")
    store.index.add(xt)
    cents, labels = store.cluster(shape[2], niter=3)
    km = fx.Kmeans(shape[1], shape[2], niter=3)
    with pytest.warns(RuntimeWarning):
        km.train(store.index)
    assert cents.tobytes() == km.centroids.tobytes()
    assert labels.dtype == np.int64 and (labels == km.assign(store.index)[1]).all()
    assert (labels == km.assign(xt)[1].cpu().numpy()).all()


def test_device_in_makes_no_host_copy(fx, torch, monkeypatch):
    """A device tensor trains in place: every step is handed the tensor's own
    device pointer, and the results come back as documented."""
    from rag_faiss_embedding_amd import _lib
    shape = ref.SHAPES[0]
    x, init = ref.case(shape, "float16")
    xt = dev(torch, x, "float16")
    calls = []
    real = _lib.lib.fx_kmeans_step

    def spy(h, n, xp, code, mem, *rest):
        calls.append((n, xp.value, code, mem))
        return real(h, n, xp, code, mem, *rest)
    monkeypatch.setattr(_lib.lib, "fx_kmeans_step", spy)
    km = kmeans(fx, shape, niter=2)
    final = km.train(xt, init_centroids=init)
    assert calls == [(shape[0], xt.data_ptr(), _lib.F16, _lib.MEM_DEVICE)] * 2
    assert isinstance(km.centroids, np.ndarray) and km.centroids.shape == (shape[2], shape[1])
    assert km.centroids.dtype == np.float32 and km.obj.dtype == np.float64 and isinstance(final, float)
    assert [set(s) for s in km.iteration_stats] == [{"obj", "nsplit"}] * 2
    # numpy rows go through the library's staged host path and cluster the same
    calls.clear()
    kh = kmeans(fx, shape, niter=2)
    kh.train(x, init_centroids=init)
    assert [c[3] for c in calls] == [_lib.MEM_HOST] * 2
    assert (kh.counts == km.counts).all()
    err = np.abs(kh.centroids.astype(np.float64) - km.centroids.astype(np.float64))
    assert (err <= ref.centroid_tol(km.centroids.astype(np.float64), x)).all()


def test_subsampling_and_redo(fx, torch):
    """n > k * max_points_per_centroid trains on the seeded subsample; nredo keeps the best final objective."""
    shape = ref.SHAPES[0]
    x, _ = ref.case(shape)
    xt = dev(torch, x)
    km = fx.Kmeans(shape[1], 5, niter=2, max_points_per_centroid=100, seed=9)
    km.train(xt)
    rows = km._subsample_rows(shape[0])
    assert rows.shape == (500,) and km.counts.sum() == 500
    sub = fx.Kmeans(shape[1], 5, niter=2, seed=9)
    sub.train(dev(torch, x[rows]), init_centroids=x[rows][km._init_rows(500)])
    assert sub.centroids.tobytes() == km.centroids.tobytes()
    redo = fx.Kmeans(shape[1], 5, niter=2, nredo=3, seed=9, max_points_per_centroid=1000)
    redo.train(xt)
    finals = []
    for r in range(3):
        one = fx.Kmeans(shape[1], 5, niter=2, max_points_per_centroid=1000)
        finals.append(one.train(xt, init_centroids=x[redo._init_rows(shape[0], r)]))
        if finals[-1] == redo.obj[-1]:
            assert one.centroids.tobytes() == redo.centroids.tobytes()
    assert redo.obj[-1] == min(finals)
    assert (redo.index.reconstruct_n(0, 5) == redo.centroids).all()

"""GPU checks of range_search (fx_range.hip through the C ABI and the Python
layers) against numpy references computed here.

Exact-arithmetic cases use the integer-grid generator (every value k/64,
|k| <= 255): N = sum (dk)^2 in int64 and D = float32(N / 4096) is exactly the
library's distance (fp64 sum of multiples of 1/4096 below 2^53, one rounding),
so lims, I and D must be bit-identical, for every storage dtype (the values
are exact in bf16 and fp16).  Gaussian cases take their radius in the middle
of a wide gap of the sorted fp64 distances, so membership does not hinge on
the last bits of the summation order; ids must be equal and D within the
project's bar 1e-5 * max(1, |D|).
"""
import json
import shutil

import numpy as np
import pytest

from oracle.flat_l2 import synth
from tests._data import gaussian_small

pytestmark = pytest.mark.gpu

DTYPES = ["float32", "bfloat16", "float16"]
RTOL = 1e-5


@pytest.fixture(scope="module")
def fx():
    from rag_faiss_embedding_amd import _lib, faiss
    if _lib.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    return faiss


def grid_dist(xq, xb):
    """Exact squared distances of integer-grid rows: float32(N / 4096)."""
    a = np.rint(xq.astype(np.float64) * 64).astype(np.int64)
    b = np.rint(xb.astype(np.float64) * 64).astype(np.int64)
    N = (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2 * (a @ b.T)
    assert (N >= 0).all()
    return (N.astype(np.float64) / 4096.0).astype(np.float32), N


def ref_range(D, radius, ip=False):
    """faiss's flat range scan: per query, ascending row id."""
    hit = D > np.float32(radius) if ip else D < np.float32(radius)
    lims = np.concatenate([[0], np.cumsum(hit.sum(1))]).astype(np.uint64)
    qi, ri = np.nonzero(hit)
    return lims, D[qi, ri], ri.astype(np.int64)


def assert_identical(got, want):
    lims, D, I = got
    assert lims.dtype == np.uint64 and D.dtype == np.float32 and I.dtype == np.int64
    np.testing.assert_array_equal(lims, want[0])
    np.testing.assert_array_equal(I, want[2])
    np.testing.assert_array_equal(D.view(np.uint32), want[1].view(np.uint32))


@pytest.fixture(scope="module")
def grid():
    """The exact case: 5000 x 384 corpus, 129 queries, the radius an attained
    distance with exactly 2000 pairs strictly inside."""
    xb, xq = synth(7, 0, 5000, 384), synth(11, 0, 129, 384)
    D, N = grid_dist(xq, xb)
    assert N.max() < 2 ** 24
    radius = np.sort(D.ravel())[2000]
    assert int((D < radius).sum()) == 2000 and int((D <= radius).sum()) == 2001
    per_q = (D < radius).sum(1)
    assert per_q.min() == 0 and per_q.max() == 164
    for a in (xb, xq, D):
        a.setflags(write=False)
    return xb, xq, D, radius


@pytest.fixture(scope="module")
def grid_indexes(fx, grid):
    """One 5000-row index per storage dtype, shared by the read-only tests."""
    out = {}
    for dt in DTYPES:
        ix = fx.IndexFlatL2(384, dtype=dt)
        ix.add(grid[0])
        out[dt] = ix
    return out


@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_case_bit_identical(grid, grid_indexes, dtype):
    xb, xq, D, radius = grid
    ix = grid_indexes[dtype]
    got = ix.range_search(xq, radius)
    assert int(got[0][-1]) == 2000
    assert_identical(got, ref_range(D, radius))
    st = ix.last_range_stats()
    assert st["passes"] == 1 and st["candidates"] >= 2000
    # the non-strict neighbour: one ulp up takes the attained pair in
    up = np.nextafter(radius, np.float32(np.inf))
    got = ix.range_search(xq, up)
    assert int(got[0][-1]) == 2001
    assert_identical(got, ref_range(D, up))


@pytest.mark.parametrize("nq", [1, 128, 129])
@pytest.mark.parametrize("n", [1, 127, 128, 129, 300, 5000])
@pytest.mark.parametrize("dtype", DTYPES)
def test_tile_edges(fx, grid, grid_indexes, dtype, n, nq):
    """Corpus and query counts around the 128 x 128 tile.  The radius is the
    attained distance of rank min(2000, pairs // 2) of the sub-problem (the
    strict edge); corpora of <= 300 rows also take every pair."""
    xb, xq, D, _ = grid
    Ds = np.ascontiguousarray(D[:nq, :n])
    if n == 5000:
        ix = grid_indexes[dtype]
    else:
        ix = fx.IndexFlatL2(384, dtype=dtype)
        ix.add(xb[:n])
    radius = np.sort(Ds.ravel())[min(2000, Ds.size // 2)]
    assert_identical(ix.range_search(xq[:nq], radius), ref_range(Ds, radius))
    if n <= 300:
        everything = np.nextafter(Ds.max(), np.float32(np.inf))
        got = ix.range_search(xq[:nq], everything)
        assert int(got[0][-1]) == n * nq
        assert_identical(got, ref_range(Ds, everything))


@pytest.mark.parametrize("d,dtype", [(64, "bfloat16"), (100, "float16"), (768, "bfloat16")])
def test_row_widths(fx, d, dtype):
    """One 128-B stage per row, a padded kdim, and a 1,536-B row."""
    xb, xq = synth(7, 0, 1000, d), synth(11, 0, 130, d)
    D, _ = grid_dist(xq, xb)
    ix = fx.IndexFlatL2(d, dtype=dtype)
    ix.add(xb)
    radius = np.sort(D.ravel())[1500]
    got = ix.range_search(xq, radius)
    assert int(got[0][-1]) > 0
    assert_identical(got, ref_range(D, radius))


# ---------------------------------------------------------------------------
# gaussian data
# ---------------------------------------------------------------------------
def _round_rows(x, dtype):
    import torch
    if dtype == "float32":
        return x
    tdt = torch.bfloat16 if dtype == "bfloat16" else torch.float16
    return torch.from_numpy(np.array(x)).to(tdt).to(torch.float32).numpy()


def gap_radius(keys64):
    """float32 midpoint of the widest gap between consecutive sorted keys of
    rank in [500, 800); the gap must be >= 1e-5 |R|."""
    s = np.sort(keys64.ravel())[500:800]
    i = int(np.argmax(np.diff(s)))
    R = np.float32(0.5 * (s[i] + s[i + 1]))
    gap = float(s[i + 1] - s[i])
    print(f"\n[range-gpu] gap {gap:.3e} = {gap / abs(float(R)):.2e} R")
    assert gap >= 1e-5 * abs(float(R)) and s[i] < float(R) < s[i + 1]
    return R


def assert_within_bar(got, keys64, hit, ip=False):
    lims, D, I = got
    np.testing.assert_array_equal(lims, np.concatenate([[0], np.cumsum(hit.sum(1))]).astype(np.uint64))
    qi, ri = np.nonzero(hit)
    np.testing.assert_array_equal(I, ri)
    want = -keys64[qi, ri] if ip else keys64[qi, ri]
    assert (np.abs(D.astype(np.float64) - want) <= RTOL * np.maximum(1.0, np.abs(want))).all()


@pytest.fixture(scope="module")
def gauss():
    xb, xq = gaussian_small()
    xb.setflags(write=False)
    xq.setflags(write=False)
    return xb, xq


@pytest.mark.parametrize("dtype", DTYPES)
def test_gaussian_l2(fx, gauss, dtype):
    xb, xq = gauss
    Y = _round_rows(xb, dtype).astype(np.float64)
    D64 = np.stack([((q.astype(np.float64) - Y) ** 2).sum(1) for q in xq])  # difference form: no cancellation
    R = gap_radius(D64)
    ix = fx.IndexFlatL2(384, dtype=dtype)
    ix.add(xb)
    got = ix.range_search(xq, R)
    hit = D64 < float(R)
    print(f"[range-gpu] {dtype}: hits {int(hit.sum())}, max per query {int(hit.sum(1).max())}, "
          f"stats {ix.last_range_stats()}")
    assert_within_bar(got, D64, hit)
    assert ix.last_range_stats()["candidates"] >= int(hit.sum())


@pytest.mark.parametrize("dtype", DTYPES)
def test_gaussian_ip(fx, gauss, dtype):
    xb, xq = gauss
    Y = _round_rows(xb, dtype).astype(np.float64)
    neg = -(xq.astype(np.float64) @ Y.T)          # the rule on -q.y
    R = gap_radius(neg)
    ix = fx.IndexFlatIP(384, dtype=dtype)
    ix.add(xb)
    got = ix.range_search(xq, -R)                 # q.y > -R  <=>  -q.y < R
    hit = neg < float(R)
    assert int(hit.sum()) > 0
    assert_within_bar(got, neg, hit, ip=True)


def test_gaussian_normalized(fx, gauss):
    xb, xq = gauss
    ix = fx.IndexFlatL2(384, normalize=True)
    ix.add(xb)
    Y = ix.reconstruct_n(0, ix.ntotal).astype(np.float64)   # the stored (normalised) rows
    assert np.allclose((Y ** 2).sum(1), 1.0, atol=1e-5)
    qn = (xq / np.linalg.norm(xq, axis=1, keepdims=True)).astype(np.float32)
    D64 = np.stack([((q.astype(np.float64) - Y) ** 2).sum(1) for q in qn])
    R = gap_radius(D64)
    hit = D64 < float(R)
    assert_within_bar(ix.range_search(qn, R), D64, hit)


# ---------------------------------------------------------------------------
# edges
# ---------------------------------------------------------------------------
def test_edges(fx, grid):
    xb, xq, D, _ = grid
    xb, xq, D = xb[:300], xq[:3], np.ascontiguousarray(D[:3, :300])
    ix = fx.IndexFlatL2(384)
    lims, Dr, Ir = ix.range_search(xq, 10.0)                 # empty index
    assert lims.tolist() == [0, 0, 0, 0] and Dr.size == 0 and Ir.size == 0
    assert ix.last_range_stats() == {"candidates": 0, "passes": 0}
    ix.add(xb)
    lims, Dr, Ir = ix.range_search(xq, D.min())              # below the smallest distance (strict)
    assert lims.tolist() == [0, 0, 0, 0] and Dr.size == 0
    lims, Dr, Ir = ix.range_search(xq, 1e30)
    assert lims.tolist() == [0, 300, 600, 900]
    assert (Ir.reshape(3, 300) == np.arange(300)).all()
    np.testing.assert_array_equal(Dr.reshape(3, 300), D)
    lims, Dr, Ir = ix.range_search(xq[:0], 1.0)              # nq == 0
    assert lims.tolist() == [0] and Dr.size == 0
    with pytest.raises(RuntimeError, match="radius"):
        ix.range_search(xq, float("nan"))
    with pytest.raises(AssertionError):
        ix.range_search(xq[:, :100], 1.0)
    with pytest.raises(RuntimeError):
        ix.set_option("range_cap", -1)
    with pytest.raises(RuntimeError):
        ix.set_option("range_cap", (1 << 30) + 1)

    # the queries themselves as rows 300..302: radius 0 is strict -> nothing;
    # a tiny radius -> each query's own row at D = 0
    ix.add(xq)
    for r0 in (0.0, -1.0):
        lims, Dr, Ir = ix.range_search(xq, r0)
        assert lims.tolist() == [0, 0, 0, 0] and Dr.size == 0
    lims, Dr, Ir = ix.range_search(xq, 1e-6)
    assert lims.tolist() == [0, 1, 2, 3] and Ir.tolist() == [300, 301, 302] and (Dr == 0).all()
    ix.set_id_offset(1000)
    lims, Dr, Ir = ix.range_search(xq, 1e-6)
    assert Ir.tolist() == [1300, 1301, 1302]
    ix.set_id_offset(0)

    # a second add, then the same search again: the new rows are seen
    radius = np.sort(D.ravel())[200]
    D2 = np.concatenate([D, grid_dist(xq, xq)[0], D[:, :50]], axis=1)
    ix.add(xb[:50])
    assert_identical(ix.range_search(xq, radius), ref_range(D2, radius))

    ix.reset()
    assert ix.ntotal == 0
    lims, Dr, Ir = ix.range_search(xq, 1e30)
    assert lims.tolist() == [0, 0, 0, 0] and Dr.size == 0
    ix.add(xb[:10])
    lims, Dr, Ir = ix.range_search(xq, 1e30)
    assert lims.tolist() == [0, 10, 20, 30]


# ---------------------------------------------------------------------------
# capacity: a scan that emits more than the buffer holds runs once more
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_two_pass_capacity(fx, grid, dtype):
    xb, xq, D, radius = grid
    want = ref_range(D, radius)
    ix = fx.IndexFlatL2(384, dtype=dtype)
    ix.add(xb)
    first = ix.range_search(xq, radius)
    s1 = ix.last_range_stats()
    assert s1["passes"] == 1 and s1["candidates"] >= 2000
    assert_identical(first, want)
    ix.set_option("range_cap", 64)
    second = ix.range_search(xq, radius)
    s2 = ix.last_range_stats()
    assert s2["passes"] == 2 and s2["candidates"] == s1["candidates"] >= 2000
    assert_identical(second, want)
    # the grown buffer is kept: the same call now fits in one pass
    third = ix.range_search(xq, radius)
    assert ix.last_range_stats()["passes"] == 1
    assert_identical(third, want)


def test_options_do_not_change_results(fx, grid):
    xb, xq, D, radius = grid
    want = ref_range(D, radius)
    ix = fx.IndexFlatL2(384)
    ix.add(xb)
    for name, value in (("f32_split", 0), ("centre", 0), ("scan_place", 0), ("scan_v5", 0), ("scan_pub", 0),
                        ("reduce_cand", 0), ("search_graph", 1), ("host_spin", 0)):
        ix.set_option(name, value)
        assert_identical(ix.range_search(xq, radius), want)


# ---------------------------------------------------------------------------
# plumbing
# ---------------------------------------------------------------------------
def test_device_tensor_queries(fx, grid, grid_indexes):
    import torch
    xb, xq, D, radius = grid
    ix = grid_indexes["float32"]
    host = ix.range_search(xq, radius)
    for tdt in (torch.float32, torch.bfloat16):   # grid values are exact in bf16
        q = torch.from_numpy(np.array(xq)).cuda().to(tdt)
        lims, Dd, Id = ix.range_search(q, float(radius))
        assert lims.dtype == torch.int64 and lims.device == q.device
        assert Dd.is_cuda and Dd.dtype == torch.float32 and Id.is_cuda and Id.dtype == torch.int64
        np.testing.assert_array_equal(lims.cpu().numpy(), host[0].astype(np.int64))
        np.testing.assert_array_equal(Id.cpu().numpy(), host[2])
        np.testing.assert_array_equal(Dd.cpu().numpy().view(np.uint32), host[1].view(np.uint32))


@pytest.mark.parametrize("graph", [0, 1])
def test_knn_search_is_undisturbed(fx, grid, graph):
    xb, xq, D, radius = grid
    ix = fx.IndexFlatL2(384)
    ix.add(xb)
    ix.set_option("search_graph", graph)
    before = [ix.search(xq[i:i + 4], 10) for i in (0, 4)]
    before += [ix.search(xq[i:i + 4], 10) for i in (0, 4)]     # (graph: the second round replays)
    want = ref_range(D, radius)
    assert_identical(ix.range_search(xq, radius), want)
    after = [ix.search(xq[i:i + 4], 10) for i in (0, 4)]
    for (Db, Ib), (Da, Ia) in zip(before[2:], after):
        np.testing.assert_array_equal(Ib, Ia)
        np.testing.assert_array_equal(Db, Da)
    assert_identical(ix.range_search(xq, radius), want)
    Dk = np.sort(D[:4], axis=1)[:, :10]
    np.testing.assert_array_equal(after[0][0], Dk)


def test_store_search_radius_on_the_shipped_index(fx, golden_dir, tmp_path, monkeypatch):
    from rag_faiss_embedding_amd import _mapping, faiss_store
    z = np.load(golden_dir / "shipped_knn.npz")
    xb = z["xb"]
    (tmp_path / "data").mkdir()
    shutil.copy(golden_dir / "shipped_index.bin", tmp_path / "data" / "faiss_index.bin")
    ids = json.loads((golden_dir / "shipped_ids.json").read_text())["mapping_ids"]
    (tmp_path / "data" / "faiss_index.bin.mapping").write_bytes(_mapping.dumps_ids(ids))
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(faiss_store.FAISSVectorStore, "_instance", None)
    monkeypatch.setattr(faiss_store.FAISSVectorStore, "_initialized", False)
    store = faiss_store.FAISSVectorStore()
    d5, d6 = float(z["D_k10"][0][4]), float(z["D_k10"][0][5])
    assert d5 < d6
    dist, got = store.search_radius(xb[0], 0.5 * (d5 + d6))
    assert got == [ids[r] for r in z["I_k5"][0]]
    np.testing.assert_allclose(dist, z["D_k5"][0], rtol=RTOL, atol=RTOL)
    monkeypatch.setattr(faiss_store.FAISSVectorStore, "_instance", None)
    monkeypatch.setattr(faiss_store.FAISSVectorStore, "_initialized", False)

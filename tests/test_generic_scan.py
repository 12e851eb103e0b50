"""The 128 x 128 tile loop shared by the k-NN scan of row widths without a
k_scan_v4 / k_scan_v5 instance (k_scan_topk) and by the radius filter
(k_range_scan), through both callers on the same index.

Row widths only the generic kernel serves, with an odd number of 128-B stages
per row, so that the stage buffer's parity and the norm slot's parity come
apart across tile boundaries: fp32 d = 96 (384 B, 3 stages), bfloat16 d = 320
(640 B, 5 stages), float16 d = 64 (128 B, 1 stage).  n = 3100 is 25 corpus
tiles (corpus-partitioned placement, the last tile with 28 rows), n = 300 is 3
tiles under placement 0 (the last with 44 rows), n = 1500 is 12 tiles under
placement 0 in 4 splits (the last tile with 92 rows): the small index on which
k = 40 fits the splits' lists, so that its scan is checked without the re-scan;
nq = 130 is two query tiles, the second with 2 live queries.

Data: the values of tests/_data.py's gaussian corpus, re-cut to (n, d) rows
and (nq, d) queries.  References are computed on the stored rows
(reconstruct_n):
  k-NN   oracle.cpu.knn_exact (L2) / oracle.flat_l2.knn_inner_product (IP, the
         oracle every IP test of the suite uses); ids equal, distances by
         assert_parity's rule; no query may need the re-scan (but where one
         split's KP-entry list cannot hold k: test_knn).
  range  test_range_gpu's reference: fp64 sums, one rounding to fp32, the
         strict test against the fp32 radius (ref_range), the radius an
         attained distance of rank min(2000, pairs // 2); ids and lims equal,
         distances within the same 1e-5 max(1, |D|) (assert_within_bar).
"""
import numpy as np
import pytest

from oracle import cpu as C
from oracle import flat_l2 as F
from tests._data import gaussian_small
from tests.test_gpu_parity import assert_parity
from tests.test_range_gpu import assert_within_bar, ref_range

pytestmark = pytest.mark.gpu

WIDTHS = [("float32", 96), ("bfloat16", 320), ("float16", 64)]
SCAN_WIDTHS_64 = (8, 12, 16, 24)  # row_bytes / 64 of the k_scan_v4 instances (and of the split-fp32 image)
NMAX, QMAX = 3100, 130
KP = 32  # candidates the scan keeps per (query, corpus split) (fx_internal.h)


@pytest.fixture(scope="module")
def fx():
    from rag_faiss_embedding_amd import _lib, faiss
    if _lib.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    return faiss


@pytest.fixture(scope="module")
def values():
    v = gaussian_small()[0].ravel()
    v.setflags(write=False)
    return v


@pytest.fixture(scope="module", params=[(m, dt, d, n) for m in ("L2", "IP") for dt, d in WIDTHS for n in (NMAX, 1500, 300)],
                ids=lambda p: "-".join(map(str, p)))
def case(request, fx, values):
    """One index per (metric, width, n) with its stored rows, its queries and
    the fp64 keys of all pairs (L2: squared distance; IP: -x.y)."""
    metric, dtype, d, n = request.param
    esz = 4 if dtype == "float32" else 2
    assert (d * esz) % 128 == 0 and (d * esz) // 64 not in SCAN_WIDTHS_64  # generic kernel, no split-fp32 image
    xb = values[:NMAX * d].reshape(NMAX, d)[:n]
    xq = values[NMAX * d:(NMAX + QMAX) * d].reshape(QMAX, d)
    ix = (fx.IndexFlatL2 if metric == "L2" else fx.IndexFlatIP)(d, dtype=dtype)
    ix.add(xb)
    Y = ix.reconstruct_n(0, n)
    Y64, q64 = Y.astype(np.float64), xq.astype(np.float64)
    if metric == "L2":
        keys = np.stack([((q - Y64) ** 2).sum(1) for q in q64])  # difference form: no cancellation
    else:
        keys = -(q64 @ Y64.T)
    for a in (Y, keys):
        a.setflags(write=False)
    return metric, ix, xq, Y, keys


@pytest.mark.parametrize("k", [10, 40])
@pytest.mark.parametrize("nq", [QMAX, 1])
def test_knn(case, nq, k):
    metric, ix, xq, Y, _ = case
    D, I = ix.search(xq[:nq], k)
    plan = ix.last_scan_plan()
    assert plan["tile_rows"] == 128 and plan["query_tile"] == 128
    Dr, Ir = C.knn_exact(xq[:nq], Y, k) if metric == "L2" else F.knn_inner_product(xq[:nq], Y, k)
    assert_parity(D, I, Dr, Ir)
    # A scan that lost rows must not hide behind the re-scan: no query may need it.  The one exception is
    # structural: the scan keeps KP candidates per (query, split), and 3 corpus tiles are one split (>= 3 tiles
    # per split), so k = 40 on 300 rows has 32 candidates for 40 results and k_refine_big flags every query
    # (n1 < k), whatever the data.
    if plan["splits"] * KP >= k:
        assert ix.last_fallbacks() == 0
    else:
        assert ix.ntotal == 300 and k == 40 and plan["splits"] == 1
        assert ix.last_fallbacks() == nq


@pytest.mark.parametrize("nq", [QMAX, 1])
def test_range(case, nq):
    metric, ix, xq, Y, keys = case
    ip = metric == "IP"
    keys = keys[:nq]
    k32 = keys.astype(np.float32)
    R = np.sort(k32.ravel())[min(2000, k32.size // 2)]  # an attained key: the strict edge
    want = ref_range(-k32, -R, ip=True) if ip else ref_range(k32, R)
    hit = k32 < R
    assert int(want[0][-1]) == int(hit.sum()) > 0
    assert (np.add.reduceat(hit.sum(0), np.arange(0, hit.shape[1], 128)) > 0).all()  # hits in every corpus tile
    got = ix.range_search(xq[:nq], float(-R if ip else R))
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[2], want[2])
    assert_within_bar(got, keys, hit, ip=ip)
    assert ix.last_range_stats()["candidates"] >= int(hit.sum())

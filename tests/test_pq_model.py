"""CPU check of the product quantizer's scan bound (fx_pq.hip k_pq_prep,
DESIGN.md 3.16) on the numpy model of tests/_pq_ref.py: for every (query, row)
the model's key -- the three bf16 products through a sequential fp32 chain, the
worst case for the MFMA's accumulation -- plus the shift lies within E of the
exact fp64 key of the decoded row.  It also counts the queries the refine's
certification would flag."""
import numpy as np
import pytest

from tests import _pq_ref as R

SHAPES = [(16, 2), (64, 8), (96, 6), (768, 96)]


def setup(d, M, metric, scale, n=160, nq=12):
    xb, xq = R.clustered(d, n, nq, seed=d + M, scale=scale)
    cents = R.sampled_centroids(xb, M)
    codes = R.encode(xb, cents)
    dec = R.decode(codes, cents)
    xh, xl, shift, eps = R.prep(xq, metric, cents)
    yh, yl = R.image_rows(codes, cents)
    ny = R.row_norms(codes, cents)
    return xq, cents, codes, dec, (xh, xl, yh, yl, ny), shift, eps


@pytest.mark.parametrize("scale", [1.0, 100.0], ids=["unit", "x100"])
@pytest.mark.parametrize("metric", [R.L2, R.IP], ids=["L2", "IP"])
@pytest.mark.parametrize("d,M", SHAPES)
def test_model_key_within_the_bound(d, M, metric, scale):
    xq, cents, codes, dec, ops, shift, eps = setup(d, M, metric, scale)
    exact = R.exact64(xq, dec, metric)
    for keys in (R.keys_chain(*ops, metric), R.keys64(*ops, metric)):
        err = np.abs(keys.astype(np.float64) + shift[:, None] - exact)
        worst = (err / eps.astype(np.float64)[:, None]).max()
        print(f"d={d} M={M} metric={metric} scale={scale}: worst |key + shift - exact| / E = {worst:.3f}")
        assert (err <= eps.astype(np.float64)[:, None]).all(), worst
    # the exactly summed key and the chained one differ by the accumulation term at most
    gap = np.abs(R.keys_chain(*ops, metric).astype(np.float64) - R.keys64(*ops, metric))
    assert (gap <= R.accumulation_term(xq, metric, cents)[:, None]).all()


def test_bound_is_not_loose_by_orders_of_magnitude():
    """E at unit norm is the ~1e-4 of the split form, not the ~8e-3 a hi-plane-only scan would need."""
    for d, M in ((64, 8), (128, 16)):
        xq, cents, *_rest, eps = setup(d, M, R.L2, 1.0)
        assert eps.max() < 1e-3 and eps.min() > 1e-6, (d, M, eps.min(), eps.max())


@pytest.mark.parametrize("metric", [R.L2, R.IP], ids=["L2", "IP"])
@pytest.mark.parametrize("d,M", [(64, 8), (128, 16)])
def test_uncertified_counts(d, M, metric):
    """At k = 32 = KP the k-th exact key is the kept list's last, which no bound E > 0 separates from
    the list's own threshold: every query of an index with 32 rows or more is flagged.  Below it the
    count is what the data gives; on these unit-norm clustered rows the split bound certifies k = 1
    and k = 10 outright."""
    xq, cents, codes, dec, ops, shift, eps = setup(d, M, metric, 1.0, n=400, nq=24)
    keys = R.keys_chain(*ops, metric)
    counts = {k: R.uncertified(keys, xq, dec, metric, shift, eps, k) for k in (1, 10, 31, 32)}
    print(f"d={d} M={M} metric={metric}: uncertified of {len(xq)} at k = 1, 10, 31, 32: {counts}")
    assert counts[32] == len(xq)
    assert counts[1] <= counts[10] <= counts[31] <= counts[32]
    assert counts[1] == 0 and counts[10] == 0

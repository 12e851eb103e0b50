"""The IndexIVFPQ reference of tests/_ivfpq_ref.py checked against the two references it is composed
from, on the CPU."""
import numpy as np
import pytest

from tests import _ivf_ref as IV
from tests import _ivfpq_ref as R
from tests import _pq_ref as PQ

L2, IP = R.METRIC_L2, R.METRIC_INNER_PRODUCT


@pytest.mark.parametrize("metric", [L2, IP], ids=["L2", "IP"])
def test_without_residual_and_every_list_probed_it_is_the_product_quantizer(metric):
    d, M = 20, 5
    c, xb, lists, xq = IV.edge_corpus(d, "float32")
    cents = R.codebook(xb, lists, c, M, by_residual=False)
    assert (cents == PQ.sampled_centroids(xb, M)).all()
    m = R.Model(xb, lists, c, cents, by_residual=False)
    # codes and decoded rows are the flat product quantizer's of the same rows
    assert (m.codes == PQ.encode(xb, cents)).all()
    assert (m.y.view(np.uint32) == PQ.decode(m.codes, cents).view(np.uint32)).all()
    order = IV.store_order(lists)
    ids = np.arange(xb.shape[0], dtype=np.int64)
    ys = np.ascontiguousarray(m.y[order])
    for k in (1, 10, 40):
        D, I = m.search(xq, ids, k, len(IV.EDGE_SIZES), metric)
        Ds, Is = PQ.search(xq, ys, k, metric)
        # the same distances; the same rows up to the tie rule (the flat search ranks equal decoded
        # rows by row number, the inverted file by (list, insertion order), which is the position in ys)
        assert (D.view(np.uint32) == Ds.view(np.uint32)).all()
        assert (I == order[Is]).all()


@pytest.mark.parametrize("d,M", [(20, 5), (384, 48)])
def test_residual_encoding_decodes_closer_to_the_rows(d, M):
    c, xb, lists, _ = IV.edge_corpus(d, "float32")
    err = {}
    for by_residual in (True, False):
        m = R.Model(xb, lists, c, R.codebook(xb, lists, c, M, by_residual), by_residual)
        err[by_residual] = np.linalg.norm(m.y.astype(np.float64) - xb.astype(np.float64), axis=1)
    print(f"d = {d} M = {M}: mean |y - x| {err[True].mean():.3g} with by_residual, {err[False].mean():.3g} without")
    assert err[True].mean() < err[False].mean()


def test_residual_and_reconstruct_are_single_rounded_fp32_operations():
    d, M = 20, 5
    c, xb, lists, _ = IV.edge_corpus(d, "float32")
    r = R.residuals(xb, lists, c)
    want = (xb.astype(np.float64) - c[lists].astype(np.float64)).astype(np.float32)  # exact difference, one rounding
    assert (r.view(np.uint32) == want.view(np.uint32)).all()
    m = R.Model(xb, lists, c, R.codebook(xb, lists, c, M))
    want = (c[lists].astype(np.float64) + m.dec.astype(np.float64)).astype(np.float32)
    assert (m.y.view(np.uint32) == want.view(np.uint32)).all()
    assert (m.dec.view(np.uint32) == PQ.decode(m.codes, m.cents).view(np.uint32)).all()
    # searching one list finds only its rows
    D, I = m.search(c[5:6], np.arange(xb.shape[0]), 400, 1, L2)
    got = I[0][I[0] >= 0]
    assert got.size == IV.EDGE_SIZES[5] and (lists[got] == 5).all()


@pytest.mark.parametrize("metric", [L2, IP], ids=["L2", "IP"])
def test_rows_of_one_list_with_equal_codes_tie_and_rank_by_insertion_order(metric):
    d, M = 20, 5
    c, xb, lists, xq = IV.edge_corpus(d, "float32")
    # a row of list 11 added three times: equal codes whatever the codebook
    r = int(np.flatnonzero(lists == 11)[7])
    xb = np.concatenate([xb, xb[r:r + 1], xb[r:r + 1]])
    lists = np.concatenate([lists, [11, 11]])
    m = R.Model(xb, lists, c, R.codebook(xb, lists, c, M))
    rows = np.flatnonzero(lists == 11)
    same = rows[(m.codes[rows] == m.codes[r]).all(1)]  # ascending: insertion order
    assert same.size >= 3 and (m.y[same].view(np.uint32) == m.y[same[0]].view(np.uint32)).all()
    ids = np.arange(xb.shape[0], dtype=np.int64)
    D, I = m.search(xq, ids, 1100, 1, metric)
    for q in range(xq.shape[0]):
        pos = [int(np.flatnonzero(I[q] == r)[0]) for r in same if (I[q] == r).any()]
        if not pos:
            continue
        assert len(pos) == same.size and pos == list(range(pos[0], pos[0] + same.size)), "ties rank by insertion order"
        assert (D[q, pos].view(np.uint32) == D[q, pos[0]].view(np.uint32)).all()

"""The IndexIVFFlat reference of tests/_ivf_ref.py checked against the flat
oracle and against its own stated tie rule (CPU)."""
import numpy as np

from oracle import flat_l2 as O
from tests import _ivf_ref as ref

L2, IP = ref.METRIC_L2, ref.METRIC_INNER_PRODUCT


def _data(seed=0, n=400, d=12, nlist=7, nq=9):
    r = np.random.default_rng(seed)
    xb = r.standard_normal((n, d)).astype(np.float32)
    xq = r.standard_normal((nq, d)).astype(np.float32)
    c = np.ascontiguousarray(xb[:nlist])
    return xb, xq, c


def test_nprobe_nlist_equals_the_flat_oracle_on_tie_free_data():
    xb, xq, c = _data()
    for metric, knn in ((L2, O.knn_exact), (IP, O.knn_inner_product)):
        lists = ref.assign(xb, c, metric)
        Df, If = knn(xq, xb, 11)
        assert (Df[:, 1:] != Df[:, :-1]).all()
        D, I = ref.search(xq, xb, np.arange(xb.shape[0]), lists, c, 10, c.shape[0], metric)
        assert (I == If[:, :10]).all() and (D == Df[:, :10]).all()


def test_probe_and_assign_follow_the_quantizer_and_its_tie_rule():
    c = np.array([[0, 0], [2, 0], [0, 2], [2, 0]], dtype=np.float32)  # centroids 1 and 3 coincide
    x = np.array([[1.9, 0.1], [1, 0], [0.1, 1.8]], dtype=np.float32)
    assert ref.assign(x, c, L2).tolist() == [1, 0, 2]  # [1, 0]: equidistant from 0 and 1 -> the smaller
    assert ref.probe(x[:1], c, 3, L2).tolist() == [[1, 3, 0]]
    assert ref.probe(x[:1], c, 50, L2).shape == (1, 4)  # nprobe is clamped to nlist
    assert ref.assign(x, c, IP).tolist() == [1, 1, 2]


def test_duplicated_rows_rank_by_distance_list_insertion():
    c = np.array([[0, 0], [10, 0]], dtype=np.float32)
    # rows at distance 1 of the query (0, 0) in list 0, two of them mirrored into list 1
    xb = np.array([[10, 1], [0, 1], [1, 0], [0, 1], [10, 1], [0, -1]], dtype=np.float32)
    ids = np.array([50, 40, 30, 20, 10, 0], dtype=np.int64)
    lists = ref.assign(xb, c, L2)
    assert lists.tolist() == [1, 0, 0, 0, 1, 0]
    xq = np.array([[0, 0], [5, 1]], dtype=np.float32)
    D, I = ref.search(xq, xb, ids, lists, c, 4, 1, L2)
    assert I[0].tolist() == [40, 30, 20, 0] and (D[0] == 1).all()  # one distance: insertion order within the list
    # query (5, 1) is equidistant from both centroids (probe tie -> list 0 first) and from rows 1, 3 (list 0)
    # and 0, 4 (list 1): the list number ranks before the insertion order
    D, I = ref.search(xq, xb, ids, lists, c, 6, 2, L2)
    assert I[1].tolist() == [30, 40, 20, 50, 10, 0] and D[1].tolist() == [17, 25, 25, 25, 25, 29]
    assert ref.store_order(lists).tolist() == [1, 2, 3, 5, 0, 4]


def test_k_larger_than_the_probed_rows_pads():
    xb, xq, c = _data(seed=3, n=60, nlist=5)
    for metric, fill in ((L2, ref.FLT_MAX), (IP, -ref.FLT_MAX)):
        lists = ref.assign(xb, c, metric)
        P = ref.probe(xq, c, 2, metric)
        D, I = ref.search(xq, xb, np.arange(60) + 1000, lists, c, 64, 2, metric)
        for q in range(xq.shape[0]):
            n = int(np.isin(lists, P[q]).sum())
            assert n < 64
            assert (I[q, :n] >= 1000).all() and (I[q, n:] == -1).all() and (D[q, n:] == fill).all()
            assert np.isin(lists[I[q, :n] - 1000], P[q]).all()
            assert len(set(I[q, :n].tolist())) == n

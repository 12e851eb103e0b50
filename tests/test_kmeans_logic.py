"""CPU checks of Kmeans' host logic (no device): the seeding and subsampling
rules, the argument errors, and the numpy reference step of the GPU tests
against a hand-computed example."""
import warnings

import numpy as np
import pytest

from rag_faiss_embedding_amd import faiss
from tests import _kmeans_ref as ref


def test_subsampling_threshold_and_permutation():
    km = faiss.Kmeans(8, 4, seed=77, max_points_per_centroid=10)
    assert km._subsample_rows(40) is None          # n == k * max_points_per_centroid: every row
    rows = km._subsample_rows(41)
    assert rows.dtype == np.int64 and rows.shape == (40,)
    assert (rows == np.random.RandomState(77).permutation(41)[:40]).all()
    assert len(set(rows.tolist())) == 40
    big = km._subsample_rows(1000)
    assert (big == np.random.RandomState(77).permutation(1000)[:40]).all()


def test_initial_centroid_rows_follow_the_seed_and_the_redo():
    km = faiss.Kmeans(8, 5, seed=1234)
    for redo in (0, 1, 3):
        want = np.random.RandomState(1234 + 1 + 15486557 * redo).permutation(300)[:5]
        assert (km._init_rows(300, redo) == want).all()
    assert not (km._init_rows(300, 0) == km._init_rows(300, 1)).all()
    assert (faiss.Kmeans(8, 5, seed=1234)._init_rows(300) == km._init_rows(300)).all()
    assert not (faiss.Kmeans(8, 5, seed=1235)._init_rows(300) == km._init_rows(300)).all()


def test_defaults_are_faiss():
    km = faiss.Kmeans(16, 3)
    assert (km.d, km.k, km.niter, km.nredo, km.verbose, km.spherical, km.seed) == (16, 3, 25, 1, False, False, 1234)
    assert (km.max_points_per_centroid, km.min_points_per_centroid) == (256, 39)
    assert km.centroids is None and km.index is None and km.iteration_stats == []
    assert "numpy" in faiss.Kmeans.__doc__ and "faiss run with the same seed" in " ".join(faiss.Kmeans.__doc__.split())


def test_weights_are_not_implemented():
    km = faiss.Kmeans(4, 2)
    with pytest.raises(NotImplementedError):
        km.train(np.zeros((100, 4), dtype=np.float32), weights=np.ones(100, dtype=np.float32))


def test_fewer_points_than_clusters_is_a_runtime_error():
    km = faiss.Kmeans(4, 8)
    with pytest.raises(RuntimeError, match="at least as large as number of clusters"):
        km.train(np.zeros((7, 4), dtype=np.float32))
    with pytest.raises(AssertionError):
        km.train(np.zeros((100, 5), dtype=np.float32))  # dimension mismatch


def test_too_few_points_only_warn_and_init_shape_is_checked():
    # (the shape check of init_centroids comes after the warning and before any device work)
    km = faiss.Kmeans(4, 2, min_points_per_centroid=39)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        with pytest.raises(AssertionError, match="init_centroids"):
            km.train(np.zeros((10, 4), dtype=np.float32), init_centroids=np.zeros((3, 4), dtype=np.float32))
    assert any("please provide at least 78 training points" in str(x.message) for x in w)


def test_reference_step_on_a_hand_computed_example():
    """6 points, 3 centroids, one of them far away: clusters {4, 2, 0}; the
    empty one is repaired from the largest."""
    x = np.array([[0, 0], [0, 2], [2, 0], [2, 2], [10, 10], [10, 12]], dtype=np.float32)
    c = np.array([[1, 1], [10, 11], [100, 100]], dtype=np.float32)
    s = ref.lloyd_step(x, c)
    assert s["assign"].tolist() == [0, 0, 0, 0, 1, 1]
    assert s["counts"].tolist() == [4, 2, 0]
    assert s["sums"].tolist() == [[4, 4], [20, 22], [0, 0]]
    assert s["obj"] == 4 * 2 + 2 * 1
    assert s["nsplit"] == 1
    up, dn = 1 + 1 / 1024, 1 - 1 / 1024
    # c0 = (1, 1) donates: c2 = c0 * (1 + EPS, 1 - EPS), c0 *= (1 - EPS, 1 + EPS); c1 = (10, 11) untouched
    assert s["centroids"].tolist() == [[dn, up], [10, 11], [up, dn]]
    assert s["centroids"].dtype == np.float32
    # every point's runner-up is far: gap = (d2 - d1) / d2
    assert s["gap"].min() > 0.9


def test_reference_ties_go_to_the_smaller_id_and_repairs_chain():
    x = np.array([[0, 0], [2, 0], [4, 0], [6, 0]], dtype=np.float32)
    c = np.array([[3, 0], [3, 0], [50, 0], [60, 0]], dtype=np.float32)  # centroids 0 and 1 tie everywhere
    s = ref.lloyd_step(x, c)
    assert s["assign"].tolist() == [0, 0, 0, 0] and s["counts"].tolist() == [4, 0, 0, 0]
    assert s["gap"].max() == 0
    # repairs in ascending order with working counts 4 -> (2, 2) -> (1, 2, 1) -> (1, 1, 1, 1):
    # ci = 1 from 0; ci = 2 from 0 (tie 2 = 2: the smaller index); ci = 3 from 1
    assert s["nsplit"] == 3
    up, dn = np.float32(1 + 1 / 1024), np.float32(1 - 1 / 1024)
    c0 = np.float32(3) * dn
    assert s["centroids"][1, 0] == np.float32(3) * up * dn      # copied from 0, then donor for 3
    assert s["centroids"][2, 0] == c0 * up
    assert s["centroids"][0, 0] == c0 * dn
    assert s["centroids"][3, 0] == np.float32(3) * up * up


def test_reference_spherical_normalises_and_takes_the_argmax():
    r = np.random.default_rng(0)
    x = r.standard_normal((50, 6)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    c = x[:4].copy()
    s = ref.lloyd_step(x, c, spherical=True)
    assert (s["assign"] == (x.astype(np.float64) @ c.astype(np.float64).T).astype(np.float32).argmax(1)).all()
    assert np.abs(np.linalg.norm(s["centroids"].astype(np.float64), axis=1) - 1).max() < 1e-6


def test_blob_inputs_are_the_issues():
    x, init = ref.blobs(1000, 20, 3, 4, 1)
    assert x.shape == (1000, 20) and init.shape == (3, 20) and x.dtype == np.float32
    assert (init[1] == 100).all()           # far = 1: index (1 + 2 * 0) % 3
    assert not x.flags.writeable
    xb, _ = ref.blobs(1000, 20, 3, 4, 1, "bfloat16")
    assert (ref.round_to(xb, "bfloat16") == xb).all() and not (xb == x).all()
    # over 5 reference iterations the k = 3 shape repairs once and its smallest gap clears the bound
    c, splits, gaps = np.array(init), [], []
    for _ in range(5):
        s = ref.lloyd_step(x, c)
        c = s["centroids"]
        splits.append(s["nsplit"])
        gaps.append(s["gap"].min())
    assert sum(splits) == 1 and min(gaps) >= ref.MIN_GAP

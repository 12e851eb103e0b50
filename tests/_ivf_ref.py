"""The CPU reference of the IndexIVFFlat tests (numpy + oracle.flat_l2): the
assignment of rows to lists, the probed lists of a query, and the search that
ranks a query's probed rows by (exact fp32 distance, list, insertion order).
Inputs are expected rounded to the storage dtype already (_kmeans_ref.round_to)."""
import functools

import numpy as np

from oracle import flat_l2 as O
from tests._kmeans_ref import round_to

METRIC_INNER_PRODUCT, METRIC_L2 = O.METRIC_INNER_PRODUCT, O.METRIC_L2
FLT_MAX = O.FLT_MAX


def _knn(xq, xb, k, metric):
    return O.knn_exact(xq, xb, k) if metric == METRIC_L2 else O.knn_inner_product(xq, xb, k)


def probe(xq, centroids, nprobe, metric):
    """[nq][min(nprobe, nlist)] list numbers: the quantizer's exact search."""
    return _knn(xq, centroids, min(int(nprobe), centroids.shape[0]), metric)[1]


def assign(x, centroids, metric):
    """The list of every row: the quantizer's k = 1 search (ties: the smaller centroid number)."""
    return probe(x, centroids, 1, metric)[:, 0]


def store_order(lists):
    """Row numbers in the list-ordered store: by list, insertion order within a list."""
    return np.argsort(np.asarray(lists), kind="stable")


def search(xq, xb, ids, lists, centroids, k, nprobe, metric, full=None):
    """(D, I): per query the k best rows among its probed lists, ranked by
    (exact fp32 distance, position in the list-ordered store); missing slots
    I = -1, D = +-FLT_MAX.  ``full``: a cached ``ranking(...)`` of the same
    queries and rows."""
    order = store_order(lists)
    ls, ids_s = np.asarray(lists)[order], np.asarray(ids, dtype=np.int64)[order]
    Df, If = ranking(xq, xb, lists, metric) if full is None else full
    P = probe(xq, centroids, nprobe, metric)
    nq = xq.shape[0]
    D = np.full((nq, k), FLT_MAX if metric == METRIC_L2 else -FLT_MAX, dtype=np.float32)
    I = np.full((nq, k), -1, dtype=np.int64)
    for q in range(nq):
        pos = If[q]
        pos = pos[pos >= 0]
        keep = np.isin(ls[pos], P[q])
        sel = np.flatnonzero(keep)[:k]
        D[q, :sel.size] = Df[q, sel]
        I[q, :sel.size] = ids_s[pos[sel]]
    return D, I


def ranking(xq, xb, lists, metric):
    """(D, positions) of EVERY row per query in (distance, store position) order."""
    xs = np.ascontiguousarray(xb[store_order(lists)])
    return _knn(xq, xs, xs.shape[0], metric)


EDGE_SIZES = (0, 1, 127, 128, 129, 300, 5, 0, 640, 64, 3, 1000)


@functools.lru_cache(maxsize=None)
def centroids_for(nlist, d, seed=7, scale=6.0):
    """nlist well-separated centroids of equal norm (so that the L2 and the IP
    quantizer both send ``centroid + small noise`` to that centroid); exact in
    bf16 / fp16 (rounded to bf16 first, which fp16 holds at this range)."""
    r = np.random.default_rng(seed)
    c = r.standard_normal((nlist, d))
    c = scale * c / np.sqrt((c * c).sum(1, keepdims=True))
    c = round_to(round_to(c.astype(np.float32), "bfloat16"), "float16")
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def edge_corpus(d, dtype, sizes=EDGE_SIZES, seed=11, noise=0.05, nq=37):
    """(centroids, xb, lists, xq): rows ``centroid[l] + noise`` with the given
    per-list counts, added in shuffled order; queries near random centroids.
    Read-only, shared."""
    r = np.random.default_rng(seed + d)
    nlist = len(sizes)
    c = centroids_for(nlist, d)
    lists = np.repeat(np.arange(nlist), sizes)
    r.shuffle(lists)
    xb = round_to(c[lists] + noise * r.standard_normal((lists.size, d)).astype(np.float32), dtype)
    ql = r.integers(0, nlist, nq)
    xq = round_to(c[ql] + 2 * noise * r.standard_normal((nq, d)).astype(np.float32), dtype)
    for a in (xb, lists, xq):
        a.setflags(write=False)
    return c, xb, lists, xq

"""The CPU reference of the IndexIVFPQ tests (include/fx_index.h "inverted file over
product-quantized codes"), composed from tests/_ivf_ref.py and tests/_pq_ref.py: assign the
rows to lists, encode r = fl32(x - c_l) (or x without by_residual) with a given codebook, decode
to y = fl32(c_l + decode(code)), and rank a query's probed rows of y as the inverted file does.
Every fp32 operation is rounded once, as the device's."""
import numpy as np

from tests import _ivf_ref as IV
from tests import _pq_ref as PQ

f32 = np.float32
METRIC_INNER_PRODUCT, METRIC_L2, FLT_MAX = IV.METRIC_INNER_PRODUCT, IV.METRIC_L2, IV.FLT_MAX


def residuals(x, lists, centroids, by_residual=True):
    """What is encoded: fl32(x - c_l), one rounded subtraction per dimension; x itself without by_residual."""
    x = np.ascontiguousarray(x, dtype=f32)
    if not by_residual:
        return x
    return (x - np.asarray(centroids, dtype=f32)[np.asarray(lists)]).astype(f32)


def reconstruct(codes, cents, lists, centroids, by_residual=True):
    """The decoded rows: fl32(c_l + decode(code)); decode(code) without by_residual."""
    dec = PQ.decode(codes, cents)
    if not by_residual:
        return dec
    return (np.asarray(centroids, dtype=f32)[np.asarray(lists)] + dec).astype(f32)


def codebook(xb, lists, centroids, M, by_residual=True):
    """The codebook the tests install: sampled from the rows' own residuals, no training."""
    return PQ.sampled_centroids(residuals(xb, lists, centroids, by_residual), M)


class Model:
    """An index over rows xb (insertion order) with given lists and codebook ``cents``
    [M][256][dsub]: ``codes`` ([n][M] uint8, insertion order), ``dec`` (decode(codes)), ``y`` (the
    decoded rows, insertion order)."""

    def __init__(self, xb, lists, centroids, cents, by_residual=True):
        self.centroids = np.asarray(centroids, dtype=f32)
        self.lists = np.asarray(lists)
        self.by_residual = bool(by_residual)
        self.cents = np.ascontiguousarray(cents, dtype=f32)
        self.codes = PQ.encode(residuals(xb, lists, centroids, by_residual), self.cents)
        self.dec = PQ.decode(self.codes, self.cents)
        self.y = reconstruct(self.codes, self.cents, lists, centroids, by_residual)
        for a in (self.cents, self.codes, self.dec, self.y):
            a.setflags(write=False)

    def list_codes(self, l):
        return self.codes[self.lists == l]

    def ranking(self, xq, metric):
        return IV.ranking(xq, self.y, self.lists, metric)

    def search(self, xq, ids, k, nprobe, metric, full=None):
        """(D, I) over the decoded rows of the probed lists, ranked by (exact fp32 distance, list,
        insertion order); missing slots I = -1, D = +-FLT_MAX."""
        return IV.search(xq, self.y, ids, self.lists, self.centroids, k, nprobe, metric, full=full)

"""The CPU reference of the k-means tests: a numpy restatement of one Lloyd
step (assignment, fp64 sums, centroids, the empty-cluster rule of
fx_kmeans_finish) and the blob data the GPU tests train on."""
import functools

import numpy as np

EPS = np.float32(1.0 / 1024.0)
UP, DOWN = np.float32(1) + EPS, np.float32(1) - EPS

# (n, d, k, seed, far): the shapes of tests/test_kmeans_gpu.py
SHAPES = [(3001, 100, 37, 1, 0), (3001, 100, 37, 2, 2), (4097, 384, 130, 3, 0), (1000, 20, 3, 4, 1),
          (2500, 768, 64, 5, 3)]
# Seeds of the rounded-data variants whose reference gap under the shape's own seed is too thin
# (bf16 3001 x 100 far = 2: 5.8e-7, fp16 2500 x 768: 3.2e-7): with these it is 1.9e-6 and 2.4e-6,
# and the repairs of iteration 1 are the same (2 and 3).
SEEDS = {((3001, 100, 37, 2, 2), "bfloat16"): 32, ((2500, 768, 64, 5, 3), "float16"): 15}
MIN_GAP = 5e-7  # > 4 fp32 ulps (4 * 2^-23 = 4.8e-7): rounding cannot decide an assignment


def round_to(x, dtype):
    """fp32 values rounded to ``dtype`` ("float32", "bfloat16", "float16") and back."""
    if dtype == "float32":
        return np.ascontiguousarray(x, dtype=np.float32)
    if dtype == "float16":
        return x.astype(np.float16).astype(np.float32)
    import torch
    return torch.from_numpy(np.array(x, dtype=np.float32)).bfloat16().float().numpy()


def case(shape, dtype="float32"):
    """(x, init) of one of SHAPES in ``dtype`` (the seed: the shape's, or SEEDS')."""
    n, d, k, seed, far = shape
    return blobs(n, d, k, SEEDS.get((tuple(shape), dtype), seed), far, dtype)


@functools.lru_cache(maxsize=None)
def blobs(n, d, k, seed, far, dtype="float32"):
    """(x, init): 12 gaussian blobs rounded to ``dtype``, and k of its rows as
    initial centroids, ``far`` of them overwritten with far-away constants (so
    their clusters are empty in iteration 1).  Read-only."""
    r = np.random.default_rng(seed)
    centres = r.standard_normal((12, d)).astype(np.float32) * 2
    which = r.integers(0, 12, n)
    x = round_to(centres[which] + r.standard_normal((n, d)).astype(np.float32) * 0.5, dtype)
    init = x[r.permutation(n)[:k]].copy()
    for j in range(far):
        init[(1 + 2 * j) % k] = 100 + j
    x.setflags(write=False)
    init.setflags(write=False)
    return x, init


def distances(x, c, spherical=False):
    """(D fp32 [n][k], D fp64): ((x64[:, None, :] - c64[None]) ** 2).sum(-1)
    (spherical: the fp64 dot products), in row blocks of bounded memory."""
    x64, c64 = x.astype(np.float64), c.astype(np.float64)
    if spherical:
        D64 = x64 @ c64.T
        return D64.astype(np.float32), D64
    n, k = x64.shape[0], c64.shape[0]
    D64 = np.empty((n, k), dtype=np.float64)
    step = max(1, (32 << 20) // (8 * k * x64.shape[1]))
    for r0 in range(0, n, step):
        diff = x64[r0:r0 + step, None, :] - c64[None]
        np.multiply(diff, diff, out=diff)
        D64[r0:r0 + step] = diff.sum(-1)
    return D64.astype(np.float32), D64


def assign(x, c, spherical=False):
    """(assignment int64 [n], its fp32 distances, relative gap to the runner-up
    per row): argmin of the fp32 distances, ties to the smaller id (spherical:
    argmax of the fp32 dot products)."""
    D32, D64 = distances(x, c, spherical)
    a = (D32.argmax(1) if spherical else D32.argmin(1)).astype(np.int64)
    rows = np.arange(x.shape[0])
    if c.shape[0] < 2:
        return a, D32[rows, a], np.full(x.shape[0], np.inf)
    two = np.partition(-D64 if spherical else D64, 1, axis=1)[:, :2]
    gap = (two[:, 1] - two[:, 0]) / np.maximum(np.abs(two[:, 1]), np.finfo(np.float64).tiny)
    return a, D32[rows, a], gap


def split_clusters(c, counts):
    """The empty-cluster rule, in place on the fp32 centroids: returns the repairs."""
    h = counts.astype(np.int64).copy()
    nsplit = 0
    for ci in np.flatnonzero(counts == 0):
        cj = int(np.argmax(h))  # the largest working count, ties to the smaller index
        if h[cj] <= 0:
            break
        c[ci] = c[cj]
        c[ci, 0::2] *= UP
        c[ci, 1::2] *= DOWN
        c[cj, 0::2] *= DOWN
        c[cj, 1::2] *= UP
        h[ci] = h[cj] // 2
        h[cj] -= h[ci]
        nsplit += 1
    return nsplit


def lloyd_step(x, c, spherical=False):
    """One step from the fp32 centroids ``c``: a dict of ``assign``, ``gap``,
    ``counts``, ``sums`` (fp64), ``obj``, ``nsplit`` and the new ``centroids``."""
    k = c.shape[0]
    a, dist, gap = assign(x, c, spherical)
    x64 = x.astype(np.float64)
    counts = np.bincount(a, minlength=k).astype(np.int64)
    sums = np.zeros((k, x.shape[1]), dtype=np.float64)
    order = np.argsort(a, kind="stable")
    bounds = np.concatenate([[0], np.cumsum(counts)])
    for ci in np.flatnonzero(counts):
        sums[ci] = x64[order[bounds[ci]:bounds[ci + 1]]].sum(0)
    new = np.array(c, dtype=np.float32, copy=True)
    nz = counts > 0
    new[nz] = (sums[nz] / counts[nz, None]).astype(np.float32)
    nsplit = split_clusters(new, counts)
    if spherical:
        n64 = new.astype(np.float64)
        nrm = np.sqrt((n64 * n64).sum(1))
        ok = nrm > 0
        new[ok] = (n64[ok] / nrm[ok, None]).astype(np.float32)
    return {"assign": a, "gap": gap, "counts": counts, "sums": sums, "obj": float(dist.astype(np.float64).sum()),
            "nsplit": nsplit, "centroids": new}


def centroid_tol(c_ref, x):
    """One fp32 rounding of two fp64 sums that differ only by summation order."""
    return 2.0 ** -23 * np.abs(c_ref) + 1e-12 * float(np.abs(x).mean())

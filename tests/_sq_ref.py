"""numpy restatement of the scalar quantizer (include/fx_index.h "scalar
quantizer"): train / encode / decode in fp32 with every operation rounded once,
and search as the oracle's exact k-NN over the decoded rows.  Inputs are rounded
to fp32 first.  Also the two clustered corpora the model and GPU tests share."""
import numpy as np

from oracle import flat_l2 as O

QT_8bit, QT_8bit_uniform = 0, 2
f32 = np.float32


def train(x, qtype=QT_8bit):
    """[vmin[d] | vdiff[d]] fp32 (QT_8bit_uniform: equal entries)."""
    x = np.ascontiguousarray(x, dtype=f32)
    d = x.shape[1]
    if qtype == QT_8bit_uniform:
        vmin = np.full(d, x.min(), dtype=f32)
        vmax = np.full(d, x.max(), dtype=f32)
    else:
        vmin, vmax = x.min(axis=0).astype(f32), x.max(axis=0).astype(f32)
    return np.concatenate([vmin, (vmax - vmin).astype(f32)])


def encode(x, trained):
    """faiss's unsigned codes [n][d] uint8."""
    x = np.ascontiguousarray(x, dtype=f32)
    d = x.shape[1]
    vmin, vdiff = trained[:d], trained[d:]
    safe = np.where(vdiff != 0, vdiff, f32(1))
    xi = ((x - vmin[None, :]).astype(f32) / safe[None, :]).astype(f32)
    xi = np.where(vdiff[None, :] != 0, np.clip(xi, f32(0), f32(1)), f32(0)).astype(f32)
    return (f32(255) * xi).astype(f32).astype(np.int32).astype(np.uint8)


def decode(codes, trained):
    """fp32 rows: vmin + ((c + 0.5f) / 255.f) * vdiff, each operation rounded once."""
    codes = np.asarray(codes)
    d = codes.shape[1]
    vmin, vdiff = trained[:d], trained[d:]
    t = ((codes.astype(f32) + f32(0.5)) / f32(255)).astype(f32)
    return (vmin[None, :] + (t * vdiff[None, :]).astype(f32)).astype(f32)


def search(xq, decoded, k, metric=O.METRIC_L2):
    """The oracle's exact k-NN over the decoded rows.  A large problem is first cut
    down per query to its 4 k + 64 nearest rows under an fp64 BLAS distance (whose
    error, ~1e-13, is far below any gap the fp32 ranking can see), kept in row order
    so that ties still go to the smaller row; the oracle then ranks those."""
    xq = np.ascontiguousarray(xq, dtype=f32)
    knn = O.knn_exact if metric == O.METRIC_L2 else O.knn_inner_product
    n, m = decoded.shape[0], 4 * k + 64
    if xq.shape[0] * n * decoded.shape[1] <= 50_000_000 or n <= m:
        return knn(xq, decoded, k)
    q, y = xq.astype(np.float64), decoded.astype(np.float64)
    dist = -(q @ y.T)
    if metric == O.METRIC_L2:
        dist = (q * q).sum(1)[:, None] + 2.0 * dist + (y * y).sum(1)[None, :]
    D = np.empty((xq.shape[0], k), dtype=f32)
    I = np.empty((xq.shape[0], k), dtype=np.int64)
    for i in range(xq.shape[0]):
        cand = np.sort(np.argpartition(dist[i], m)[:m])
        Di, Ii = knn(xq[i:i + 1], decoded[cand], k)
        D[i], I[i] = Di[0], cand[Ii[0]]
    return D, I


def clustered(spread, d=384, n=20000, nq=256, seed=0, ncentres=64):
    """Unit-norm rows and queries around 64 unit-norm cluster centres:
    normalize(centre + spread * g / sqrt(d)), g standard normal."""
    rng = np.random.default_rng(seed)

    def unit(a):
        return a / np.linalg.norm(a, axis=1, keepdims=True)

    centres = unit(rng.standard_normal((ncentres, d)))

    def draw(m):
        c = centres[rng.integers(0, ncentres, m)]
        return unit(c + spread * rng.standard_normal((m, d)) / np.sqrt(d)).astype(f32)

    return draw(n), draw(nq)

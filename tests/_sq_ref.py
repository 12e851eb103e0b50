"""numpy restatement of the scalar quantizer (include/fx_index.h "scalar
quantizer"): train / encode / decode in fp32 with every operation rounded once,
and search as the oracle's exact k-NN over the decoded rows.  Inputs are rounded
to fp32 first.  Also the corpora the model and GPU tests share: the two clustered ones
and the box-corner corpus that drives the int8 accumulators past 2^24."""
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


def corner_corpus(n, nq, d=1100, ncorner=16, seed=3):
    """A corpus whose int8 dots pass 2^24 (possible from d = 1,033 on).

    Rows: standard normal clipped to [-3, 3], with 2 ncorner of them (spread over the whole
    corpus) replaced by the box corners +-3 sgn_i, sgn_i random signs per dimension.  Every
    dimension then trains to vmin = -3, vdiff = 6, and a corner row is all codes 127 / -128.
    Queries: (2.5 +- 0.05) sgn_i, jittered per dimension (first digits |h1| of 118 .. 123 under the
    scale 2^-11 that |x| <= 2.63 keeps: against +-3 sgn_i the first plane's dot is ~ 120.5 * 127.5 *
    d = 1.007 * 2^24 at d = 1100, odd as often as even -- the unjittered 2.5 sgn_i gives an inner-
    product query 120 in every dimension and only even dots), then 3 sgn_i, then the jittered
    queries negated; the rest standard normal.  Needs nq >= 3 ncorner and n >= 2 ncorner."""
    assert nq >= 3 * ncorner and n >= 2 * ncorner
    rng = np.random.default_rng(seed)
    sgn = rng.choice(np.array([-1.0, 1.0], dtype=f32), size=(ncorner, d))
    assert np.unique(sgn, axis=0).shape[0] == ncorner
    xb = np.clip(rng.standard_normal((n, d)), -3.0, 3.0).astype(f32)
    at = np.linspace(0, n - 1, 2 * ncorner).astype(np.int64)  # first and last row included
    xb[at[0::2]] = f32(3) * sgn
    xb[at[1::2]] = f32(-3) * sgn
    xq = rng.standard_normal((nq, d)).astype(f32)
    xq[:ncorner] = (2.5 + 0.05 * rng.uniform(-1.0, 1.0, size=(ncorner, d))).astype(f32) * sgn
    xq[ncorner:2 * ncorner] = f32(3) * sgn
    xq[2 * ncorner:3 * ncorner] = -xq[:ncorner]
    return xb, xq


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

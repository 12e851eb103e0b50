"""numpy restatement of the product quantizer (include/fx_index.h "product
quantizer"): the codec (encode: fp64 argmin with every operation rounded once,
dimensions ascending, the lowest centroid on a tie; decode: a gather), search as
the oracle's exact k-NN over the decoded rows, and the model of k_pq_prep, the
gather scan's key and the bound E (fx_pq.hip).  Also the corpora
the model and GPU tests share."""
import numpy as np
import torch

from oracle import flat_l2 as O
from tests._sq_ref import search  # noqa: F401  (the oracle's exact k-NN over decoded rows, ties to the smaller row)

f32, f64 = np.float32, np.float64
L2, IP = O.METRIC_L2, O.METRIC_INNER_PRODUCT
KSUB, KP, STAGE_D = 256, 32, 32
U = 2.0 ** -24


def kpad(d):
    return (d + STAGE_D - 1) // STAGE_D * STAGE_D


# ---------------------------------------------------------------------------
# codec
# ---------------------------------------------------------------------------
def encode(x, cents):
    """codes [n][M] uint8 of rows x under centroids cents [M][256][dsub] fp32."""
    x = np.ascontiguousarray(x, dtype=f32)
    M, _, dsub = cents.shape
    codes = np.empty((x.shape[0], M), dtype=np.uint8)
    for m in range(M):
        xs = x[:, m * dsub:(m + 1) * dsub].astype(f64)
        c = cents[m].astype(f64)
        acc = np.zeros((x.shape[0], KSUB), dtype=f64)
        for e in range(dsub):  # ascending, one rounding per operation
            df = xs[:, e, None] - c[None, :, e]
            acc = acc + df * df
        codes[:, m] = np.argmin(acc, axis=1)  # the first minimum: the lowest j
    return codes


def decode(codes, cents):
    """fp32 rows: the concatenation of the centroids the codes name."""
    codes = np.asarray(codes)
    return np.concatenate([cents[m][codes[:, m]] for m in range(cents.shape[0])], axis=1).astype(f32)


def row_norms(codes, cents):
    """n_y = |decode|^2: the fp64 sum in dimension order, rounded once."""
    dec = decode(codes, cents).astype(f64)
    acc = np.zeros(dec.shape[0], dtype=f64)
    for j in range(dec.shape[1]):
        acc = acc + dec[:, j] * dec[:, j]
    return acc.astype(f32)


# ---------------------------------------------------------------------------
# the scan's model
# ---------------------------------------------------------------------------
def split(v32):
    """(hi, lo, rest) of fp32 values: hi = rn_bf16(v), rest = v - hi (fp32, exact), lo = rn_bf16(rest)."""
    t = torch.from_numpy(np.ascontiguousarray(v32, dtype=f32))
    hi = t.to(torch.bfloat16).to(torch.float32)
    rest = t - hi
    lo = rest.to(torch.bfloat16).to(torch.float32)
    return hi.numpy(), lo.numpy(), rest.numpy()


def bf16_bits(v32):
    """The bf16 bit patterns of values that are exactly representable."""
    return (np.ascontiguousarray(v32, dtype=f32).view(np.uint32) >> 16).astype(np.uint16)


def constants(cents):
    """(Y, Ry, Yl): max |decode|, max |y - y_hi - y_lo|, max |y_lo| over ANY code row -- the square
    roots of the sums over m of the per-sub-quantizer maxima, times 1 + 1e-9."""
    hi, lo, rest = split(cents)
    c, res, lo = cents.astype(f64), rest.astype(f64) - lo.astype(f64), lo.astype(f64)
    up = 1.0 + 1e-9
    return tuple(float(np.sqrt(((a * a).sum(2)).max(1).sum()) * up) for a in (c, res, lo))


def prep(xq, metric, cents):
    """k_pq_prep: (x_hi, x_lo) [nq][kp] as fp32 values, shift [nq] f64, E [nq] f32."""
    xq = np.ascontiguousarray(xq, dtype=f32)
    nq, d = xq.shape
    kp = kpad(d)
    l2 = metric == L2
    xs = np.zeros((nq, kp), dtype=f32)
    xs[:, :d] = (f32(-2.0) if l2 else f32(-1.0)) * xq
    xs[xs == 0] = f32(0.0)  # zeros as +0, as the padding
    hi, lo, rest = split(xs)
    Y, Ry, Yl = constants(cents)
    xx = (xq.astype(f64) ** 2).sum(1)
    rr = ((rest.astype(f64) - lo.astype(f64)) ** 2).sum(1)
    ll = (lo.astype(f64) ** 2).sum(1)
    nt = 3.0 * kp + 1.0
    gamma = nt * U / (1.0 - nt * U)
    xn = (2.0 if l2 else 1.0) * np.sqrt(xx)
    A = 1.03 * xn * Y
    eps = xn * Ry + np.sqrt(rr) * (Y + Ry) + np.sqrt(ll) * Yl + (gamma + U) * A
    shift = xx if l2 else np.zeros(nq)
    if l2:
        eps = eps + 2.0 * U * Y * Y
    eps = eps + 1e-12 * shift
    return hi, lo, shift, (eps * 1.0625 + 1e-30).astype(f32)


def image_rows(codes, cents):
    """(y_hi, y_lo) [n][kp]: what the gather stages for the rows (zero pieces past d)."""
    dec = decode(codes, cents)
    n, d = dec.shape
    y = np.zeros((n, kpad(d)), dtype=f32)
    y[:, :d] = dec
    hi, lo, _ = split(y)
    return hi, lo


def keys64(xh, xl, yh, yl, ny, metric):
    """The scan's key with its three products summed exactly (fp64): n_y + S (IP: S)."""
    a, b = xh.astype(f64), xl.astype(f64)
    S = a @ yh.astype(f64).T + a @ yl.astype(f64).T + b @ yh.astype(f64).T
    return S + ny.astype(f64)[None, :] if metric == L2 else S


def keys_chain(xh, xl, yh, yl, ny, metric):
    """The same key through a sequential fp32 chain over the 3 K products, stage by stage (a worst
    case for the MFMA's accumulation), and the key's own fp32 addition."""
    nq, kp = xh.shape
    acc = np.zeros((nq, yh.shape[0]), dtype=f32)
    for s0 in range(0, kp, STAGE_D):
        for a, b in ((xh, yh), (xh, yl), (xl, yh)):
            for j in range(s0, s0 + STAGE_D):
                acc = (acc + a[:, j, None] * b[None, :, j]).astype(f32)  # bf16 products are exact in fp32
    return (ny[None, :] + acc).astype(f32) if metric == L2 else acc


def exact64(xq, dec, metric):
    q, y = xq.astype(f64), dec.astype(f64)
    if metric == L2:
        return ((q[:, None, :] - y[None, :, :]) ** 2).sum(2)
    return -(q @ y.T)


def accumulation_term(xq, metric, cents):
    """(gamma_{3K+1} + u) 1.03 |x'| Y + u Y^2: how far a device key may lie from keys64 (the fp32
    accumulation and the key's last addition, u (|S| + n_y); n_y itself is the same rounded value on
    both sides)."""
    d = xq.shape[1]
    Y = constants(cents)[0]
    nt = 3.0 * kpad(d) + 1.0
    gamma = nt * U / (1.0 - nt * U)
    xn = (2.0 if metric == L2 else 1.0) * np.sqrt((xq.astype(f64) ** 2).sum(1))
    return (gamma + U) * 1.03 * xn * Y + (U * Y * Y if metric == L2 else 0.0)


def certified(kth, tb, shift, eps):
    """sq_certified with rho = 0 (fx_sq_common.h)."""
    kup = float(kth) + abs(float(kth)) * 2.384185791015625e-7
    return kup < float(tb) + float(shift) - float(eps)


def uncertified(keys, xq, dec, metric, shift, eps, k, splits=1):
    """Queries k_pq_refine would flag: per split of the rows (whole 128-row tiles, the kernel's
    division) the KP best (key, row); merged, their KP best re-ranked exactly; certified when the
    k-th exact key lies below the merged list's KP-th scan key + shift - E.  Fewer than KP
    candidates in all: nothing was dropped, certified."""
    nq, n = keys.shape
    nct = (n + 127) // 128
    bounds = [min(n, (s * nct // splits) * 128) for s in range(splits)] + [n]
    flagged = 0
    for q in range(nq):
        cand = []
        for s in range(splits):
            a, b = bounds[s], bounds[s + 1]
            order = np.lexsort((np.arange(a, b), keys[q, a:b]))[:KP]
            cand += [(float(keys[q, a + i]), a + int(i)) for i in order]
        cand.sort()
        if len(cand) < KP:
            continue
        top = cand[:KP]
        rows = np.array([r for _, r in top])
        ex = exact64(xq[q:q + 1], dec[rows], metric)[0].astype(f32)
        kth = np.sort(ex)[k - 1]
        if not certified(kth, top[KP - 1][0], shift[q], eps[q]):
            flagged += 1
    return flagged


# ---------------------------------------------------------------------------
# corpora
# ---------------------------------------------------------------------------
def clustered(d, n, nq, seed=0, ncentres=16, spread=0.3, scale=1.0):
    """Unit-norm rows and queries around unit-norm cluster centres, times `scale`."""
    rng = np.random.default_rng(seed)

    def unit(a):
        return a / np.linalg.norm(a, axis=1, keepdims=True)

    centres = unit(rng.standard_normal((ncentres, d)))

    def draw(m):
        c = centres[rng.integers(0, ncentres, m)]
        return (scale * unit(c + spread * rng.standard_normal((m, d)) / np.sqrt(d))).astype(f32)

    return draw(n), draw(nq)


def sampled_centroids(x, M, seed=1):
    """Centroids [M][256][dsub] drawn from the rows' own subvectors (with repetition when the
    corpus has fewer than 256 rows): a codebook that fits the data, no training needed."""
    rng = np.random.default_rng(seed)
    n, d = x.shape
    dsub = d // M
    pick = np.stack([rng.choice(n, size=KSUB, replace=n < KSUB) for _ in range(M)])
    return np.stack([x[pick[m], m * dsub:(m + 1) * dsub] for m in range(M)]).astype(f32)

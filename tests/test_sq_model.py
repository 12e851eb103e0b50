"""The scalar-quantizer scan in numpy: the query operand as
three int8 digit planes with a per-query power-of-two scale, the integer dots,
the key formed in fp32 as k_sq_scan's epilogue forms it, and the bound E
restated from k_sq_prep (csrc/fx_sq.hip; keep the two in step).

Asserted for every (query, row) pair: the scan key plus the query's shift is
within E of the exact fp64 key of the DECODED fp32 row,

    L2   | key + |z|^2 - D | <= E          IP   | key - x.m + x.y | <= E

and that every query certifies at k = 1 and k = 10 against its 32nd key by the
refine's own test.  (What is PROVED for L2 is E + 2 rho_dec sqrt(D): the decoded
fp32 row differs from the affine model m + s c' by the decode's own roundings,
at most rho_dec in norm, which is a term of the 2 rho sqrt(D) form and is what
the refine's certification takes it as.  The assertion here is the stricter E
alone; the observed error stays below 0.3 E.)"""
import numpy as np
import pytest

from tests import _sq_ref as R

U = 2.0 ** -24


def index_consts(trained, codes_u8):
    """What the index keeps: s, m, the rows' n_c (fp64 sum rounded once), max n_c,
    max sum c'^2 and the decode bound rho_dec (k_sq_consts)."""
    d = codes_u8.shape[1]
    vmin, vdiff = trained[:d].astype(np.float64), trained[d:].astype(np.float64)
    s = vdiff / 255.0
    m = vmin + 128.5 * s
    cs = codes_u8.astype(np.int64) - 128
    nc = ((s[None, :] * cs) ** 2).sum(axis=1).astype(np.float32)
    c2max = int((cs * cs).sum(axis=1).max())
    dj = U * (2.0 * vdiff + np.maximum(np.abs(vmin), np.abs(vmin + vdiff))) * 1.001 + 1e-44
    rho_dec = float(np.float32(np.sqrt((dj * dj).sum()) * 1.000001))
    return s, m, cs, nc, float(nc.max()), c2max, rho_dec


def digit(r):
    return np.clip(np.rint(r), -127.0, 127.0)


def prep(xq, s, m, metric_l2, M2, c2max, rho_dec):
    """k_sq_prep: planes, sigma, shift and E per query."""
    x = xq.astype(np.float64)
    z = x - m[None, :] if metric_l2 else x
    w = z * s[None, :]
    wmax = np.abs(w).max(axis=1)
    sg = np.ones(len(x))
    for i, v in enumerate(wmax):
        if v > 0:
            f, e = np.frexp(v / 127.0)
            sg[i] = np.ldexp(1.0, int(np.clip(e - 1 if f == 0.5 else e, -120, 120)))
    r1 = w / sg[:, None]
    h1 = digit(r1)
    r2 = (r1 - h1) * 256.0
    h2 = digit(r2)
    r3 = (r2 - h2) * 256.0
    h3 = digit(r3)
    res = (r3 - h3) * (sg[:, None] / 65536.0)
    rp = np.sqrt((res * res).sum(axis=1))
    C = np.sqrt(float(c2max))
    H = np.sqrt((h1 * h1).sum(1)) + np.sqrt((h2 * h2).sum(1)) / 256.0 + np.sqrt((h3 * h3).sum(1)) / 65536.0
    A = sg * H * C
    if metric_l2:
        sh = (z * z).sum(axis=1)
        eps = 2.0 * rp * C + U * (2.0 * M2 + 8.0 * A) * 1.01 + rho_dec * rho_dec + 1e-12 * sh
        shift = sh
    else:
        sh = (x * m[None, :]).sum(axis=1)
        eps = rp * C + 3.0 * U * A * 1.01 + np.sqrt((x * x).sum(axis=1)) * rho_dec + 1e-12 * np.abs(sh)
        shift = -sh
    E = (eps * 1.0625 + 1e-30).astype(np.float32)
    return (h1.astype(np.int64), h2.astype(np.int64), h3.astype(np.int64)), sg.astype(np.float32), shift, E


def int_dots(planes, cs):
    """The three i32 accumulators of every (query, row): exact integer dots."""
    return [(h @ cs.T) for h in planes]


def inexact_conversions(a):
    """Entries of an accumulator past the fp32 integer range (|a| > 2^24) that f32(a) rounds."""
    a = np.asarray(a)
    return int(((np.abs(a) > 2 ** 24) & (a.astype(np.float32).astype(np.float64) != a.astype(np.float64))).sum())


def scan_keys(planes, sg, cs, nc, metric_l2):
    """k_sq_scan's epilogue in fp32: exact integer dots, f32(acc) conversions,
    two fused multiply-adds by powers of two, one for the key."""
    a = int_dots(planes, cs)
    f = [x.astype(np.float32) for x in a]
    t1 = (f[1].astype(np.float64) / 256.0 + f[0].astype(np.float64)).astype(np.float32)      # fmaf: one rounding
    t2 = (f[2].astype(np.float64) / 65536.0 + t1.astype(np.float64)).astype(np.float32)
    scale = (-2.0 if metric_l2 else -1.0) * sg.astype(np.float64)[:, None]
    if metric_l2:
        return (scale * t2.astype(np.float64) + nc.astype(np.float64)[None, :]).astype(np.float32)
    return (scale * t2.astype(np.float64)).astype(np.float32)


def certified(kth, tb, shift, eps, rho):
    """sq_certified of fx_sq.hip."""
    T = float(tb) + shift - float(eps)
    dmin = T
    if rho > 0.0:
        t = max(T, 0.0)
        sd = t / (np.sqrt(rho * rho + t) + rho)
        dmin = sd * sd * (1.0 - 1e-12)
    kup = float(kth) + abs(float(kth)) * 2.384185791015625e-7
    return kup < dmin


def run_model(xb, xq, metric_l2):
    trained = R.train(xb)
    codes = R.encode(xb, trained)
    y = R.decode(codes, trained).astype(np.float64)
    s, m, cs, nc, M2, c2max, rho_dec = index_consts(trained, codes)
    planes, sg, shift, E = prep(xq, s, m, metric_l2, M2, c2max, rho_dec)
    keys = scan_keys(planes, sg, cs, nc, metric_l2).astype(np.float64)
    x = xq.astype(np.float64)
    if metric_l2:
        exact = ((x * x).sum(1)[:, None] - 2.0 * x @ y.T + (y * y).sum(1)[None, :])
        # (the expansion is only the model's reference for the bound; recompute the small ones directly)
        exact = np.maximum(exact, 0.0)
        near = np.argsort(exact, axis=1)[:, :64]
        for i in range(len(x)):
            df = x[i][None, :] - y[near[i]]
            exact[i, near[i]] = (df * df).sum(1)
        err = np.abs(keys + shift[:, None] - exact)
        bound = E.astype(np.float64)[:, None] + 1e-13 * (1.0 + exact)  # (the slack: this fp64 reference's own rounding)
    else:
        exact = -(x @ y.T)
        err = np.abs(keys + shift[:, None] - exact)
        bound = E.astype(np.float64)[:, None] + 1e-13 * (1.0 + np.abs(exact))
    return keys, exact, err, bound, shift, E, (rho_dec if metric_l2 else 0.0)


def certify_all(keys, exact, shift, E, rho, k):
    """Every query: the exact k-th key (fp32) against the 32nd scan key."""
    n = 0
    for i in range(keys.shape[0]):
        tb = np.float32(np.sort(keys[i])[31])
        best = np.sort(exact[i, np.argsort(keys[i], kind="stable")[:32]].astype(np.float32))
        n += bool(certified(best[k - 1], tb, shift[i], E[i], rho))
    return n


@pytest.fixture(scope="module")
def corpora():
    return {sp: R.clustered(sp) for sp in (0.1, 0.02)}


@pytest.mark.parametrize("spread", [0.1, 0.02])
@pytest.mark.parametrize("metric_l2", [True, False], ids=["L2", "IP"])
def test_key_within_the_bound_on_the_clustered_corpora(corpora, spread, metric_l2):
    xb, xq = corpora[spread]
    keys, exact, err, bound, shift, E, rho = run_model(xb, xq, metric_l2)
    worst = float((err / bound).max())
    print(f"spread {spread} {'L2' if metric_l2 else 'IP'}: E median {np.median(E):.3g}, worst error / bound {worst:.3f}")
    assert (err <= bound).all()
    if spread == 0.1 or metric_l2:
        for k in (1, 10):
            assert certify_all(keys, exact, shift, E, rho, k) == len(xq), f"k = {k}"


def test_key_within_the_bound_past_the_exact_accumulator_range():
    """d = 1100: past d = 1032 an accumulator can pass 2^24, so f32(acc) may round."""
    rng = np.random.default_rng(1)
    xb = rng.standard_normal((2000, 1100)).astype(np.float32)
    xq = rng.standard_normal((32, 1100)).astype(np.float32)
    for metric_l2 in (True, False):
        _, _, err, bound, _, _, _ = run_model(xb, xq, metric_l2)
        assert (err <= bound).all()


@pytest.mark.parametrize("metric_l2", [True, False], ids=["L2", "IP"])
def test_key_within_the_bound_where_an_accumulator_passes_2_24(metric_l2):
    """The standard normal rows of the test above stay 36 times short of 2^24 (max |a| ~ 4.6e5), so
    f32(acc) never rounds there.  tests/_sq_ref.corner_corpus does pass it: the precondition asserted
    first is a (query, row) pair with |a1| > 2^24 whose fp32 conversion is inexact, the 6 u A term of
    the bound."""
    xb, xq = R.corner_corpus(2000, 48)
    trained = R.train(xb)
    s, m, cs, nc, M2, c2max, rho_dec = index_consts(trained, R.encode(xb, trained))
    planes, _, _, _ = prep(xq, s, m, metric_l2, M2, c2max, rho_dec)
    a = int_dots(planes, cs)
    amax = [int(np.abs(x).max()) for x in a]
    rounded = inexact_conversions(a[0])
    print(f"{'L2' if metric_l2 else 'IP'}: max |a1|, |a2|, |a3| = {amax}, f32(a1) != a1 for {rounded} of {a[0].size} pairs")
    assert amax[0] > 2 ** 24 and rounded >= 1, "the corpus does not reach the accumulator's inexact fp32 range"
    keys, exact, err, bound, shift, E, rho = run_model(xb, xq, metric_l2)
    print(f"worst error / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all()

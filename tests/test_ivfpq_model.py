"""The IndexIVFPQ list scan in numpy: operand preparation per (query, probe) pair
with the list's centroid folded in, the key k_ivfpq_scan's epilogue forms (the gather model of
tests/_pq_ref.py, then the pair's fp32 shift in one more rounded addition), the pair's bound E
restated from k_ivfpq_prep, and the refine's merge and certification over a query's slots
(csrc/fx_ivfpq.hip; keep the two in step).

Asserted on the corpora the GPU tests use (tests/test_ivfpq_gpu.py):

  bound    | key - exact | <= E + 2 rho_dec sqrt(D) for every (pair, row of the pair's list) (IP: E),
           where key already carries the shift and exact is the fp64 key of the decoded fp32 row;
           through the exactly summed key (keys64) and through the sequential fp32 chain;
  ids      every query the model certifies has exactly the reference's ids;
  a condition, not a measurement: at k = 10 the model certifies at least 90 % of the queries;
  at k = 32 every query with 32 candidate rows or more is flagged."""
import functools

import numpy as np
import pytest

from tests import _ivf_ref as IV
from tests import _ivfpq_ref as R
from tests import _pq_ref as PQ
from tests.test_ivfsq_model import chunk_rows, groups_corpus, long_corpus, plan_chunks

L2, IP = R.METRIC_L2, R.METRIC_INNER_PRODUCT
KP, TILE = 32, 128
U = PQ.U
f32, f64 = np.float32, np.float64

FUSED_SHAPES = [(16, 2), (384, 48), (384, 24), (1096, 137)]


def rho_dec(cent, cents):
    """The rounding bound of y = fl32(c_l + decode): per dimension u (max_l |c_lj| + max_j |centroid
    value|), root of the sum of squares (fx_ivfpq_set_centroids)."""
    M, _, dsub = cents.shape
    cmax = np.abs(cent.astype(f64)).max(axis=0)
    ymax = np.abs(cents.astype(f64)).max(axis=1).reshape(M * dsub)
    dj = U * (cmax + ymax) * 1.001
    return float(np.sqrt((dj * dj).sum()) * 1.000001)


def certified(kth, tb, eps, rho):
    """sq_certified with shift 0 (fx_sq_common.h)."""
    T = float(tb) - float(eps)
    dmin = T
    if rho > 0.0:
        t = max(T, 0.0)
        sd = t / (np.sqrt(rho * rho + t) + rho)
        dmin = sd * sd * (1.0 - 1e-12)
    kup = float(kth) + abs(float(kth)) * 2.384185791015625e-7
    return kup < dmin


def prep_pairs(x, cl, metric_l2, consts, rdec):
    """k_ivfpq_prep for pair rows: x [npairs][d] the pair's query (fp32), cl [npairs][d] the pair's
    fp32 centroid or None.  (x_hi, x_lo) [npairs][kp] as fp32 values, the fp64 shift and E per pair."""
    Y, Ry, Yl = consts
    n, d = x.shape
    kp = PQ.kpad(d)
    x64 = x.astype(f64)
    xx = (x64 * x64).sum(1)
    folded = metric_l2 and cl is not None
    z = (x - cl).astype(f32) if folded else x
    xs = np.zeros((n, kp), dtype=f32)
    xs[:, :d] = (f32(-2.0) if metric_l2 else f32(-1.0)) * z
    xs[xs == 0] = f32(0.0)
    hi, lo, rest = PQ.split(xs)
    rr = ((rest.astype(f64) - lo.astype(f64)) ** 2).sum(1)
    ll = (lo.astype(f64) ** 2).sum(1)
    zz = (z.astype(f64) ** 2).sum(1)
    if folded:
        w = x64 - cl.astype(f64)
        sh = (w * w).sum(1)
    elif metric_l2:
        sh = xx
    elif cl is not None:
        sh = -(x64 * cl.astype(f64)).sum(1)
    else:
        sh = np.zeros(n)
    nt = 3.0 * kp + 1.0
    gamma = nt * U / (1.0 - nt * U)
    xn = (2.0 if metric_l2 else 1.0) * np.sqrt(zz)
    A = 1.03 * xn * Y
    eps = xn * Ry + np.sqrt(rr) * (Y + Ry) + np.sqrt(ll) * Yl + (gamma + U) * A
    if metric_l2:
        eps = eps + 2.0 * U * Y * Y
    eps = eps + U * (2.0 * np.abs(sh) + (Y * Y if metric_l2 else 0.0) + A) * 1.01
    if folded:
        eps = eps + U * xn * Y * 1.01
    eps = eps + (rdec * rdec if metric_l2 else np.sqrt(xx) * rdec)
    eps = eps + 1e-12 * np.abs(sh)
    return hi, lo, sh, (eps * 1.0625 + 1e-30).astype(f32)


class ScanModel:
    """The model of one index and one query batch: everything that belongs to a (query, list) pair,
    for every list a query can probe (pair (q, j) probes the j-th list of the full coarse ranking,
    of which a search with nprobe uses the first nprobe)."""

    def __init__(self, cent, xb, lists, xq, metric, M, by_residual=True, chain=False):
        self.l2 = metric == L2
        self.metric = metric
        self.cent = np.asarray(cent, dtype=f32)
        self.cents = R.codebook(xb, lists, cent, M, by_residual)
        self.ref = R.Model(xb, lists, cent, self.cents, by_residual)
        self.nlist, self.d = self.cent.shape
        self.xq = np.ascontiguousarray(xq, dtype=f32)
        self.nq = self.xq.shape[0]
        self.order = IV.store_order(lists)
        ls = np.asarray(lists)[self.order]
        self.off = np.searchsorted(ls, np.arange(self.nlist + 1))
        self.ys = np.ascontiguousarray(self.ref.y[self.order])
        self.codes_s = np.ascontiguousarray(self.ref.codes[self.order])
        self.ny = PQ.row_norms(self.codes_s, self.cents)
        self.yh, self.yl = PQ.image_rows(self.codes_s, self.cents)
        self.consts = PQ.constants(self.cents.copy())
        self.rho_dec = rho_dec(self.cent, self.cents) if by_residual else 0.0
        self.rho = self.rho_dec if self.l2 else 0.0
        self.P = IV.probe(self.xq, self.cent, self.nlist, metric)  # [nq][nlist]
        x = np.repeat(self.xq, self.nlist, axis=0)
        cl = self.cent[self.P.reshape(-1)] if by_residual else None
        self.xh, self.xl, self.shift, self.E = prep_pairs(x, cl, self.l2, self.consts, self.rho_dec)
        self.shift32 = self.shift.astype(f32)
        nt = 3.0 * PQ.kpad(self.d) + 1.0
        self.gamma = nt * U / (1.0 - nt * U)
        # keys and exact values per list: pairs idx[l] (flat pair numbers of the full ranking) x rows of l
        self.key64, self.key0, self.keyc, self.exact, self.idx = {}, {}, {}, {}, {}
        flat = self.P.reshape(-1)
        x64 = x.astype(f64)
        for l in range(self.nlist):
            r0, r1 = self.off[l], self.off[l + 1]
            idx = np.flatnonzero(flat == l)
            self.idx[l] = idx
            if r1 == r0 or idx.size == 0:
                continue
            ops = (self.xh[idx], self.xl[idx], self.yh[r0:r1], self.yl[r0:r1], self.ny[r0:r1])
            k64 = PQ.keys64(*ops, metric)
            self.key64[l] = k64 + self.shift[idx][:, None]
            # the device's form with S rounded once: fl(n_y + fl(S)) (IP: fl(S))
            S = (k64 - self.ny[r0:r1].astype(f64)[None, :]) if self.l2 else k64
            S32 = S.astype(f32)
            self.key0[l] = (self.ny[r0:r1][None, :] + S32).astype(f32) if self.l2 else S32
            if chain:
                self.keyc[l] = PQ.keys_chain(*ops, metric)
            yy = self.ys[r0:r1].astype(f64)
            ex = np.empty((idx.size, r1 - r0))
            for i, p in enumerate(idx):
                ex[i] = ((x64[p][None, :] - yy) ** 2).sum(1) if self.l2 else -(yy @ x64[p])
            self.exact[l] = ex
        self.keys = {l: (k0 + self.shift32[self.idx[l]][:, None]).astype(f32) for l, k0 in self.key0.items()}
        self.keys_chain = {l: (kc + self.shift32[self.idx[l]][:, None]).astype(f32) for l, kc in self.keyc.items()}

    def pair(self, q, j):
        return q * self.nlist + j

    def pair_keys(self, q, j):
        """(row0, keys, exact) of pair (q, j) over its list's rows."""
        l = int(self.P[q, j])
        if l not in self.keys:
            return int(self.off[l]), np.zeros(0, f32), np.zeros(0)
        i = int(np.searchsorted(self.idx[l], self.pair(q, j)))
        return int(self.off[l]), self.keys[l][i], self.exact[l][i]

    def pair_slack(self, q, j):
        """The accumulation term of pair (q, j): (gamma_{3K+1} + u) 1.03 |x'| Y + u Y^2 + u |key|."""
        p = self.pair(q, j)
        Y = self.consts[0]
        xn = float(np.sqrt(((self.xh[p].astype(f64) + self.xl[p].astype(f64)) ** 2).sum())) * 1.01
        return (self.gamma + U) * 1.03 * xn * Y + (U * Y * Y if self.l2 else 0.0) + 2.0 * U * abs(float(self.shift[p]))

    def slot(self, q, j, C, c):
        """The list k_ivfpq_scan leaves in slot j * C + c of query q: (keys, rows), the first KP of the
        chunk's rows by (key, row)."""
        r0, keys, _ = self.pair_keys(q, j)
        a, b = chunk_rows(r0, r0 + keys.size, C)[c]
        sub = keys[a - r0:b - r0]
        o = np.argsort(sub, kind="stable")[:KP]
        return sub[o], o + a

    def refine(self, q, nprobe, C, k, escale=1.0, tslack=0.0):
        """k_ivfpq_refine for query q: (flagged, rows of its top k by (exact fp32 key, row)).  tslack
        (in units of the query's largest accumulation term) moves the merged list's KP-th key."""
        ks, rs = [], []
        npr = min(nprobe, self.nlist)
        for j in range(npr):
            for c in range(C):
                kk, rr = self.slot(q, j, C, c)
                ks.append(kk)
                rs.append(rr)
        ks, rs = np.concatenate(ks), np.concatenate(rs)
        o = np.lexsort((rs, ks))[:KP]
        mk, mr = ks[o], rs[o]
        x = self.xq[q].astype(f64)
        y = self.ys[mr].astype(f64)
        ex = (((x[None, :] - y) ** 2).sum(1) if self.l2 else -(y @ x)).astype(f32)
        o2 = np.lexsort((mr, ex))
        top = mr[o2][:k]
        flagged = False
        if ks.size >= KP:
            kth = ex[o2][k - 1] if k <= ex.size else np.inf
            Eq = float(self.E[q * self.nlist:q * self.nlist + npr].max()) * escale
            tb = float(mk[KP - 1])
            if tslack != 0.0:
                tb += tslack * max(self.pair_slack(q, j) for j in range(npr))
            flagged = not certified(kth, tb, Eq, self.rho)
        return flagged, top

    def flagged_range(self, nprobe, C, k):
        """(lo, hi): the count of uncertified queries with E scaled by 1 -+ 1e-5 (the device's E is the
        same fp64 formula summed in another order) and the merged list's last key moved by the
        accumulation term (the MFMA sums the same products in another order)."""
        lo = sum(self.refine(q, nprobe, C, k, 1.0 - 1e-5, +1.0)[0] for q in range(self.nq))
        hi = sum(self.refine(q, nprobe, C, k, 1.0 + 1e-5, -1.0)[0] for q in range(self.nq))
        return lo, hi

    def candidates(self, q, nprobe):
        """Rows in the query's first nprobe probed lists."""
        return int(sum(self.off[l + 1] - self.off[l] for l in self.P[q, :min(nprobe, self.nlist)]))

    def max_list_rows(self):
        return int(np.diff(self.off).max())


@functools.lru_cache(maxsize=4)
def edge_model(d, M, metric, by_residual, chain=False):
    c, xb, lists, xq = IV.edge_corpus(d, "float32")
    return ScanModel(c, xb, lists, xq, metric, M, by_residual, chain=chain)


def check_bound(m):
    """The bound for every (pair, row), through keys64, the once-rounded key and (when built) the
    sequential fp32 chain; returns the worst error / bound."""
    worst = 0.0
    for l, ex in m.exact.items():
        E = m.E[m.idx[l]].astype(f64)[:, None]
        bound = E + 1e-13 * (1.0 + np.abs(ex))  # (the slack: this fp64 reference's own rounding)
        if m.l2:
            bound = bound + 2.0 * m.rho_dec * np.sqrt(ex)
        for name, keys in (("keys64", m.key64[l]), ("rounded", m.keys[l]), ("chain", m.keys_chain.get(l))):
            if keys is None:
                continue
            err = np.abs(keys.astype(f64) - ex)
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), f"list {l} ({name}): {float((err / bound).max())}"
    return worst


def check_certified(m, ids, nprobe, C, k):
    """Every query the model certifies has the reference's ids; returns the certified count."""
    Dr, Ir = m.ref.search(m.xq, ids, k, nprobe, m.metric)
    ids_s = np.asarray(ids)[m.order]
    n = 0
    for q in range(m.nq):
        flagged, top = m.refine(q, nprobe, C, k)
        if flagged:
            continue
        n += 1
        want = Ir[q][Ir[q] >= 0]
        assert (ids_s[top] == want).all(), f"query {q}: a certified query with the wrong ids"
    return n


@pytest.mark.parametrize("by_residual", [True, False], ids=["residual", "plain"])
@pytest.mark.parametrize("metric", [L2, IP], ids=["L2", "IP"])
@pytest.mark.parametrize("d,M", FUSED_SHAPES)
def test_edge_corpus(d, M, metric, by_residual):
    m = edge_model(d, M, metric, by_residual, chain=d <= 384)
    worst = check_bound(m)
    ids = np.arange(m.order.size, dtype=np.int64)
    out = []
    for nprobe in (1, 3, 12):
        C = plan_chunks(m.nq, nprobe, m.max_list_rows())
        for k in (1, 10):
            n = check_certified(m, ids, nprobe, C, k)
            out.append((nprobe, C, k, n))
            if k == 10:
                assert n >= 0.9 * m.nq, f"nprobe {nprobe} k {k}: only {n} of {m.nq} queries certify"
        for q in range(m.nq):  # k = KP: the k-th exact key is the kept list's last
            if m.candidates(q, nprobe) >= KP:
                assert m.refine(q, nprobe, C, KP)[0], f"nprobe {nprobe} query {q}: certified at k = 32"
    print(f"d {d} M {M} {'L2' if metric == L2 else 'IP'} by_residual {by_residual}: E median {np.median(m.E):.3g}, "
          f"rho_dec {m.rho_dec:.3g}, worst error / bound {worst:.3f}, certified (nprobe, C, k, n of {m.nq}) {out}")


def test_more_than_one_pair_group():
    c, xb, lists, xq = groups_corpus()
    assert (IV.assign(xq, c, L2) == np.asarray(IV.probe(xq, c, 1, L2))[:, 0]).all()
    m = ScanModel(c, xb, lists, xq, L2, 48)
    check_bound(m)
    n = check_certified(m, np.arange(xb.shape[0], dtype=np.int64), 2, 1, 10)
    assert n >= 0.9 * m.nq, n
    assert (m.P[:, 0] == 11).sum() >= 300 > TILE


@pytest.mark.parametrize("nq", [1, 5])
def test_chunked_long_list(nq):
    c, xb, lists, xq = long_corpus(nq)
    m = ScanModel(c, xb, lists, xq, L2, 48)
    check_bound(m)
    C = plan_chunks(nq, 1, m.max_list_rows())
    assert C > 1
    # the chunks tile the list: every row in exactly one
    r0, r1 = int(m.off[0]), int(m.off[1])
    cover = np.zeros(r1 - r0, dtype=int)
    for a, b in chunk_rows(r0, r1, C):
        cover[a - r0:b - r0] += 1
    assert (cover == 1).all()
    n = check_certified(m, np.arange(xb.shape[0], dtype=np.int64), 1, C, 10)
    assert n >= 0.9 * nq, n


def test_shift_in_the_key_costs_what_the_bound_says():
    """The terms the pair's E gains over 3.16's: fl32(shift), the one addition, and (L2 with
    by_residual) the rounding of the operand's fl32(x - c_l) against the exact shift."""
    m = edge_model(384, 48, L2, True)
    Y = m.consts[0]
    for l, keys in m.keys.items():
        idx = m.idx[l]
        exact_sum = m.key0[l].astype(f64) + m.shift[idx][:, None]
        err = np.abs(keys.astype(f64) - exact_sum)
        A2 = np.abs(m.key0[l]).max()
        assert (err <= U * (2.0 * np.abs(m.shift[idx])[:, None] + A2) * 1.01).all()
        # |a| <= Y^2 + 1.03 |x'| Y, what E charges for the addition
        xn = np.sqrt(((m.xh[idx].astype(f64) + m.xl[idx].astype(f64)) ** 2).sum(1))
        assert (np.abs(m.key0[l]) <= (Y * Y + 1.03 * xn * Y * 1.01)[:, None]).all()

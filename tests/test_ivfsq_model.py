"""The IndexIVFScalarQuantizer list scan in numpy: operand preparation per (query,
probe) pair with the list's centroid folded in, the key k_ivfsq_scan's epilogue forms (the int8
model of tests/test_sq_model.py, then the pair's fp32 shift in one more rounded addition), the
pair's bound E restated from k_ivfsq_prep, and the refine's merge and certification over a
query's slots (csrc/fx_ivfsq.hip; keep the two in step).

Asserted on the corpora the GPU tests use (tests/test_ivfsq_gpu.py; those whose centroids are
given -- the two that train k-means on the device assert nothing about certification):

  bound    | key - exact | <= E + 2 rho_dec sqrt(D) for every (pair, row of the pair's list) (IP: E),
           where key already carries the shift and exact is the fp64 key of the decoded fp32 row;
  ids      every query the model certifies has exactly the reference's ids;
  a condition, not a measurement: at k = 10 the model certifies at least 90 % of the queries."""
import functools

import numpy as np
import pytest

from tests import _ivf_ref as IV
from tests import _ivfsq_ref as R
from tests import _kmeans_ref as kref
from tests.test_sq_model import U, certified, digit, index_consts as sq_index_consts, scan_keys

L2, IP = R.METRIC_L2, R.METRIC_INNER_PRODUCT
KP, TILE = 32, 128
f32 = np.float32


def index_consts(trained, codes_u8, cent):
    """test_sq_model.index_consts with k_ivfsq_consts' rho_dec: the centroid's addition costs u (max_l
    |c_lj| + max |decode_j|) per dimension on top of the decode's own roundings."""
    s, m, cs, nc, M2, c2max, rho = sq_index_consts(trained, codes_u8)
    if cent is not None:
        d = codes_u8.shape[1]
        vmin, vdiff = trained[:d].astype(np.float64), trained[d:].astype(np.float64)
        ymax = np.maximum(np.abs(vmin), np.abs(vmin + vdiff))
        cmax = np.abs(cent.astype(np.float64)).max(axis=0)
        dj = U * (2.0 * vdiff + ymax) * 1.001 + 1e-44 + U * (cmax + ymax * 1.000001) * 1.001
        rho = float(f32(np.sqrt((dj * dj).sum()) * 1.000001))
    return s, m, cs, nc, M2, c2max, rho


def prep_pairs(x, mt, s, metric_l2, M2, c2max, rho_dec):
    """k_ivfsq_prep for pair rows: x [npairs][d] the pair's query, mt [npairs][d] = m + c_l in fp64
    (m alone without by_residual).  Planes, sigma, the fp64 shift and E per pair."""
    x = x.astype(np.float64)
    z = x - mt if metric_l2 else x
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
        eps = (2.0 * rp * C + U * (2.0 * M2 + 8.0 * A) * 1.01 + rho_dec * rho_dec + 1e-12 * sh +
               U * (2.0 * sh + M2 + 2.0 * A) * 1.01)
        shift = sh
    else:
        sh = (x * mt).sum(axis=1)
        eps = (rp * C + 3.0 * U * A * 1.01 + np.sqrt((x * x).sum(axis=1)) * rho_dec + 1e-12 * np.abs(sh) +
               U * (2.0 * np.abs(sh) + A) * 1.01)
        shift = -sh
    E = (eps * 1.0625 + 1e-30).astype(f32)
    return (h1, h2, h3), sg.astype(f32), shift, E


def plan_chunks(nq, nprobe, max_list_rows):
    """plan_ivf's chunk count (csrc/fx_plan.cpp)."""
    pairs = max(nq, 1) * nprobe
    tiles = (max(max_list_rows, 0) + TILE - 1) // TILE + 1
    if pairs >= 256:
        return 1
    return max(1, min((512 + pairs - 1) // pairs, max(1, tiles // 4), 64))


def chunk_rows(r0, r1, C):
    """The rows of list [r0, r1) each of k_ivfsq_scan's C chunks covers: tiles of 128 rows from the
    list's start aligned down to 4 rows, divided evenly by tile count."""
    a0 = r0 & ~3
    nt = (r1 - a0 + TILE - 1) // TILE
    out = []
    for c in range(C):
        t0, t1 = nt * c // C, nt * (c + 1) // C
        out.append((max(r0, a0 + t0 * TILE), min(r1, a0 + t1 * TILE)) if r1 > r0 and t1 > t0 else (r0, r0))
    return out


class ScanModel:
    """The model of one index and one query batch: everything that belongs to a (query, list) pair,
    for every list a query can probe (pair (q, j) probes the j-th list of the full coarse ranking,
    of which a search with nprobe uses the first nprobe)."""

    def __init__(self, cent, xb, lists, xq, metric, qtype=R.QT_8bit, by_residual=True, trained=None):
        self.l2 = metric == L2
        self.metric = metric
        self.ref = R.Model(xb, lists, cent, qtype, by_residual)
        if trained is not None:
            assert (np.asarray(trained) == self.ref.trained).all()
        self.cent = np.asarray(cent, dtype=f32)
        self.nlist, self.d = self.cent.shape
        self.xq = np.ascontiguousarray(xq, dtype=f32)
        self.nq = self.xq.shape[0]
        self.order = IV.store_order(lists)
        ls = np.asarray(lists)[self.order]
        self.off = np.searchsorted(ls, np.arange(self.nlist + 1))
        self.ys = np.ascontiguousarray(self.ref.y[self.order])
        codes_s = self.ref.codes[self.order]
        (self.s, self.m, cs, self.nc, self.M2, self.c2max, self.rho_dec) = index_consts(
            self.ref.trained, codes_s, self.cent if by_residual else None)
        self.rho = self.rho_dec if self.l2 else 0.0
        self.P = IV.probe(self.xq, self.cent, self.nlist, metric)  # [nq][nlist]
        npairs = self.nq * self.nlist
        x = np.repeat(self.xq.astype(np.float64), self.nlist, axis=0)
        mt = np.broadcast_to(self.m[None, :], (npairs, self.d))
        if by_residual:
            mt = self.m[None, :] + self.cent[self.P.reshape(-1)].astype(np.float64)
        self.planes, self.sg, self.shift, self.E = prep_pairs(x, mt, self.s, self.l2, self.M2, self.c2max,
                                                              self.rho_dec)
        self.shift32 = self.shift.astype(f32)
        # keys and exact values per list: pairs idx[l] (flat pair numbers of the full ranking) x rows of l
        self.keys, self.key0, self.exact, self.idx = {}, {}, {}, {}
        csf = cs.astype(np.float64)
        flat = self.P.reshape(-1)
        for l in range(self.nlist):
            r0, r1 = self.off[l], self.off[l + 1]
            idx = np.flatnonzero(flat == l)
            self.idx[l] = idx
            if r1 == r0 or idx.size == 0:
                continue
            pl = tuple(h[idx] for h in self.planes)
            self.key0[l] = scan_keys(pl, self.sg[idx], csf[r0:r1], self.nc[r0:r1], self.l2)  # fp32
            xx, yy = x[idx], self.ys[r0:r1].astype(np.float64)
            ex = np.empty((idx.size, r1 - r0))
            for i in range(idx.size):
                ex[i] = ((xx[i][None, :] - yy) ** 2).sum(1) if self.l2 else -(yy @ xx[i])
            self.exact[l] = ex
        self.set_shift32(self.shift32)

    def set_shift32(self, shift32):
        """The keys with the pairs' fp32 shifts given (the model's own, or the device's where the two
        fp64 sums round differently): key = fl32(key0 + shift), one rounded fp32 addition."""
        self.shift32 = np.asarray(shift32, dtype=f32)
        for l, k0 in self.key0.items():
            self.keys[l] = (k0 + self.shift32[self.idx[l]][:, None]).astype(f32)

    def pair(self, q, j):
        return q * self.nlist + j

    def pair_keys(self, q, j):
        """(row0, keys, exact) of pair (q, j) over its list's rows."""
        l = int(self.P[q, j])
        if l not in self.keys:
            return int(self.off[l]), np.zeros(0, f32), np.zeros(0)
        i = int(np.searchsorted(self.idx[l], self.pair(q, j)))
        return int(self.off[l]), self.keys[l][i], self.exact[l][i]

    def slot(self, q, j, C, c):
        """The list k_ivfsq_scan leaves in slot j * C + c of query q: (keys, rows), the first KP of the
        chunk's rows by (key, row)."""
        r0, keys, _ = self.pair_keys(q, j)
        a, b = chunk_rows(r0, r0 + keys.size, C)[c]
        sub = keys[a - r0:b - r0]
        o = np.argsort(sub, kind="stable")[:KP]
        return sub[o], o + a

    def refine(self, q, nprobe, C, k, escale=1.0):
        """k_ivfsq_refine for query q: (flagged, rows of its top k by (exact fp32 key, row))."""
        ks, rs = [], []
        for j in range(min(nprobe, self.nlist)):
            for c in range(C):
                kk, rr = self.slot(q, j, C, c)
                ks.append(kk)
                rs.append(rr)
        ks, rs = np.concatenate(ks), np.concatenate(rs)
        o = np.lexsort((rs, ks))[:KP]
        mk, mr = ks[o], rs[o]
        x = self.xq[q].astype(np.float64)
        y = self.ys[mr].astype(np.float64)
        ex = (((x[None, :] - y) ** 2).sum(1) if self.l2 else -(y @ x)).astype(f32)
        o2 = np.lexsort((mr, ex))
        top = mr[o2][:k]
        flagged = False
        if ks.size >= KP:
            kth = ex[o2][k - 1] if k <= ex.size else np.inf
            Eq = float(self.E[q * self.nlist:q * self.nlist + min(nprobe, self.nlist)].max()) * escale
            flagged = not certified(kth, mk[KP - 1], 0.0, Eq, self.rho)
        return flagged, top

    def flagged_range(self, nprobe, C, k):
        """(lo, hi): the count of uncertified queries with E scaled by 1 -+ 1e-5 (the device's E is the
        same fp64 formula summed in another order)."""
        lo = sum(self.refine(q, nprobe, C, k, 1.0 - 1e-5)[0] for q in range(self.nq))
        hi = sum(self.refine(q, nprobe, C, k, 1.0 + 1e-5)[0] for q in range(self.nq))
        return lo, hi

    def max_list_rows(self):
        return int(np.diff(self.off).max())


# ---- the corpora the GPU tests use (fp32 rows, centroids given) -----------------------------------
def groups_corpus(d=384):
    """320 queries, 300 of them nearest the 1000-row list: more than one pair group per list."""
    c, xb, lists, _ = IV.edge_corpus(d, "float32")
    r = np.random.default_rng(5)
    ql = np.concatenate([np.full(300, 11), r.integers(0, 11, 20)])
    r.shuffle(ql)
    xq = (c[ql] + 0.1 * r.standard_normal((ql.size, d)).astype(f32)).astype(f32)
    return c, xb, lists, xq


LONG_SIZES = (20000, 3, 0, 130, 1, 64, 7, 256)


def long_corpus(nq, d=384):
    """One list of 20,000 rows probed by nq queries: chunks > 1."""
    c, xb, lists, _ = IV.edge_corpus(d, "float32", sizes=LONG_SIZES, seed=3, nq=5)
    r = np.random.default_rng(8)
    xq = (c[np.zeros(nq, dtype=int)] + 0.1 * r.standard_normal((nq, d)).astype(f32)).astype(f32)
    return c, xb, lists, xq


@functools.lru_cache(maxsize=4)
def edge_model(d, metric, by_residual, qtype=R.QT_8bit):
    c, xb, lists, xq = IV.edge_corpus(d, "float32")
    return ScanModel(c, xb, lists, xq, metric, qtype, by_residual)


def check_bound(m):
    worst = 0.0
    for l, keys in m.keys.items():
        ex = m.exact[l]
        err = np.abs(keys.astype(np.float64) - ex)
        E = m.E[m.idx[l]].astype(np.float64)[:, None]
        bound = E + 1e-13 * (1.0 + np.abs(ex))  # (the slack: this fp64 reference's own rounding)
        if m.l2:
            bound = bound + 2.0 * m.rho_dec * np.sqrt(ex)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), f"list {l}"
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
@pytest.mark.parametrize("d", [20, 384, 1100])
def test_edge_corpus(d, metric, by_residual):
    m = edge_model(d, metric, by_residual)
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
    print(f"d {d} {'L2' if metric == L2 else 'IP'} by_residual {by_residual}: E median {np.median(m.E):.3g}, "
          f"rho_dec {m.rho_dec:.3g}, worst error / bound {worst:.3f}, certified (nprobe, C, k, n of {m.nq}) {out}")


@pytest.mark.parametrize("metric", [L2, IP], ids=["L2", "IP"])
def test_uniform_qtype(metric):
    m = edge_model(384, metric, True, R.QT_8bit_uniform)
    check_bound(m)
    n = check_certified(m, np.arange(m.order.size, dtype=np.int64), 3, plan_chunks(m.nq, 3, m.max_list_rows()), 10)
    assert n >= 0.9 * m.nq


def test_more_than_one_pair_group():
    c, xb, lists, xq = groups_corpus()
    assert (IV.assign(xq, c, L2) == np.asarray(IV.probe(xq, c, 1, L2))[:, 0]).all()
    m = ScanModel(c, xb, lists, xq, L2)
    check_bound(m)
    n = check_certified(m, np.arange(xb.shape[0], dtype=np.int64), 2, 1, 10)
    assert n >= 0.9 * m.nq, n
    assert (m.P[:, 0] == 11).sum() >= 300 > TILE


@pytest.mark.parametrize("nq", [1, 5])
def test_chunked_long_list(nq):
    c, xb, lists, xq = long_corpus(nq)
    m = ScanModel(c, xb, lists, xq, L2)
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
    """The two terms the pair's E gains over 3.14's: fl32(shift) and the one addition."""
    m = edge_model(384, L2, True)
    for l, keys in m.keys.items():
        idx = m.idx[l]
        r0, r1 = m.off[l], m.off[l + 1]
        pl = tuple(h[idx] for h in m.planes)
        k0 = scan_keys(pl, m.sg[idx], (m.ref.codes[m.order][r0:r1].astype(np.float64) - 128), m.nc[r0:r1], True)
        exact_sum = k0.astype(np.float64) + m.shift[idx][:, None]
        err = np.abs(keys.astype(np.float64) - exact_sum)
        A2 = np.abs(k0).max()
        assert (err <= U * (2.0 * np.abs(m.shift[idx])[:, None] + A2) * 1.01).all()


def test_store_blobs_have_the_shape_the_gpu_test_needs():
    x, _ = kref.blobs(2000, 100, 16, 7, 0)
    assert np.asarray(x).shape == (2000, 100)

"""Scan-level parity of the scalar quantizer: what k_sq_prep and k_sq_scan leave
on the device against the numpy model of tests/test_sq_model.py.

An IndexScalarQuantizer search is exact even when the int8 scan is wrong: the
refine recomputes distances from the codes and the exact scan repairs every query
the refine cannot certify.  A wrong plane, scale, key or bound
then shows only as flagged queries, or not at all.  So the diagnostic build dumps
(FX_SQ_CAND, fx_api_sq.cpp) what the scan wrote before the refine reads it: every
(query tile, split) list, the digit planes, sigma, E, the shift, and the index's
constants.  Asserted per case:

  prep   planes and sigma bitwise the model's, padding zero, shift / E / the index
         words within the rounding of one fp64 formula;
  keys   every listed (key, row) bitwise the model's key of that pair;
  lists  every (query tile, split, query) list is the first KP of the model's keys
         over exactly the split's rows, by (key, row) -- the property the refine's
         certification rests on;
  flags  last_fallbacks() is the model's count of uncertified queries;
  and the search result against the oracle, as tests/test_sq_gpu.py does.

The box-corner case (tests/_sq_ref.corner_corpus) has accumulators past 2^24, where
f32(acc) rounds: there the model's restatement of that conversion is what is pinned.
"""
import os

import numpy as np
import pytest

from tests import _sq_ref as R
from tests.test_sq_gpu import check
from tests.test_sq_model import certified, index_consts, inexact_conversions, int_dots, prep, scan_keys

pytestmark = pytest.mark.gpu

L2, IP = 1, 0
KP, TILE = 32, 128
NQ, K = 150, 10
FLAG_KS = (K, 28, 31, 32)  # flag parity: the search's k, then k at and just below KP

# (d, metric, corpus, ntotal): 1300 + d rows are >= 11 tiles -- 3 splits of uneven tile ranges and a ragged
# last tile; 20 rows are fewer than KP (lists padded); the corner corpus passes the accumulator's fp32 range
CASES = [(d, m, "normal", 1300 + d) for d in (20, 100, 384, 1100) for m in (L2, IP)]
CASES += [(100, m, "normal", 20) for m in (L2, IP)]
CASES += [(1100, m, "corner", 1300 + 1100) for m in (L2, IP)]


def _id(c):
    return f"d{c[0]}-{'L2' if c[1] == L2 else 'IP'}-{c[2]}-n{c[3]}"


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class Dump:
    """The FX_SQ_CAND file of a single-pass search."""

    def __init__(self, path, qtiles, splits, nq, rb, ntotal):
        buf = open(path, "rb").read()
        self.off = 0

        def take(dtype, *shape):
            n = int(np.prod(shape)) * np.dtype(dtype).itemsize
            a = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape)), offset=self.off).reshape(shape)
            self.off += n
            return a

        nq_pad = qtiles * TILE
        # [qtile][split][128][KP] -> [query][split][KP]; the scan writes no list for a padding query row
        # (its flush stops at nq), so those entries are whatever the buffer held and are not read here:
        # a padding row can only show as a wrong key under a live query, which key parity catches
        def per_query(a):
            return a.transpose(0, 2, 1, 3).reshape(nq_pad, splits, KP)[:nq]

        self.cand_d = per_query(take(np.float32, qtiles, splits, TILE, KP))
        self.cand_i = per_query(take(np.int32, qtiles, splits, TILE, KP))
        self.sigma = take(np.float32, nq_pad)
        self.qeps = take(np.float32, nq)
        self.qshift = take(np.float64, nq)
        self.planes = take(np.int8, 3, nq_pad, rb)
        self.words = take(np.uint32, 4)
        self.nc = take(np.float32, ntotal)
        assert self.off == len(buf), "one pass was expected in the dump"


class Case:
    pass


@pytest.fixture(scope="module", params=CASES, ids=_id)
def case(request, diag_fx, tmp_path_factory):
    d, metric, corpus, ntotal = request.param
    l2 = metric == L2
    if corpus == "corner":
        xb, xq = R.corner_corpus(ntotal, NQ, d)
    else:
        rng = np.random.default_rng(1000 + d + metric)
        xb = rng.standard_normal((ntotal, d)).astype(np.float32)
        xq = rng.standard_normal((NQ, d)).astype(np.float32)
    path = tmp_path_factory.mktemp("sqcand") / "cand.bin"
    os.environ["FX_SQ_CAND"] = str(path)  # (read when the index is created)
    try:
        ix = diag_fx.IndexScalarQuantizer(d, R.QT_8bit, metric)
    finally:
        del os.environ["FX_SQ_CAND"]
    ix.train(xb)
    ix.add(xb)
    c = Case()
    c.d, c.l2, c.metric, c.corpus, c.ntotal, c.xb, c.xq, c.ix = d, l2, metric, corpus, ntotal, xb, xq, ix
    c.got = ix.search(xq, K)
    c.fallbacks = ix.last_fallbacks()
    c.plan = ix.last_sq_plan()
    assert c.plan["path"] == "fused" and c.plan["qtiles"] == 2 and c.plan["q_batch"] >= NQ, c.plan
    c.splits = c.plan["splits"]
    c.rb = (d + 127) // 128 * 128
    c.dump = Dump(path, 2, c.splits, NQ, c.rb, ntotal)
    # flagged counts at larger k as well (the dump above is read already; these passes append to the file):
    # k = 10 certifies every query of these corpora, k near KP leaves the refine little or no room
    c.flags = {K: c.fallbacks}
    for k in FLAG_KS[1:]:
        ix.search(xq, k)
        c.flags[k] = ix.last_fallbacks()

    # the model, from the trained tables the device holds and the reference's codes
    trained = ix.trained
    assert (trained == R.train(xb)).all()
    codes = R.encode(xb, trained)
    assert (ix.sa_encode(xb) == codes).all()
    c.dec = R.decode(codes, trained)
    c.s, c.m, cs, c.nc, c.M2, c.c2max, c.rho_dec = index_consts(trained, codes)
    c.planes, c.sg, c.shift, c.E = prep(xq, c.s, c.m, l2, c.M2, c.c2max, c.rho_dec)
    # (the dots through the fp64 BLAS: exact, every partial sum is an integer below 2^53)
    pf, csf = tuple(h.astype(np.float64) for h in c.planes), cs.astype(np.float64)
    c.acc = int_dots(pf, csf)
    c.keys = scan_keys(pf, c.sg, csf, c.nc, l2)
    assert c.keys.dtype == np.float32 and c.keys.shape == (NQ, ntotal)
    # L2: the model's last step fl(scale t2 + n_c) goes through fp64; it is the device's single rounding
    # wherever that fp64 sum is exact (two-sum residual 0)
    c.inexact = np.zeros(c.keys.shape, dtype=bool)
    if l2:
        a = 2.0 * scan_keys(pf, c.sg, csf, c.nc, False).astype(np.float64)  # -2 sigma t2, exact
        b = np.broadcast_to(c.nc.astype(np.float64)[None, :], a.shape)
        sm = a + b
        bb = sm - a
        c.inexact = ((a - (sm - bb)) + (b - bb)) != 0.0
    return c


def test_plan_has_the_shape_the_case_is_about(case):
    n_ctiles = (case.ntotal + TILE - 1) // TILE
    if case.ntotal > KP:
        assert n_ctiles >= 11 and case.ntotal % TILE != 0
        assert case.splits >= 3, case.plan
        sizes = {(s + 1) * n_ctiles // case.splits - s * n_ctiles // case.splits for s in range(case.splits)}
        assert len(sizes) > 1 or n_ctiles % case.splits == 0, "uneven tile ranges were expected"
    else:
        assert case.splits == 1
    if case.corpus == "corner":
        rounded = inexact_conversions(case.acc[0])
        amax = float(np.abs(case.acc[0]).max())
        print(f"{_id((case.d, case.metric, case.corpus, case.ntotal))}: max |a1| = {amax:.0f}, "
              f"f32(a1) != a1 for {rounded} pairs")
        assert amax > 2 ** 24 and rounded >= 1, "the corpus does not reach the accumulator's inexact fp32 range"


def test_prep_parity(case):
    c, dm = case, case.dump
    d, nq = c.d, NQ
    for p in range(3):
        assert (dm.planes[p, :nq, :d] == c.planes[p]).all(), f"plane {p + 1}"
    assert (dm.planes[:, nq:, :] == 0).all(), "padding query rows of the planes"
    assert (dm.planes[:, :, d:] == 0).all(), "padding dimensions of the planes"
    assert (bits(dm.sigma[:nq]) == bits(c.sg)).all(), "sigma"
    assert (np.abs(dm.qshift - c.shift) <= 1e-12 * np.abs(c.shift)).all(), "shift"
    E = c.E.astype(np.float64)
    assert np.isfinite(dm.qeps).all() and (np.abs(dm.qeps.astype(np.float64) - E) <= 1e-6 * E).all(), "E"
    # the index words and the rows' constants
    assert int(dm.words[1]) == c.c2max, "max sum c'^2"
    assert int(dm.words[0]) == int(bits(np.float32(c.M2))[0]), "max n_c"
    assert (bits(dm.nc) == bits(c.nc)).all(), "n_c"
    rho = float(dm.words[2:3].view(np.float32)[0])
    assert abs(rho - c.rho_dec) <= 1e-6 * c.rho_dec, "rho_dec"


def test_key_parity(case):
    c, dm = case, case.dump
    ci, cd = dm.cand_i, dm.cand_d
    assert ((ci >= -1) & (ci < c.ntotal)).all(), "a listed row outside [0, ntotal)"
    q, s, j = np.nonzero(ci >= 0)
    rows = ci[q, s, j]
    dev, mod = cd[q, s, j], c.keys[q, rows]
    same = bits(dev) == bits(mod)
    loose = c.inexact[q, rows]
    near = (dev == np.nextafter(mod, np.float32(-np.inf))) | (dev == np.nextafter(mod, np.float32(np.inf)))
    print(f"{rows.size} listed pairs, {int(loose.sum())} with an inexact fp64 sum in the model, "
          f"{int((~same).sum())} keys differ")
    assert loose.sum() < 0.01 * rows.size, "the double-rounding exception covers too many pairs"
    bad = ~(same | (loose & near))
    assert not bad.any(), (f"{int(bad.sum())} keys differ from the model, first (query, row) = "
                           f"({q[bad][0]}, {rows[bad][0]}): {dev[bad][0]!r} vs {mod[bad][0]!r}")
    if c.corpus == "corner":  # the pairs whose f32(acc) rounds are among the listed ones, or the case pins nothing
        a1 = c.acc[0][q, rows]
        assert ((np.abs(a1) > 2 ** 24) & (a1.astype(np.float32).astype(np.float64) != a1)).any(), \
            "no listed pair has an inexactly converted accumulator"


def test_list_parity(case):
    c, dm = case, case.dump
    n_ctiles = (c.ntotal + TILE - 1) // TILE
    for s in range(c.splits):
        r0 = (s * n_ctiles // c.splits) * TILE
        r1 = min(((s + 1) * n_ctiles // c.splits) * TILE, c.ntotal)
        sub = c.keys[:, r0:r1]
        order = np.argsort(sub, axis=1, kind="stable")[:, :KP]  # (key, row): rows ascend within equal keys
        n = order.shape[1]
        want_i = np.full((NQ, KP), -1, dtype=np.int64)
        want_d = np.full((NQ, KP), np.inf, dtype=np.float32)
        want_i[:, :n] = order + r0
        want_d[:, :n] = np.take_along_axis(sub, order, axis=1)
        got_i, got_d = dm.cand_i[:, s, :], dm.cand_d[:, s, :]
        bad = np.flatnonzero((got_i != want_i).any(1))
        assert bad.size == 0, (f"split {s} rows [{r0}, {r1}): lists differ for queries {bad[:5]}: "
                               f"{got_i[bad[0]]} vs {want_i[bad[0]]}")
        assert (got_d[:, n:] == np.inf).all(), f"split {s}: missing entries must hold +inf"
        loose = np.zeros((NQ, KP), dtype=bool)
        loose[:, :n] = np.take_along_axis(c.inexact[:, r0:r1], order, axis=1)
        assert ((bits(got_d) == bits(want_d)) | loose).all(), f"split {s}: keys differ"  # (loose: test_key_parity)


def test_flags_and_results(case):
    c = case
    x = c.xq.astype(np.float64)
    y = c.dec.astype(np.float64)
    rho = c.rho_dec if c.l2 else 0.0
    lo, hi = dict.fromkeys(FLAG_KS, 0), dict.fromkeys(FLAG_KS, 0)
    if c.ntotal >= KP:  # (fewer than KP candidates in all never flag: no split dropped a row)
        for i in range(NQ):
            best = np.argsort(c.keys[i], kind="stable")[:KP]
            tb = c.keys[i, best[KP - 1]]
            if c.l2:
                df = x[i][None, :] - y[best]
                ex = np.sort((df * df).sum(1).astype(np.float32))
            else:
                ex = np.sort((-(y[best] @ x[i])).astype(np.float32))
            E = float(c.E[i])
            for k in FLAG_KS:
                lo[k] += not certified(ex[k - 1], tb, c.shift[i], E * (1.0 - 1e-5), rho)
                hi[k] += not certified(ex[k - 1], tb, c.shift[i], E * (1.0 + 1e-5), rho)
    for k in FLAG_KS:
        print(f"{_id((c.d, c.metric, c.corpus, c.ntotal))} k={k}: {c.flags[k]} of {NQ} queries flagged "
              f"(model: {lo[k]} .. {hi[k]}), splits {c.splits}")
    for k in FLAG_KS:
        assert lo[k] <= c.flags[k] <= hi[k], f"k = {k}"
    check(c.ix, c.got, R.search(c.xq, c.dec, K, c.metric), "search")

"""Scan-level parity of IndexIVFScalarQuantizer: what k_ivfsq_prep and k_ivfsq_scan leave on the device
against the numpy model of tests/test_ivfsq_model.py.

As for the two parent indexes (tests/test_sq_scan_parity.py, tests/test_ivf_scan_parity.py) a search
is exact even when the list scan is wrong: the refine recomputes distances from the codes and the
exact list scan repairs every query the refine cannot certify.  So the diagnostic build dumps
(FX_IVFSQ_CAND, fx_api_ivfsq.cpp) what the scan wrote before the refine reads it.  Asserted per case
on the edge corpus (nprobe = 3: 111 pairs, so every list is cut into two chunks):

  prep   the pairs' planes and sigma bitwise the model's, padding zero; the fp32 shift the model's
         fp64 shift rounded (or its neighbour: the device sums the same fp64 terms in another order),
         E within 1e-6; the probed lists, list_off and the rows' n_c the model's;
  keys   every listed (key, row) bitwise the model's key of that (pair, row);
  lists  every slot is the first KP of the model's keys over exactly that list chunk's rows, by
         (key, row) -- the property the refine's certification rests on."""
import os

import numpy as np
import pytest

from tests import _ivf_ref as IV
from tests import _ivfsq_ref as R
from tests.test_ivfsq_gpu import check, make_index
from tests.test_ivfsq_model import KP, ScanModel, chunk_rows
from tests.test_sq_model import scan_keys

pytestmark = pytest.mark.gpu

L2, IP = R.METRIC_L2, R.METRIC_INNER_PRODUCT
NPROBE, K = 3, 10
CASES = [(d, m, True) for d in (20, 384, 1100) for m in (L2, IP)] + [(384, L2, False)]


def _id(c):
    return f"d{c[0]}-{'L2' if c[1] == L2 else 'IP'}-{'res' if c[2] else 'plain'}"


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class Dump:
    """The FX_IVFSQ_CAND file of a single-pass search."""

    def __init__(self, path, nq, slots, nprobe, nlist, rb, ntotal):
        buf = open(path, "rb").read()
        self.off = 0

        def take(dtype, *shape):
            n = int(np.prod(shape))
            a = np.frombuffer(buf, dtype=dtype, count=n, offset=self.off).reshape(shape)
            self.off += n * np.dtype(dtype).itemsize
            return a

        pairs_pad = (nq * nprobe + 127) // 128 * 128
        self.cand_d = take(np.float32, nq, slots, KP)
        self.cand_i = take(np.int32, nq, slots, KP)
        self.coarse = take(np.int64, nq, nprobe)
        self.list_off = take(np.int32, nlist + 1)
        self.sigma = take(np.float32, pairs_pad)
        self.pshift = take(np.float32, pairs_pad)
        self.peps = take(np.float32, pairs_pad)
        self.planes = take(np.int8, 3, pairs_pad, rb)
        self.nc = take(np.float32, ntotal)
        assert self.off == len(buf), "one pass was expected in the dump"


class Case:
    pass


@pytest.fixture(scope="module", params=CASES, ids=_id)
def case(request, diag_fx, tmp_path_factory):
    d, metric, by_residual = request.param
    cent, xb, lists, xq = IV.edge_corpus(d, "float32")
    path = tmp_path_factory.mktemp("ivfsqcand") / "cand.bin"
    os.environ["FX_IVFSQ_CAND"] = str(path)  # (read when the index is created)
    try:
        ix = make_index(diag_fx, cent, metric, R.QT_8bit, by_residual)
    finally:
        del os.environ["FX_IVFSQ_CAND"]
    ix.train(xb)
    ix.add(xb)
    ix.nprobe = NPROBE
    c = Case()
    c.d, c.metric, c.l2, c.ix, c.xq = d, metric, metric == L2, ix, xq
    c.got = ix.search(xq, K)
    c.plan = ix.last_ivf_plan()
    c.fallbacks = ix.last_fallbacks()
    assert c.plan["path"] == "fused" and c.plan["q_batch"] >= xq.shape[0], c.plan
    c.C = c.plan["chunks"]
    assert c.C == 2 and c.plan["slots"] == NPROBE * c.C, c.plan
    c.nq, c.nlist, c.rb = xq.shape[0], cent.shape[0], (d + 127) // 128 * 128
    c.dump = Dump(path, c.nq, c.plan["slots"], NPROBE, c.nlist, c.rb, xb.shape[0])
    c.m = ScanModel(cent, xb, lists, xq, metric, R.QT_8bit, by_residual)
    # the model's pair (q, j) is pair q * nlist + j of the full ranking; the device's q * NPROBE + j
    c.mp = (np.arange(c.nq)[:, None] * c.nlist + np.arange(NPROBE)[None, :]).reshape(-1)
    c.model_shift32 = c.m.shift32.copy()
    s32 = c.m.shift32.copy()
    s32[c.mp] = c.dump.pshift[:c.nq * NPROBE]
    c.m.set_shift32(s32)  # keys under the device's fp32 shifts (test_prep_parity pins those to the model's)
    # L2: the model's fl(scale t2 + n_c) goes through fp64; it is the device's single rounding wherever that
    # fp64 sum is exact (two-sum residual 0)
    c.inexact = {}
    for l, k0 in c.m.key0.items():
        bad = np.zeros(k0.shape, dtype=bool)
        if c.l2:
            idx = c.m.idx[l]
            r0, r1 = c.m.off[l], c.m.off[l + 1]
            pl = tuple(h[idx] for h in c.m.planes)
            cs = c.m.ref.codes[c.m.order][r0:r1].astype(np.float64) - 128.0
            a = 2.0 * scan_keys(pl, c.m.sg[idx], cs, c.m.nc[r0:r1], False).astype(np.float64)  # -2 sigma t2, exact
            b = np.broadcast_to(c.m.nc[r0:r1].astype(np.float64)[None, :], a.shape)
            sm = a + b
            bb = sm - a
            bad = ((a - (sm - bb)) + (b - bb)) != 0.0
        c.inexact[l] = bad
    return c


def test_prep_parity(case):
    c, dm, m = case, case.dump, case.m
    npairs = c.nq * NPROBE
    assert (dm.coarse == m.P[:, :NPROBE]).all(), "probed lists"
    assert (dm.list_off == m.off).all(), "list_off"
    assert (bits(dm.nc) == bits(m.nc)).all(), "n_c"
    for p in range(3):
        assert (dm.planes[p, :npairs, :c.d] == m.planes[p][c.mp]).all(), f"plane {p + 1}"
    assert (dm.planes[:, npairs:, :] == 0).all(), "padding pair rows of the planes"
    assert (dm.planes[:, :, c.d:] == 0).all(), "padding dimensions of the planes"
    assert (bits(dm.sigma[:npairs]) == bits(m.sg[c.mp])).all(), "sigma"
    want = c.model_shift32[c.mp]
    got = dm.pshift[:npairs]
    near = (got == want) | (got == np.nextafter(want, np.float32(-np.inf))) | (got == np.nextafter(want, np.float32(np.inf)))
    assert near.all(), "shift"
    assert (np.abs(got.astype(np.float64) - m.shift[c.mp]) <= 6.0e-8 * np.abs(m.shift[c.mp])).all(), "shift"
    E = m.E[c.mp].astype(np.float64)
    got = dm.peps[:npairs]
    assert np.isfinite(got).all() and (np.abs(got.astype(np.float64) - E) <= 1e-6 * E).all(), "E"


def _model_of(c, q, slot):
    j, ch = divmod(slot, c.C)
    return j, ch, int(c.m.P[q, j])


def test_key_parity(case):
    c, dm, m = case, case.dump, case.m
    ntotal = dm.nc.size
    assert ((dm.cand_i >= -1) & (dm.cand_i < ntotal)).all(), "a listed row outside [0, ntotal)"
    n = differ = loose_n = 0
    for q in range(c.nq):
        for slot in range(NPROBE * c.C):
            j, ch, l = _model_of(c, q, slot)
            rows = dm.cand_i[q, slot]
            rows = rows[rows >= 0]
            if rows.size == 0:
                continue
            r0, keys, _ = m.pair_keys(q, j)
            assert ((rows >= r0) & (rows < r0 + keys.size)).all(), f"query {q} slot {slot}: a row outside list {l}"
            i = int(np.searchsorted(m.idx[l], m.pair(q, j)))
            dev, mod = dm.cand_d[q, slot, :rows.size], keys[rows - r0]
            same = bits(dev) == bits(mod)
            loose = c.inexact[l][i][rows - r0]
            near = (dev == np.nextafter(mod, np.float32(-np.inf))) | (dev == np.nextafter(mod, np.float32(np.inf)))
            bad = ~(same | (loose & near))
            assert not bad.any(), (f"query {q} slot {slot} (list {l}): key of row {rows[bad][0]} is "
                                   f"{dev[bad][0]!r}, the model's {mod[bad][0]!r}")
            n += rows.size
            differ += int((~same).sum())
            loose_n += int(loose.sum())
    print(f"{_id((c.d, c.metric, True))}: {n} listed pairs, {loose_n} with an inexact fp64 sum in the model, "
          f"{differ} keys differ")
    assert n > 0 and loose_n < 0.01 * n, "the double-rounding exception covers too many pairs"


def test_list_parity(case):
    c, dm, m = case, case.dump, case.m
    for q in range(c.nq):
        for slot in range(NPROBE * c.C):
            j, ch, l = _model_of(c, q, slot)
            kk, rr = m.slot(q, j, c.C, ch)
            want_i = np.full(KP, -1, dtype=np.int64)
            want_i[:rr.size] = rr
            got_i = dm.cand_i[q, slot]
            r0, r1 = int(m.off[l]), int(m.off[l + 1])
            assert (got_i == want_i).all(), (f"query {q} slot {slot}: list {l} rows [{r0}, {r1}) chunk "
                                             f"{chunk_rows(r0, r1, c.C)[ch]}: {got_i} vs {want_i}")
            if rr.size:
                i = int(np.searchsorted(m.idx[l], m.pair(q, j)))
                loose = c.inexact[l][i][rr - r0]
                assert ((bits(dm.cand_d[q, slot, :rr.size]) == bits(kk)) | loose).all(), f"query {q} slot {slot}: keys"
                assert (dm.cand_d[q, slot, rr.size:] == np.inf).all(), "missing entries must hold +inf"


def test_flags_and_results(case):
    c, m = case, case.m
    lo, hi = m.flagged_range(NPROBE, c.C, K)
    print(f"{c.fallbacks} of {c.nq} queries flagged (model: {lo} .. {hi})")
    assert lo <= c.fallbacks <= hi
    ids = np.arange(m.order.size, dtype=np.int64)
    check(c.ix, c.got, m.ref.search(c.xq, ids, K, NPROBE, c.metric), "search")

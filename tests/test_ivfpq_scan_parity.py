"""Scan-level parity of IndexIVFPQ: what k_ivfpq_prep and k_ivfpq_scan leave on the device against
the numpy model of tests/test_ivfpq_model.py.

As for the parent indexes (tests/test_ivfsq_scan_parity.py, tests/test_pq_scan_parity.py) a search is
exact even when the list scan is wrong: the refine recomputes distances from the codes and the exact
list scan repairs every query the refine cannot certify.  So the diagnostic build dumps
(FX_IVFPQ_CAND, fx_api_ivfpq.cpp) what the scan wrote before the refine reads it.  Asserted per case
on the edge corpus (nprobe = 3: 111 pairs, so every list is cut into two chunks):

  prep   the operand planes bitwise the model's, padding zero; the rows' codes and n_y bitwise; the
         probed lists and list_off the model's; the fp32 shift the model's fp64 shift rounded (or its
         neighbour: the device sums the same fp64 terms in another order), E within 1e-6;
  keys   every listed key lies within the accumulation term of the model's exactly summed key
         (the MFMA sums the same 3 K products in another order);
  lists  every slot holds rows of exactly its list chunk, sorted by (key, row), as many as the chunk
         has up to KP, and no row of the chunk left out is better than the slot's last by more than
         the accumulation term -- the property the refine's certification rests on;
  flags  at k = 10, 31, 32 the refine flags exactly the queries the certification rule flags on the
         dumped lists."""
import os

import numpy as np
import pytest

from tests import _ivf_ref as IV
from tests import _ivfpq_ref as R
from tests import _pq_ref as PQ
from tests.test_ivfpq_gpu import check, make_index
from tests.test_ivfpq_model import KP, ScanModel, certified, chunk_rows

pytestmark = pytest.mark.gpu

L2, IP = R.METRIC_L2, R.METRIC_INNER_PRODUCT
NPROBE = 3
CASES = [(16, 2, L2, True), (16, 2, IP, True), (384, 48, L2, True), (384, 48, IP, True), (384, 24, L2, False),
         (384, 24, IP, False), (1096, 137, L2, True), (1096, 137, IP, True)]


def _id(c):
    return f"d{c[0]}-M{c[1]}-{'L2' if c[2] == L2 else 'IP'}-{'res' if c[3] else 'plain'}"


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class Dump:
    """The FX_IVFPQ_CAND file of a single-pass search."""

    def __init__(self, path, nq, slots, nprobe, nlist, kp, op_rows, stride, ntotal):
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
        self.pshift = take(np.float32, pairs_pad)
        self.peps = take(np.float32, pairs_pad)
        self.planes = take(np.uint16, 2, op_rows, kp)
        self.codes = take(np.uint8, ntotal, stride)
        self.ny = take(np.float32, ntotal)
        assert self.off == len(buf), "one pass was expected in the dump"


class Case:
    pass


@pytest.fixture(scope="module", params=CASES, ids=_id)
def case(request, diag_fx, tmp_path_factory):
    d, M, metric, by_residual = request.param
    cent, xb, lists, xq = IV.edge_corpus(d, "float32")
    c = Case()
    c.m = ScanModel(cent, xb, lists, xq, metric, M, by_residual)
    c.path = tmp_path_factory.mktemp("ivfpqcand") / "cand.bin"
    os.environ["FX_IVFPQ_CAND"] = str(c.path)  # (read when the index is created)
    try:
        ix = make_index(diag_fx, cent, M, metric, by_residual, c.m.cents)
    finally:
        del os.environ["FX_IVFPQ_CAND"]
    ix.add(xb)
    ix.nprobe = NPROBE
    c.d, c.M, c.metric, c.l2, c.ix, c.xq, c.by_residual = d, M, metric, metric == L2, ix, xq, by_residual
    c.nq, c.nlist, c.ntotal = xq.shape[0], cent.shape[0], xb.shape[0]
    c.per_pair = c.l2 and by_residual
    # the model's pair (q, j) is pair q * nlist + j of the full ranking; the device's q * NPROBE + j
    c.mp = (np.arange(c.nq)[:, None] * c.nlist + np.arange(NPROBE)[None, :]).reshape(-1)
    return c


def search(c, k):
    c.path.write_bytes(b"")
    got = c.ix.search(c.xq, k)
    plan = c.ix.last_ivf_plan()
    assert plan["path"] == "fused" and plan["q_batch"] >= c.nq, plan
    C = plan["chunks"]
    assert C == 2 and plan["slots"] == NPROBE * C, plan
    op_rows = ((c.nq * NPROBE if c.per_pair else c.nq) + 127) // 128 * 128
    dump = Dump(c.path, c.nq, plan["slots"], NPROBE, c.nlist, PQ.kpad(c.d), op_rows, (c.M + 15) // 16 * 16, c.ntotal)
    return got, C, dump, c.ix.last_fallbacks()


def test_prep_parity(case):
    c, m = case, case.m
    _, _, dm, _ = search(c, 10)
    npairs = c.nq * NPROBE
    assert (dm.coarse == m.P[:, :NPROBE]).all(), "probed lists"
    assert (dm.list_off == m.off).all(), "list_off"
    assert (dm.codes[:, :c.M] == m.codes_s).all() and (dm.codes[:, c.M:] == 0).all(), "codes"
    assert (bits(dm.ny) == bits(m.ny)).all(), "n_y"
    # one operand per pair (L2 with by_residual), else per query: the model holds one per pair either way
    rows = c.mp if c.per_pair else c.mp[::NPROBE]
    live = rows.size
    assert (dm.planes[0, :live] == PQ.bf16_bits(m.xh[rows])).all(), "hi plane"
    assert (dm.planes[1, :live] == PQ.bf16_bits(m.xl[rows])).all(), "lo plane"
    assert (dm.planes[:, live:] == 0).all(), "padding operand rows"
    assert (dm.planes[:, :, c.d:] == 0).all(), "padding dimensions"
    want = m.shift32[c.mp]
    got = dm.pshift[:npairs]
    near = (got == want) | (got == np.nextafter(want, np.float32(-np.inf))) | (got == np.nextafter(want, np.float32(np.inf)))
    assert near.all(), "shift"
    assert (np.abs(got.astype(np.float64) - m.shift[c.mp]) <= 6.0e-8 * np.abs(m.shift[c.mp])).all(), "shift"
    E = m.E[c.mp].astype(np.float64)
    got = dm.peps[:npairs]
    assert np.isfinite(got).all() and (np.abs(got.astype(np.float64) - E) <= 1e-6 * E).all(), "E"


def test_key_and_list_parity(case):
    c, m = case, case.m
    _, C, dm, _ = search(c, 10)
    assert ((dm.cand_i >= -1) & (dm.cand_i < c.ntotal)).all(), "a listed row outside [0, ntotal)"
    n = 0
    worst = 0.0
    for q in range(c.nq):
        for slot in range(NPROBE * C):
            j, ch = divmod(slot, C)
            l = int(m.P[q, j])
            r0, r1 = int(m.off[l]), int(m.off[l + 1])
            a, b = chunk_rows(r0, r1, C)[ch]
            cd, ci = dm.cand_d[q, slot], dm.cand_i[q, slot]
            live = ci >= 0
            cnt = int(live.sum())
            what = f"query {q} slot {slot}: list {l} rows [{r0}, {r1}) chunk [{a}, {b})"
            assert cnt == min(KP, b - a) and live[:cnt].all(), what
            if cnt == 0:  # (no block wrote the slot: it keeps the host's -1 ids, its keys are not read)
                continue
            assert (cd[cnt:] == np.inf).all(), what + ": missing entries must hold +inf"
            rows = ci[:cnt].astype(np.int64)
            assert ((rows >= a) & (rows < b)).all() and len(set(rows.tolist())) == cnt, what
            pairs = list(zip(cd[:cnt].tolist(), rows.tolist()))
            assert pairs == sorted(pairs), what
            i = int(np.searchsorted(m.idx[l], m.pair(q, j)))
            # the exactly summed key under the device's own fp32 shift
            k64 = m.key64[l][i] - m.shift[m.pair(q, j)] + float(dm.pshift[q * NPROBE + j])
            term = m.pair_slack(q, j)
            err = np.abs(cd[:cnt].astype(np.float64) - k64[rows - r0])
            worst = max(worst, float((err / term).max()))
            assert (err <= term).all(), what + f": key off by {err.max()} (term {term})"
            rest = np.setdiff1d(np.arange(a, b), rows)
            if rest.size:  # no better row of the chunk was left out
                assert k64[rest - r0].min() >= float(cd[cnt - 1]) - term, what
            n += cnt
    print(f"{_id((c.d, c.M, c.metric, c.by_residual))}: {n} listed keys, worst |key - model| / accumulation term {worst:.3f}")
    assert n > 0


def flagged_on_lists(c, dm, k):
    """k_ivfpq_refine's rule applied to the dumped lists."""
    m = c.m
    count = 0
    for q in range(c.nq):
        cd, ci = dm.cand_d[q].reshape(-1), dm.cand_i[q].reshape(-1)
        ok = ci >= 0
        cand = sorted(zip(cd[ok].tolist(), ci[ok].tolist()))
        if len(cand) < KP:
            continue
        top = cand[:KP]
        y = m.ys[[r for _, r in top]].astype(np.float64)
        x = c.xq[q].astype(np.float64)
        ex = (((x[None, :] - y) ** 2).sum(1) if c.l2 else -(y @ x)).astype(np.float32)
        Eq = float(dm.peps[q * NPROBE:(q + 1) * NPROBE].max())
        if not certified(np.sort(ex)[k - 1], np.float32(top[KP - 1][0]), Eq, m.rho):
            count += 1
    return count


@pytest.mark.parametrize("k", [10, 31, 32])
def test_flags_and_results(case, k):
    c, m = case, case.m
    got, C, dm, fallbacks = search(c, k)
    want = flagged_on_lists(c, dm, k)
    print(f"{_id((c.d, c.M, c.metric, c.by_residual))} k={k}: {fallbacks} of {c.nq} queries flagged, the rule gives {want}")
    assert fallbacks == want
    if k == 32:  # every query with KP candidates or more
        assert fallbacks == sum(m.candidates(q, NPROBE) >= KP for q in range(c.nq))
    ids = np.arange(m.order.size, dtype=np.int64)
    check(c.ix, got, m.ref.search(c.xq, ids, k, NPROBE, c.metric), f"search k={k}")

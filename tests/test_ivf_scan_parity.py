"""Scan-level parity of the inverted file: the candidate lists k_ivf_scan writes,
against a float64 restatement of the same operands.

An IndexIVFFlat search is exact within the probed lists even when the list scan
is wrong: the refine recomputes distances and the exact list scan repairs every
query the refine cannot certify.  Rows the scan let in from a
neighbouring list are ranked away by the refine; rows it dropped at a list's edge
show only when they were true neighbours.  So the diagnostic build dumps
(FX_IVF_CAND, fx_api_ivf.cpp) every (query, slot) list before the refine reads it,
with the probed list numbers and the list offsets.  Per (query, probe j):

  the probed list is the reference's j-th coarse choice; every listed row lies in
  the list; rows are distinct within a slot, across the probe's slots and across
  the query's probes; every slot is sorted by (key, row); |key - key_ref| <= B.

With one chunk per list, slot j is the whole list of probe j: a list of r rows
yields min(r, KP) entries, and no unlisted row of it has a key below the slot's last
by more than 2 B.  With C > 1 chunks (a pass of fewer than 256 (query, list) pairs:
plan_ivf) the probe has C slots whose tile ranges are the kernel's own; then no
unlisted row has a key below the smallest last key of the probe's FULL slots by more
than 2 B, and a probe without a full slot lists every row.  An empty list leaves its
slots empty.

key_ref and B are those of tests/test_scan_keys.py: |y|^2 - 2 x.y (IP: -x.y) in
fp64 on the stored values, B = (2 gamma_d + u)(|y|^2 + 2 |x| |y|).
"""
import os

import numpy as np
import pytest

from tests import _ivf_ref as ref
from tests import _kmeans_ref as kref

pytestmark = pytest.mark.gpu

L2, IP = ref.METRIC_L2, ref.METRIC_INNER_PRODUCT
KP, K = 32, 10
U = 2.0 ** -24


def make_ivf(diag, tmp_path, centroids, metric, dtype):
    """(index on the diagnostic build, its dump path)."""
    nlist, d = centroids.shape
    q = (diag.IndexFlatL2 if metric == L2 else diag.IndexFlatIP)(d)
    q.add(centroids)
    path = tmp_path / "ivf_cand.bin"
    os.environ["FX_IVF_CAND"] = str(path)  # (read when the index is created)
    try:
        ivf = diag.IndexIVFFlat(q, d, nlist, metric, dtype=dtype)
    finally:
        del os.environ["FX_IVF_CAND"]
    return ivf, path


def search_dump(ivf, path, xq, nprobe):
    """One search; (D, I, cand_d [nq][slots][KP], cand_i, coarse [nq][np], list_off [nlist + 1], plan)."""
    if path.exists():
        path.unlink()
    ivf.nprobe = nprobe
    D, I = ivf.search(xq, K)
    assert ivf.last_dropped_candidates() == 0
    plan = ivf.last_ivf_plan()
    assert plan["path"] == "fused" and plan["q_batch"] >= xq.shape[0], plan
    nq, np_eff, slots = xq.shape[0], min(nprobe, ivf.nlist), plan["slots"]
    assert slots == np_eff * plan["chunks"], plan
    buf = path.read_bytes()
    n = nq * slots * KP
    cd = np.frombuffer(buf, np.float32, n, 0).reshape(nq, slots, KP)
    ci = np.frombuffer(buf, np.int32, n, 4 * n).reshape(nq, slots, KP)
    coarse = np.frombuffer(buf, np.int64, nq * np_eff, 8 * n).reshape(nq, np_eff)
    off = np.frombuffer(buf, np.int32, ivf.nlist + 1, 8 * n + 8 * nq * np_eff)
    assert 8 * n + 8 * nq * np_eff + 4 * (ivf.nlist + 1) == len(buf), "one pass was expected in the dump"
    return D, I, cd, ci, coarse, off, plan


def reference_keys(xq, xs, metric, d):
    """(key_ref, B) [nq][n] over the stored rows xs (store order), as tests/test_scan_keys.py."""
    x, y = xq.astype(np.float64), xs.astype(np.float64)
    dot = x @ y.T
    ny = (y * y).sum(1)
    key = ny[None, :] - 2.0 * dot if metric == L2 else -dot
    g = d * U / (1 - d * U)
    nx = np.sqrt((x * x).sum(1))[:, None]
    return key, (2 * g + U) * (ny[None, :] + 2 * nx * np.sqrt(ny)[None, :]) + 1e-30


def check_slot(ids, keys, r0, r1, key_ref, B, what):
    """Membership, order and the key bound of one slot's valid entries; returns (rows, worst |err| / B)."""
    nv = int((ids >= 0).sum())
    assert (ids[:nv] >= 0).all() and (ids[nv:] == -1).all(), f"{what}: valid entries are not a prefix: {ids}"
    rows, kv = ids[:nv].astype(np.int64), keys[:nv].astype(np.float64)
    assert ((rows >= r0) & (rows < r1)).all(), f"{what}: rows outside the list [{r0}, {r1}): {rows}"
    assert np.unique(rows).size == nv, f"{what}: a row listed twice"
    assert np.isfinite(kv).all()
    asc = (kv[1:] > kv[:-1]) | ((kv[1:] == kv[:-1]) & (rows[1:] > rows[:-1]))
    assert asc.all(), f"{what}: not sorted by (key, row)"
    if nv == 0:
        return rows, 0.0
    ratio = np.abs(kv - key_ref[rows]) / B[rows]
    assert (ratio <= 1.0).all(), f"{what}: |key - key_ref| / B = {ratio.max():.3g}"
    return rows, float(ratio.max())


def check_lists(cd, ci, coarse, off, C, key_ref, B, what):
    """Every (query, probe) of one dumped search; returns (worst |err| / B, empty probes)."""
    worst, empty = 0.0, 0
    for q in range(coarse.shape[0]):
        seen = []
        for j in range(coarse.shape[1]):
            l = int(coarse[q, j])
            r0, r1 = int(off[l]), int(off[l + 1])
            w_ = f"{what} query {q} probe {j} (list {l}, {r1 - r0} rows)"
            rows, last_full = [], []
            for s in range(j * C, (j + 1) * C):
                rs, w = check_slot(ci[q, s], cd[q, s], r0, r1, key_ref[q], B[q], f"{w_} slot {s}")
                worst = max(worst, w)
                rows.append(rs)
                if rs.size == KP:
                    last_full.append(float(cd[q, s, KP - 1]))
            rows = np.concatenate(rows)
            assert np.unique(rows).size == rows.size, f"{w_}: a row in two of the probe's slots"
            if C == 1:
                assert rows.size == min(r1 - r0, KP), f"{w_}: {rows.size} entries"
            empty += r1 == r0
            rest = np.setdiff1d(np.arange(r0, r1), rows)
            if not last_full:
                assert rest.size == 0, f"{w_}: no slot is full, yet rows {rest[:5]} are not listed"
            else:  # completeness: no unlisted row belongs before the last entry of the slot that dropped it
                short = key_ref[q, rest] < min(last_full) - 2.0 * B[q, rest]
                assert not short.any(), f"{w_}: unlisted rows {rest[short][:5]} have smaller keys than the last listed"
            seen.append(rows)
        allrows = np.concatenate(seen)
        assert np.unique(allrows).size == allrows.size, f"{what} query {q}: a row under two probes"
    return worst, empty


@pytest.mark.parametrize("metric", [L2, IP], ids=["L2", "IP"])
@pytest.mark.parametrize("d,dtype", [(20, "float32"), (384, "bfloat16"), (768, "float16")])
def test_slots_are_the_probed_lists(diag_fx, tmp_path, d, dtype, metric):
    """The edge corpus twice: its 37 queries (fewer than 256 pairs at nprobe 1 and 3, which the planner
    cuts into chunks) and 256 queries, where every nprobe has one chunk and slot j is the whole list."""
    sizes = np.array(ref.EDGE_SIZES)
    starts = np.concatenate([[0], np.cumsum(sizes)])
    assert {0, 1, 127, 128, 129, 1000} <= set(sizes.tolist()), "the list sizes the scan's edges need"
    assert (starts[:-1][sizes > 0] % 4 != 0).any(), "no list starts off a 4-row boundary"
    c, xb, lists, xq37 = ref.edge_corpus(d, dtype)
    xq256 = ref.edge_corpus(d, dtype, nq=256)[3]
    assert (ref.edge_corpus(d, dtype, nq=256)[1] == xb).all()
    ivf, path = make_ivf(diag_fx, tmp_path, c, metric, dtype)
    ivf.add(xb)
    xs = np.ascontiguousarray(xb[ref.store_order(lists)])  # the stored rows, list by list
    ids = np.arange(xb.shape[0], dtype=np.int64)
    for xq in (xq37, xq256):
        nq = xq.shape[0]
        key_ref, B = reference_keys(xq, xs, metric, d)
        full = ref.ranking(xq, xb, lists, metric) if nq == 37 else None
        for nprobe in (1, 3, 12):
            D, I, cd, ci, coarse, off, plan = search_dump(ivf, path, xq, nprobe)
            if nq * nprobe >= 256:
                assert plan["chunks"] == 1, plan
            assert (off == starts).all(), "list offsets"
            assert (coarse == ref.probe(xq, c, nprobe, metric)).all(), "the probed lists are not the reference's"
            what = f"d={d} {dtype} {'L2' if metric == L2 else 'IP'} nq={nq} nprobe={nprobe}"
            worst, empty = check_lists(cd, ci, coarse, off, plan["chunks"], key_ref, B, what)
            print(f"{what}: chunks {plan['chunks']}, worst |key - key_ref| / B = {worst:.3g}, {empty} empty probes, "
                  f"{ivf.last_fallbacks()} queries flagged")
            if nprobe == 12:
                assert empty == 2 * nq, "every query probes the two empty lists"
            assert ivf.last_fallbacks() == 0
            if full is not None:  # the search itself, as tests/test_ivf_gpu.py asserts it
                Dr, Ir = ref.search(xq, xb, ids, lists, c, K, nprobe, metric, full=full)
                assert (I == Ir).all()
                assert (np.abs(D.astype(np.float64) - Dr) <= 1e-5 * np.maximum(1.0, np.abs(Dr))).all()


def test_chunked_list_slots(diag_fx, tmp_path):
    """One query over a 20,000-row list cut into many chunks (tests/test_ivf_gpu.py's sizes)."""
    d, dtype = 384, "bfloat16"
    sizes = (20000, 3, 0, 130, 1, 64, 7, 256)
    c, xb, lists, _ = ref.edge_corpus(d, dtype, sizes=sizes, seed=3, nq=5)
    r = np.random.default_rng(8)
    xq = kref.round_to(c[np.zeros(1, dtype=int)] + 0.1 * r.standard_normal((1, d)).astype(np.float32), dtype)
    ivf, path = make_ivf(diag_fx, tmp_path, c, L2, dtype)
    ivf.add(xb)
    xs = np.ascontiguousarray(xb[ref.store_order(lists)])
    key_ref, B = reference_keys(xq, xs, L2, d)
    D, I, cd, ci, coarse, off, plan = search_dump(ivf, path, xq, 1)
    assert plan["chunks"] > 2 and plan["slots"] == plan["chunks"], plan
    assert (off == np.concatenate([[0], np.cumsum(sizes)])).all()
    assert coarse[0, 0] == 0 == ref.probe(xq, c, 1, L2)[0, 0]
    worst, _ = check_lists(cd, ci, coarse, off, plan["chunks"], key_ref, B, "chunked")
    full_slots = int((ci[0, :, KP - 1] >= 0).sum())
    assert full_slots == plan["chunks"], "every chunk of the 20,000-row list holds more than KP rows"
    print(f"chunked: {plan['chunks']} chunks, worst |key - key_ref| / B = {worst:.3g}")
    Dr, Ir = ref.search(xq, xb, np.arange(xb.shape[0]), lists, c, K, 1, L2)
    assert (I == Ir).all() and ivf.last_fallbacks() == 0

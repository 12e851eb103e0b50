"""The gather scan pinned to its numpy model on the GPU (diagnostic build,
FX_PQ_CAND: the scan's lists, the query operands and the rows' constants, dumped
before the refine reads them).  Planes, n_y and codes are bitwise the model's;
shift and E match to the rounding of one fp64 formula; every listed key lies
within the fp32-accumulation term of the model's exactly summed key; every list
holds exactly its split's best rows; and the refine flags exactly the queries
the certification rule flags on those lists."""
import numpy as np
import pytest

from tests import _pq_ref as R

pytestmark = pytest.mark.gpu

KP, TILE = 32, 128
SHAPES = {16: 2, 64: 8, 96: 6, 776: 97}


def parse(path, nq, ntotal, d, M, qtiles, splits):
    buf = path.read_bytes()
    kp, stride, nq_pad = R.kpad(d), (M + 15) // 16 * 16, qtiles * TILE
    ncand = qtiles * splits * TILE * KP
    out, off = {}, 0
    for name, dt, cnt in (("cand_d", np.float32, ncand), ("cand_i", np.int32, ncand), ("eps", np.float32, nq),
                          ("shift", np.float64, nq), ("planes", np.uint16, 2 * nq_pad * kp),
                          ("codes", np.uint8, ntotal * stride), ("ny", np.float32, ntotal)):
        out[name] = np.frombuffer(buf, dtype=dt, count=cnt, offset=off).copy()
        off += cnt * np.dtype(dt).itemsize
    assert off == len(buf), "one pass, one dump"
    out["cand_d"] = out["cand_d"].reshape(qtiles, splits, TILE, KP)
    out["cand_i"] = out["cand_i"].reshape(qtiles, splits, TILE, KP)
    out["planes"] = out["planes"].reshape(2, nq_pad, kp)
    out["codes"] = out["codes"].reshape(ntotal, stride)
    return out


def flagged_on_lists(dump, xq, dec, metric, k):
    """k_pq_refine's rule applied to the dumped lists."""
    qtiles, splits = dump["cand_d"].shape[:2]
    count = 0
    for q in range(len(xq)):
        cd, ci = dump["cand_d"][q // TILE, :, q % TILE].reshape(-1), dump["cand_i"][q // TILE, :, q % TILE].reshape(-1)
        ok = ci >= 0
        cand = sorted(zip(cd[ok].tolist(), ci[ok].tolist()))
        if len(cand) < KP:
            continue
        top = cand[:KP]
        ex = R.exact64(xq[q:q + 1], dec[[r for _, r in top]], metric)[0].astype(np.float32)
        if not R.certified(np.sort(ex)[k - 1], np.float32(top[KP - 1][0]), dump["shift"][q], dump["eps"][q]):
            count += 1
    return count


@pytest.mark.parametrize("n_extra", [1300, 20], ids=["1300+d", "20"])
@pytest.mark.parametrize("metric", [R.L2, R.IP], ids=["L2", "IP"])
@pytest.mark.parametrize("d", sorted(SHAPES))
def test_scan_lists_match_the_model(diag_fx, monkeypatch, tmp_path, d, metric, n_extra):
    M = SHAPES[d]
    n = n_extra + d if n_extra > 20 else 20
    nq = 150
    xb, xq = R.clustered(d, n, nq, seed=2 * d + 1)
    cents = R.sampled_centroids(xb, M)
    path = tmp_path / "pq_cand.bin"
    monkeypatch.setenv("FX_PQ_CAND", str(path))  # (read when the index is created)
    ix = diag_fx.IndexPQ(d, M, 8, metric)
    monkeypatch.delenv("FX_PQ_CAND")
    ix.pq.centroids = cents
    ix.add(xb)
    codes = R.encode(xb, cents)
    dec = R.decode(codes, cents)
    ny = R.row_norms(codes, cents)
    xh, xl, shift, eps = R.prep(xq, metric, cents)
    yh, yl = R.image_rows(codes, cents)
    k64 = R.keys64(xh, xl, yh, yl, ny, metric)
    term = R.accumulation_term(xq, metric, cents)
    for k in (10, 31, 32):
        path.write_bytes(b"")
        D, I = ix.search(xq, k)
        plan = ix.last_pq_plan()
        assert plan["path"] == "fused" and ix.last_dropped_candidates() == 0
        qtiles, splits = plan["qtiles"], plan["splits"]
        dump = parse(path, nq, n, d, M, qtiles, splits)
        # operands and row constants: bitwise
        assert (dump["codes"][:, :M] == codes).all() and (dump["codes"][:, M:] == 0).all()
        assert (dump["ny"].view(np.uint32) == ny.view(np.uint32)).all()
        assert (dump["planes"][0, :nq] == R.bf16_bits(xh)).all() and (dump["planes"][1, :nq] == R.bf16_bits(xl)).all()
        assert (dump["planes"][:, nq:] == 0).all()
        # shift and E: one fp64 formula, rounded (E to fp32)
        assert np.allclose(dump["shift"], shift, rtol=1e-12, atol=0)
        assert np.allclose(dump["eps"], eps, rtol=1e-6, atol=0)
        # the lists
        nct = (n + TILE - 1) // TILE
        for q in range(nq):
            for s in range(splits):
                a, b = min(n, (s * nct // splits) * TILE), min(n, ((s + 1) * nct // splits) * TILE)
                cd, ci = dump["cand_d"][q // TILE, s, q % TILE], dump["cand_i"][q // TILE, s, q % TILE]
                live = ci >= 0
                m = int(live.sum())
                assert m == min(KP, b - a) and live[:m].all(), (q, s)
                rows = ci[:m]
                assert ((rows >= a) & (rows < b)).all() and len(set(rows.tolist())) == m, (q, s)
                pairs = list(zip(cd[:m].tolist(), rows.tolist()))
                assert pairs == sorted(pairs), (q, s)
                assert (np.abs(cd[:m].astype(np.float64) - k64[q, rows]) <= term[q]).all(), (q, s)
                # no better row of the split was left out
                rest = np.setdiff1d(np.arange(a, b), rows)
                if rest.size:
                    assert k64[q, rest].min() >= float(cd[m - 1]) - term[q], (q, s)
        want = flagged_on_lists(dump, xq, dec, metric, k)
        print(f"d={d} metric={metric} n={n} k={k}: splits={splits}, flagged {ix.last_fallbacks()}, the rule gives {want}")
        assert ix.last_fallbacks() == want
        Dr, Ir = R.search(xq, dec, k, metric)
        assert (I == Ir).all()

"""The IndexIVFScalarQuantizer reference of tests/_ivfsq_ref.py checked against the two references it
is composed from, on the CPU."""
import numpy as np
import pytest

from tests import _ivf_ref as IV
from tests import _ivfsq_ref as R
from tests import _sq_ref as SQ

L2, IP = R.METRIC_L2, R.METRIC_INNER_PRODUCT


@pytest.mark.parametrize("metric", [L2, IP], ids=["L2", "IP"])
@pytest.mark.parametrize("qtype", [R.QT_8bit, R.QT_8bit_uniform], ids=["8bit", "uniform"])
def test_without_residual_and_every_list_probed_it_is_the_scalar_quantizer(metric, qtype):
    c, xb, lists, xq = IV.edge_corpus(20, "float32")
    m = R.Model(xb, lists, c, qtype, by_residual=False)
    # the tables, codes and decoded rows are the flat scalar quantizer's of the same rows
    trained = SQ.train(xb, qtype)
    assert (m.trained == trained).all()
    assert (m.codes == SQ.encode(xb, trained)).all()
    assert (m.y.view(np.uint32) == SQ.decode(m.codes, trained).view(np.uint32)).all()
    order = IV.store_order(lists)
    ids = np.arange(xb.shape[0], dtype=np.int64)
    for k in (1, 10, 40):
        D, I = m.search(xq, ids, k, len(IV.EDGE_SIZES), metric)
        Ds, Is = SQ.search(xq, np.ascontiguousarray(m.y[order]), k, metric)
        assert (I == order[Is]).all()
        assert (D.view(np.uint32) == Ds.view(np.uint32)).all()


@pytest.mark.parametrize("d", [20, 384])
def test_residual_encoding_decodes_closer_to_the_rows(d):
    c, xb, lists, _ = IV.edge_corpus(d, "float32")
    err = {}
    for by_residual in (True, False):
        m = R.Model(xb, lists, c, R.QT_8bit, by_residual)
        e = np.linalg.norm(m.y.astype(np.float64) - xb.astype(np.float64), axis=1)
        err[by_residual] = e
        # a decoded value lies within half a step of the encoded one (plus the fp32 roundings)
        step = m.trained[d:].astype(np.float64) / 255.0
        r = R.residuals(xb, lists, c, by_residual).astype(np.float64)
        dec = SQ.decode(m.codes, m.trained).astype(np.float64)
        assert (np.abs(dec - r) <= 0.5 * step[None, :] * (1 + 1e-4) + 1e-6).all()
    print(f"d = {d}: mean |y - x| {err[True].mean():.3g} with by_residual, {err[False].mean():.3g} without")
    assert err[True].mean() < 0.5 * err[False].mean()
    assert err[True].max() < err[False].max()


def test_residual_and_reconstruct_are_single_rounded_fp32_operations():
    c, xb, lists, _ = IV.edge_corpus(20, "float32")
    r = R.residuals(xb, lists, c)
    want = (xb.astype(np.float64) - c[lists].astype(np.float64)).astype(np.float32)  # exact difference, one rounding
    assert (r.view(np.uint32) == want.view(np.uint32)).all()
    m = R.Model(xb, lists, c)
    dec = SQ.decode(m.codes, m.trained)
    want = (c[lists].astype(np.float64) + dec.astype(np.float64)).astype(np.float32)
    assert (m.y.view(np.uint32) == want.view(np.uint32)).all()
    # searching one list finds only its rows
    D, I = m.search(c[5:6], np.arange(xb.shape[0]), 400, 1, L2)
    got = I[0][I[0] >= 0]
    assert got.size == IV.EDGE_SIZES[5] and (lists[got] == 5).all()

"""GPU checks of stable external ids: ``IndexIDMap`` / ``IndexIDMap2`` and
``add_with_ids`` on the flat index (fx_idmap.hip and the label translation at
the writers of ``I``, through the C ABI and the Python surface).

The common fixture is a labelled index of 1037 rows (9 tiles, 13 rows in the
last; 33 mask words, the last with 13 rows) added in three ragged
``add_with_ids`` calls (500 + 37 + 500, so growth carries labels), next to a
TWIN unlabelled index of the same rows: bfloat16 and float16 d = 64, float32
d = 32.  The labels are a fixed permutation times 3 plus 100, with every 7th
row repeating an earlier row's label, negatives, values >= 2^40 and one -1.

The expectation everywhere is the twin's answer translated:
``D`` bit-identical and ``I == where(I_twin >= 0, labels[I_twin], -1)``; one
case per dtype is also checked against the CPU oracle directly.
"""
import numpy as np
import pytest

from oracle import cpu as C
from oracle import flat_l2 as F
from tests._data import gaussian_small
from tests.test_gpu_parity import assert_parity

pytestmark = pytest.mark.gpu

N, NQ = 1037, 33
ADDS = (500, 37, 500)
WIDTHS = [("bfloat16", 64), ("float16", 64), ("float32", 32)]
CASES = [(m, dt, d) for m in ("L2", "IP") for dt, d in WIDTHS]
ids_of = lambda p: "-".join(map(str, p))  # noqa: E731
FLT_MAX = F.FLT_MAX


def make_labels(n=N):
    """perm * 3 + 100; rows r % 11 == 3 negative, r % 13 == 5 at 2^40 and above,
    row 18 the one legal -1, and every 7th row the label of row r // 2."""
    perm = np.random.default_rng(77).permutation(n).astype(np.int64)
    lab = perm * 3 + 100
    r = np.arange(n)
    lab[r % 11 == 3] = -(perm[r % 11 == 3] + 5)
    lab[r % 13 == 5] = (1 << 40) + perm[r % 13 == 5]
    lab[18] = -1
    for i in range(7, n, 7):
        lab[i] = lab[i // 2]
    assert (lab == -1).sum() == 1 and (lab < 0).sum() > 50 and (lab >= 1 << 40).sum() > 50 and len(np.unique(lab)) < n
    return lab


LABELS = make_labels()
LABELS.setflags(write=False)


def translate(I, labels):
    I = np.asarray(I)
    return np.where(I >= 0, labels[np.maximum(I, 0)], -1)


@pytest.fixture(scope="module")
def fx():
    from rag_faiss_embedding_amd import _lib, faiss
    if _lib.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    return faiss


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def values():
    xb, xq = gaussian_small()
    v = np.concatenate([xb.ravel(), xq.ravel()])
    v.setflags(write=False)
    return v


def _cut(values, d, n=N, nq=NQ):
    return values[:n * d].reshape(n, d), values[n * d:(n + nq) * d].reshape(nq, d)


def _cls(mod, metric):
    return mod.IndexFlatL2 if metric == "L2" else mod.IndexFlatIP


def build_pair(fx_mod, flat_mod, values, metric, dtype, d, n=N, labels=LABELS, adds=ADDS):
    """(labelled IndexIDMap2 over flat_mod's index, the twin, the queries)."""
    xb, xq = _cut(values, d, n)
    idx = fx_mod.IndexIDMap2(_cls(flat_mod, metric)(d, dtype=dtype))
    r0 = 0
    for a in adds:
        idx.add_with_ids(xb[r0:r0 + a], labels[r0:r0 + a])
        r0 += a
    assert r0 == n and idx.ntotal == n
    twin = _cls(flat_mod, metric)(d, dtype=dtype)
    twin.add(xb)
    return idx, twin, xq


class Pair:
    def __init__(self, fx_mod, values, metric, dtype, d):
        self.metric, self.dtype, self.d = metric, dtype, d
        self.idx, self.twin, self.xq = build_pair(fx_mod, fx_mod, values, metric, dtype, d)
        self.Y = self.twin.reconstruct_n(0, N)
        self.Y.setflags(write=False)


@pytest.fixture(scope="module", params=CASES, ids=ids_of)
def pair(request, fx, values):
    return Pair(fx, values, *request.param)


def oracle(metric, xq, rows, k):
    nq = len(xq)
    D = np.full((nq, k), FLT_MAX if metric == "L2" else -FLT_MAX, dtype=np.float32)
    I = np.full((nq, k), -1, dtype=np.int64)
    kk = min(k, len(rows))
    if kk:
        knn = C.knn_exact if metric == "L2" else F.knn_inner_product
        D[:, :kk], I[:, :kk] = knn(xq, np.ascontiguousarray(rows), kk)
    return D, I


def assert_translated(D, I, Dt, It, labels=LABELS):
    np.testing.assert_array_equal(np.asarray(I), translate(It, labels))
    assert np.asarray(D).tobytes() == np.asarray(Dt).tobytes()


# --------------------------------------------------------------------------
# 1. every writer of I
# --------------------------------------------------------------------------
def test_growth_carried_the_labels(pair):
    np.testing.assert_array_equal(pair.idx.id_map, LABELS)
    assert pair.idx.index.has_ids and not pair.twin.has_ids
    assert (pair.idx.d, pair.idx.ntotal, pair.idx.metric_type, pair.idx.is_trained) == \
        (pair.d, N, pair.twin.metric_type, True)


def test_k10_refine_host_and_oracle(pair):
    """k = 10, nq = 33: k_refine; also against the CPU oracle directly."""
    D, I = pair.idx.search(pair.xq, 10)
    Dt, It = pair.twin.search(pair.xq, 10)
    assert pair.idx.index.last_scan_plan() == pair.twin.last_scan_plan()
    assert pair.idx.index.last_scan_plan()["splits"] < 64  # (not the workgroup refine)
    assert_translated(D, I, Dt, It)
    Dr, Ir = oracle(pair.metric, pair.xq, pair.Y, 10)
    assert_parity(D, I, Dr, translate(Ir, LABELS))


def test_k10_device_in_device_out(pair, torch_cuda):
    t = torch_cuda
    xq = t.from_numpy(np.array(pair.xq)).cuda()
    D, I = pair.idx.search(xq, 10)
    Dt, It = pair.twin.search(xq, 10)
    assert D.is_cuda and I.is_cuda
    assert_translated(D.cpu().numpy(), I.cpu().numpy(), Dt.cpu().numpy(), It.cpu().numpy())


def test_k100_refine_big(pair):
    D, I = pair.idx.search(pair.xq, 100)
    assert_translated(D, I, *pair.twin.search(pair.xq, 100))


def test_k1100_sort_path_pads_past_ntotal(pair, torch_cuda):
    """k > MAX_K: fx_hugek.hip; slots past ntotal stay -1 / +-FLT_MAX."""
    k = 1100
    D, I = pair.idx.search(pair.xq[:5], k)
    Dt, It = pair.twin.search(pair.xq[:5], k)
    assert_translated(D, I, Dt, It)
    assert (It[:, N:] == -1).all() and (I[:, N:] == -1).all()
    pad = FLT_MAX if pair.metric == "L2" else -FLT_MAX
    assert (D[:, N:] == pad).all()
    # every row appears exactly once per query: the multiset of labels is the index's
    np.testing.assert_array_equal(np.sort(I[0, :N]), np.sort(LABELS))
    t = torch_cuda
    xq = t.from_numpy(np.array(pair.xq[:5])).cuda()
    Dd, Id = pair.idx.search(xq, k)
    np.testing.assert_array_equal(Id.cpu().numpy(), I)
    assert Dd.cpu().numpy().tobytes() == D.tobytes()


@pytest.mark.parametrize("case", CASES, ids=ids_of)
@pytest.mark.parametrize("force", [1, 2])
def test_rescan_and_exact_fallback_translate(fx, diag_fx, values, case, force):
    """force_fallback 1: every query through the re-scan (k_refine_big writes the
    slots again); 2: through the exact scan (k_fb_merge)."""
    metric, dtype, d = case
    idx, twin, xq = build_pair(fx, diag_fx, values, metric, dtype, d)
    Dp, Ip = twin.search(xq, 10)  # the plain path's answer
    for ix in (idx.index, twin):
        ix.set_option("force_fallback", force)
    D, I = idx.search(xq, 10)
    counts = (idx.index.last_fallbacks(), idx.index.last_exact_fallbacks())
    assert counts[0] == NQ and (force == 1 or counts[1] == NQ)
    Dt, It = twin.search(xq, 10)
    assert (twin.last_fallbacks(), twin.last_exact_fallbacks()) == counts
    assert_translated(D, I, Dt, It)
    np.testing.assert_array_equal(It, Ip)


@pytest.mark.parametrize("case", [("L2", "bfloat16", 64), ("IP", "float32", 32)], ids=ids_of)
def test_workgroup_refine_translates(fx, values, torch_cuda, case):
    """k_refine_wg: k <= 32, nq <= 256 and >= 64 corpus splits (24,700 rows: 193
    tiles, 8 splits per XCD)."""
    metric, dtype, d = case
    n = 24700
    assert values.size >= (n + NQ) * d
    labels = (np.random.default_rng(5).permutation(n).astype(np.int64) - 9000) * 1000003
    idx, twin, xq = build_pair(fx, fx, values, metric, dtype, d, n=n, labels=labels, adds=(n,))
    xq = xq[:4]
    D, I = idx.search(xq, 10)
    assert idx.index.last_scan_plan()["splits"] >= 64
    Dt, It = twin.search(xq, 10)
    assert twin.last_scan_plan()["splits"] >= 64
    assert_translated(D, I, Dt, It, labels)
    Y = twin.reconstruct_n(0, n)
    Dr, Ir = oracle(metric, xq, Y, 10)
    assert_parity(D, I, Dr, translate(Ir, labels))


# --------------------------------------------------------------------------
# 2. range_search
# --------------------------------------------------------------------------
def test_range_search_translates_in_row_order(pair, torch_cuda):
    Dk, _ = pair.twin.search(pair.xq, 20)
    radius = float(np.median(Dk[:, -1]))  # about 20 rows per query on either metric
    lims, D, I = pair.idx.range_search(pair.xq, radius)
    lt, Dt, It = pair.twin.range_search(pair.xq, radius)
    assert lims[-1] > NQ
    np.testing.assert_array_equal(lims, lt)
    for q in range(NQ):  # the twin's ids are rows: ascending within a query
        assert (np.diff(It[lt[q]:lt[q + 1]]) > 0).all()
    assert_translated(D, I, Dt, It)
    t = torch_cuda
    ld, Dd, Id = pair.idx.range_search(t.from_numpy(np.array(pair.xq)).cuda(), radius)
    np.testing.assert_array_equal(ld.cpu().numpy(), lt.astype(np.int64))
    np.testing.assert_array_equal(Id.cpu().numpy(), I)


# --------------------------------------------------------------------------
# 3. selectors by label
# --------------------------------------------------------------------------
def bitmap_of_rows(mask_rows):
    bits = np.zeros((N + 7) // 8, dtype=np.uint8)
    r = np.flatnonzero(mask_rows)
    np.bitwise_or.at(bits, r >> 3, (1 << (r & 7)).astype(np.uint8))
    return bits


def label_bitmap(nbytes):
    """Bits of every label in [0, 8 nbytes) set, except the multiples of 5."""
    bits = np.zeros(nbytes, dtype=np.uint8)
    lab = np.unique(LABELS[(LABELS >= 0) & (LABELS < 8 * nbytes) & (LABELS % 5 != 0)])
    np.bitwise_or.at(bits, lab >> 3, (1 << (lab & 7)).astype(np.uint8))
    return bits


def selector_cases(fx_mod, torch_mod):
    """(name, selector by label, the rows it selects computed in numpy)."""
    lo, hi = 400, 2100  # a label interval: rows scattered by the permutation
    some = np.concatenate([LABELS[5:60], LABELS[7:9], LABELS[900:1037:3], [-1, 987654321, -(1 << 50), LABELS[14]]])
    few = np.array([LABELS[21], LABELS[21], 424242424242, LABELS[1030]], dtype=np.int64)
    nbytes = 200  # labels below 1600 only: part of the label range
    bits = label_bitmap(nbytes)
    in_bits = (LABELS >= 0) & (LABELS < 8 * nbytes) & (LABELS % 5 != 0)
    return [
        ("range", fx_mod.IDSelectorRange(lo, hi), (LABELS >= lo) & (LABELS < hi)),
        ("batch", fx_mod.IDSelectorBatch(some), np.isin(LABELS, some)),
        ("batch-device", fx_mod.IDSelectorBatch(torch_mod.from_numpy(some).cuda()), np.isin(LABELS, some)),
        ("batch-few", fx_mod.IDSelectorBatch(few), np.isin(LABELS, few)),
        ("bitmap", fx_mod.IDSelectorBitmap(bits), in_bits),
        ("range-negative", fx_mod.IDSelectorRange(-600, 0), (LABELS >= -600) & (LABELS < 0)),
    ]


def test_selectors_by_label(pair, fx, torch_cuda):
    for name, sel, rows in selector_cases(fx, torch_cuda):
        for inverted in (False, True):
            s = fx.IDSelectorNot(sel) if inverted else sel
            m = ~rows if inverted else rows
            assert 0 < m.sum() < N, name
            assert s.stats(pair.idx)["rows"] == int(m.sum()), (name, inverted)
            D, I = pair.idx.search(pair.xq, 10, params=fx.SearchParameters(sel=s))
            Dt, It = pair.twin.search(pair.xq, 10,
                                      params=fx.SearchParameters(sel=fx.IDSelectorBitmap(bitmap_of_rows(m))))
            assert_translated(D, I, Dt, It)
            if name == "batch-few" and not inverted:  # fewer than k members: the rest are missing slots
                assert m.sum() < 10
                assert (I[:, int(m.sum()):] == -1).all() and (It[:, :int(m.sum())] >= 0).all()


def test_selector_against_the_oracle(pair, fx):
    rows = (LABELS >= 400) & (LABELS < 2100)
    D, I = pair.idx.search(pair.xq, 10, params=fx.SearchParameters(sel=fx.IDSelectorRange(400, 2100)))
    Dr, Ir = oracle(pair.metric, pair.xq, pair.Y[rows], 10)
    assert_parity(D, I, Dr, translate(np.where(Ir >= 0, np.flatnonzero(rows)[np.maximum(Ir, 0)], -1), LABELS))


# --------------------------------------------------------------------------
# 4. remove_ids
# --------------------------------------------------------------------------
def apply_removal(twin, keep_rows):
    """Remove ~keep_rows from the twin through a row bitmap (its ids are rows)."""
    gone = ~keep_rows
    bits = np.zeros((len(keep_rows) + 7) // 8, dtype=np.uint8)
    r = np.flatnonzero(gone)
    np.bitwise_or.at(bits, r >> 3, (1 << (r & 7)).astype(np.uint8))
    from rag_faiss_embedding_amd import faiss
    return twin.remove_ids(faiss.IDSelectorBitmap(bits))


@pytest.mark.parametrize("case", [("L2", "bfloat16", 64), ("IP", "float16", 64), ("L2", "float32", 32)], ids=ids_of)
@pytest.mark.parametrize("stage_rows", [0, 3])
def test_remove_ids_by_label(fx, values, case, stage_rows):
    metric, dtype, d = case
    idx, twin, xq = build_pair(fx, fx, values, metric, dtype, d)
    if stage_rows:  # a staging buffer of a few rows' bytes: several chunks
        rb = (d * (4 if dtype == "float32" else 2) + 127) // 128 * 128
        idx.index.set_option("remove_stage", stage_rows * rb)
        twin.set_option("remove_stage", stage_rows * rb)
    lab = LABELS.copy()

    def step(sel_or_ids, gone):
        nonlocal lab
        assert 0 < gone.sum() < len(lab)
        n = idx.remove_ids(sel_or_ids)
        assert n == int(gone.sum()) == apply_removal(twin, ~gone)
        lab = lab[~gone]
        assert idx.ntotal == twin.ntotal == len(lab)
        np.testing.assert_array_equal(idx.id_map, lab)
        D, I = idx.search(xq, 10)
        assert_translated(D, I, *twin.search(xq, 10), labels=lab)

    # a label list with a duplicated label (LABELS[14] == LABELS[7]: both rows go) and an unknown one
    assert LABELS[14] == LABELS[7]
    ids = np.concatenate([LABELS[100:140], [LABELS[14], 55555555555, LABELS[1036]]])
    step(ids, np.isin(lab, ids))
    if stage_rows:
        assert idx.index.last_remove_stats()["chunks"] > 1
    # a range of labels
    step(fx.IDSelectorRange(1000, 1500), (lab >= 1000) & (lab < 1500))
    # an inverted bitmap: everything whose label is NOT in it goes (negatives and 2^40 labels included)
    bits = label_bitmap(420)
    member = (lab >= 0) & (lab < 8 * 420) & (lab % 5 != 0)
    step(fx.IDSelectorNot(fx.IDSelectorBitmap(bits)), ~member)
    # a removal that selects nothing leaves everything, the selector's validity included
    sel = fx.IDSelectorBatch(np.array([77777777777, -123456789], dtype=np.int64))
    resets = idx.index._resets
    assert idx.remove_ids(sel) == 0 and idx.index._resets == resets
    assert sel.stats(idx)["rows"] == 0
    np.testing.assert_array_equal(idx.id_map, lab)
    D, I = idx.search(xq, 10, params=fx.SearchParameters(sel=sel))
    assert (I == -1).all()


# --------------------------------------------------------------------------
# 5. search graph
# --------------------------------------------------------------------------
def test_search_graph_sees_new_labels(fx, values):
    idx, twin, xq = build_pair(fx, fx, values, "L2", "bfloat16", 64)
    idx.index.set_option("search_graph", 1)
    q = xq[:3]
    for _ in range(3):  # eager, captured, replayed
        D0, I0 = idx.search(q, 10)
        assert_translated(D0, I0, *twin.search(q, 10))
    gone = np.unique(I0[:, 0])[:5]  # labels of the nearest rows: the next answer must change
    gone = np.concatenate([gone[gone != -1], np.setdiff1d(LABELS[200:300], gone)])[:5]
    rows_gone = np.isin(LABELS, gone)
    assert idx.remove_ids(gone) == int(rows_gone.sum())
    apply_removal(twin, ~rows_gone)
    lab = LABELS[~rows_gone]
    new_rows = np.ascontiguousarray(q[:1].repeat(5, axis=0) + np.arange(5, dtype=np.float32)[:, None] * 1e-2)
    new_labels = np.array([9001, 9002, -9003, (1 << 41) + 4, 9005], dtype=np.int64)
    idx.add_with_ids(new_rows, new_labels)
    twin.add(new_rows)
    lab = np.concatenate([lab, new_labels])
    for _ in range(3):
        D, I = idx.search(q, 10)
        assert_translated(D, I, *twin.search(q, 10), labels=lab)
        assert not np.isin(I, gone).any()
    assert np.isin(new_labels, I[0]).all()  # the five copies of query 0 are its nearest rows


# --------------------------------------------------------------------------
# 6. rows_of_ids / reconstruct
# --------------------------------------------------------------------------
def last_row_of(labels, ids):
    out = np.full(len(ids), -1, dtype=np.int64)
    for i, v in enumerate(ids):
        r = np.flatnonzero(labels == v)
        if len(r):
            out[i] = r[-1]
    return out


def test_rows_of_ids_and_reconstruct(pair, torch_cuda):
    assert LABELS[14] == LABELS[7] and LABELS[28] == LABELS[14]
    ids = np.array([LABELS[0], LABELS[7], LABELS[1036], 31337, LABELS[7], -1, LABELS[3], 31337, LABELS[1036],
                    LABELS[16], -(1 << 45)], dtype=np.int64)
    want = last_row_of(LABELS, ids)
    assert want[1] > 28 and want[3] == -1 and want[5] == 18  # (row 28's label is repeated again further up)
    flat = pair.idx.index
    np.testing.assert_array_equal(flat.rows_of_ids(ids), want)
    np.testing.assert_array_equal(flat.rows_of_ids(ids[:1]), want[:1])
    rows = flat.rows_of_ids(torch_cuda.from_numpy(ids).cuda())
    np.testing.assert_array_equal(rows.cpu().numpy(), want)
    # every label at once (10 duplicates and all)
    np.testing.assert_array_equal(flat.rows_of_ids(LABELS), last_row_of(LABELS, LABELS))
    assert flat.rows_of_ids(np.zeros(0, dtype=np.int64)).size == 0
    for key in (int(LABELS[0]), int(LABELS[7]), -1, int(LABELS[1036])):
        row = int(last_row_of(LABELS, [key])[0])
        assert pair.idx.reconstruct(key).tobytes() == flat.reconstruct_n(row, 1)[0].tobytes()
    with pytest.raises(RuntimeError):
        pair.idx.reconstruct(31337)
    with pytest.raises(RuntimeError):
        pair.twin.rows_of_ids(ids)  # no labels


# --------------------------------------------------------------------------
# 7. mode rules
# --------------------------------------------------------------------------
def test_mode_rules(fx, values):
    xb, _ = _cut(values, 32, 20)
    flat = fx.IndexFlatL2(32)
    idx = fx.IndexIDMap(flat)
    with pytest.raises(RuntimeError):
        idx.add(xb)
    idx.add_with_ids(xb, np.arange(20) * 10)
    with pytest.raises(RuntimeError):
        flat.add(xb)  # add after add_with_ids
    with pytest.raises(RuntimeError):
        flat.set_id_offset(5)
    with pytest.raises(AssertionError):
        idx.add_with_ids(xb, np.arange(19))
    with pytest.raises(AssertionError):
        fx.IndexIDMap(flat)  # not empty
    assert flat.ntotal == 20 and flat.has_ids
    resets = flat._resets
    idx.reset()
    assert flat._resets == resets + 1 and not flat.has_ids and idx.ntotal == 0
    flat.add(xb)  # reset cleared the mode
    with pytest.raises(RuntimeError):
        flat.add_with_ids(xb, np.arange(20))  # add_with_ids after add
    D, I = flat.search(xb[:2], 1)
    np.testing.assert_array_equal(I[:, 0], [0, 1])
    other = fx.IndexFlatL2(32)
    other.set_id_offset(7)
    with pytest.raises(RuntimeError):
        other.add_with_ids(xb, np.arange(20))
    other.set_id_offset(0)
    other.add_with_ids(xb, np.arange(20) - 5)
    np.testing.assert_array_equal(other.get_ids(), np.arange(20) - 5)


def test_add_with_ids_from_device_tensors_and_normalize(fx, values, torch_cuda):
    t = torch_cuda
    xb, xq = _cut(values, 64, 300)
    lab = LABELS[:300]
    idx = fx.IndexIDMap2(fx.IndexFlatIP(64, dtype="bfloat16", normalize=True))
    idx.add_with_ids(t.from_numpy(np.array(xb[:170])).cuda(), t.from_numpy(lab[:170].copy()).cuda())
    idx.add_with_ids(t.from_numpy(np.array(xb[170:])).cuda().to(t.bfloat16), lab[170:])
    twin = fx.IndexFlatIP(64, dtype="bfloat16", normalize=True)
    twin.add(t.from_numpy(np.array(xb[:170])).cuda())
    twin.add(t.from_numpy(np.array(xb[170:])).cuda().to(t.bfloat16))
    np.testing.assert_array_equal(idx.id_map, lab)
    D, I = idx.search(xq, 10)
    assert_translated(D, I, *twin.search(xq, 10), labels=lab)


# --------------------------------------------------------------------------
# 8. file round trip
# --------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,d", WIDTHS, ids=lambda p: str(p))
def test_file_round_trip(fx, values, tmp_path, dtype, d):
    idx, twin, xq = build_pair(fx, fx, values, "L2", dtype, d)
    path = tmp_path / "labelled.index"
    fx.write_index(idx, str(path))
    raw = path.read_bytes()
    assert raw[:4] == b"IxM2" and raw[37:41] == b"IxF2"
    assert len(raw) == 37 + 45 + N * d * 4 + 8 + N * 8
    assert np.frombuffer(raw[-N * 8:], dtype=np.int64).tolist() == LABELS.tolist()
    back = fx.read_index(str(path), dtype=dtype)
    assert isinstance(back, fx.IndexIDMap2) and back.ntotal == N
    np.testing.assert_array_equal(back.id_map, LABELS)
    D, I = idx.search(xq, 10)
    Db, Ib = back.search(xq, 10)
    np.testing.assert_array_equal(Ib, I)
    assert Db.tobytes() == D.tobytes()
    cut = tmp_path / "cut.index"
    for c in (0, 3, 4, 36, 37, 41, 81, 82, 82 + N * d * 4 - 1, 82 + N * d * 4, 82 + N * d * 4 + 8, len(raw) - 1):
        cut.write_bytes(raw[:c])
        with pytest.raises(RuntimeError):
            fx.read_index(str(cut), dtype=dtype)
    # a plain file still reads as a plain index
    plain = tmp_path / "plain.index"
    fx.write_index(twin, str(plain))
    assert plain.read_bytes() == raw[37:37 + 45 + N * d * 4]
    p = fx.read_index(str(plain), dtype=dtype)
    assert isinstance(p, fx.IndexFlatL2) and not p.has_ids and p.ntotal == N
    np.testing.assert_array_equal(p.search(xq, 10)[1], twin.search(xq, 10)[1])

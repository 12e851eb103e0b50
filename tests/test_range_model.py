"""CPU model of range_search's filter threshold (fx_range.hip k_range_thr) and
the host logic of its Python callers.

The MFMA pass of range_search keeps a (query, row) pair when its scan key is
<= T_q; the exact pass then decides membership.  The filter is sound when no
pair with exact D < R has a key > T_q.  With k_prep_queries in its no-image
mode (mu = 0, srcC = |y|^2; restated below) and a(y) the key,

    a(y) + s_q = D(y) + 2 r.(y - x) + err,  |2 r.(y - x)| <= 2 rho sqrt(D),  |err| <= E
    L2:  T_q = R - s_q + 2 rho sqrt(R) + E         IP:  T_q = -R + E

in fp64, rounded up to fp32.  Here the operands are rounded to bf16 / fp16
through torch on the CPU, the keys are accumulated in fp32 as the MFMA chain
does (one rounding per exact product; both "onto |y|^2" and "sum, then +
|y|^2", the order k_range_scan's epilogue uses), and the claim is checked
pair by pair on gaussian, clustered and large-norm data.

The callers (FAISSVectorStore.search_radius, retrieval.documents_within,
RetrievalEngine.search_within) run over a numpy stand-in for the index.
"""
import importlib
import sqlite3

import numpy as np
import pytest
import torch

from oracle.flat_l2 import synth
from rag_faiss_embedding_amd import retrieval as R

U = 2.0 ** -24


def rn(x, dt):
    """fp32 -> storage dtype -> fp32, through torch on the CPU."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if dt == "f32":
        return x
    tdt = torch.bfloat16 if dt == "bf16" else torch.float16
    return torch.from_numpy(x).to(tdt).to(torch.float32).numpy()


def prep(x, M, Smax, K, dt, metric):
    """k_prep_queries without an image (mu = 0), restated: operand, E, rho, s_q
    as the kernel stores them (E and rho as fp32, inflated as there)."""
    op = rn(x, dt)
    x64, op64 = x.astype(np.float64), op.astype(np.float64)
    r = x64 - op64
    rr, rx, xn2 = np.sum(r * r), np.dot(r, x64), np.sum(x64 * x64)
    on = np.sqrt(np.sum(op64 * op64))
    gamma = (K + 1) * U / (1 - (K + 1) * U)
    if metric == "l2":
        E = U * Smax * 1.01 + gamma * (Smax * 1.01 + 2.0 * M * on) + 1e-12 * (xn2 + 2.0 * abs(rx))
        shift, rho = xn2 - 2.0 * rx, np.sqrt(rr)
    else:
        E = (gamma + U) * on * M + np.sqrt(rr) * M
        shift, rho = 0.0, 0.0
    return op, float(np.float32(E * 1.0625 + 1e-30)), float(np.float32(rho * 1.0000002)), shift


def threshold(R_, E, rho, shift, metric):
    """k_range_thr restated."""
    R64 = float(np.float32(R_))
    T = R64 - shift + 2.0 * rho * np.sqrt(R64) + E if metric == "l2" else -R64 + E
    T += 1e-15 * abs(T)
    f = np.float32(T)
    if float(f) < T:
        f = np.nextafter(f, np.float32(np.inf))
    return f


def scan_keys(Y, op, metric, onto_norm):
    """The fp32 MFMA chain: one rounding per product y_k * (s op_k), s = -2
    (L2) or -1 (IP); L2 adds |y|^2 (fp64 sum, one rounding) first or last."""
    S = np.sum(Y.astype(np.float64) ** 2, axis=1).astype(np.float32)
    B = ((-2.0 if metric == "l2" else -1.0) * op).astype(np.float32)
    acc = S.copy() if (metric == "l2" and onto_norm) else np.zeros(len(Y), np.float32)
    for k in range(Y.shape[1]):
        acc = (acc.astype(np.float64) + Y[:, k].astype(np.float64) * np.float64(B[k])).astype(np.float32)
    if metric == "l2" and not onto_norm:
        acc = (acc.astype(np.float64) + S.astype(np.float64)).astype(np.float32)
    return acc, S


def _data(kind, rng, n, d):
    if kind == "gaussian":
        return rng.standard_normal((n, d)), rng.standard_normal((8, d))
    if kind == "clustered":
        base = rng.standard_normal(d)
        base /= np.linalg.norm(base)
        Y = base + 0.05 * rng.standard_normal((n, d)) / np.sqrt(d)
        return Y / np.linalg.norm(Y, axis=1, keepdims=True), base + 0.05 * rng.standard_normal((8, d)) / np.sqrt(d)
    return 30.0 + 0.01 * rng.standard_normal((n, d)), 30.0 + 0.01 * rng.standard_normal((8, d))  # large norm


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("kind", ["gaussian", "clustered", "large_norm"])
def test_no_row_inside_the_radius_is_filtered_out(kind, dt, metric):
    rng = np.random.default_rng({"gaussian": 5, "clustered": 6, "large_norm": 7}[kind])
    n, d = 1500, 96
    Y, Xq = _data(kind, rng, n, d)
    Y = rn(Y.astype(np.float32), dt)        # the stored rows
    Xq = Xq.astype(np.float32)              # fp32 queries, inexact in 16 bits
    Y64 = Y.astype(np.float64)
    M = float(np.sqrt(np.max(np.sum(Y64 ** 2, axis=1))))
    inside = tight = 0
    for x in Xq:
        if metric == "l2":
            D = np.sum((x.astype(np.float64) - Y64) ** 2, axis=1).astype(np.float32)
        else:
            D = (Y64 @ x.astype(np.float64)).astype(np.float32)
        for onto_norm in (True, False):
            op, _, _, _ = prep(x, M, 0.0, d, dt, metric)
            a, S = scan_keys(Y, op, metric, onto_norm)
            op, E, rho, shift = prep(x, M, float(S.max()), d, dt, metric)
            # radii: attained values (the strict edge) and points between
            for quant in (0.0, 0.01, 0.3, 0.5, 1.0):
                Rv = np.float32(np.quantile(D, quant if metric == "l2" else 1.0 - quant))
                for Rr in (Rv, np.nextafter(Rv, np.float32(np.inf)), np.nextafter(Rv, np.float32(-np.inf))):
                    if metric == "l2" and Rr <= 0:
                        continue
                    T = threshold(Rr, E, rho, shift, metric)
                    member = D < Rr if metric == "l2" else D > Rr
                    assert (a[member] <= T).all(), (kind, dt, metric, float(Rr), float((a[member] - T).max()))
                    inside += int(member.sum())
                    tight += int((a <= T).sum())
    assert inside > 0
    print(f"\n[range-model] {kind} {dt} {metric}: candidates / members = {tight / inside:.3f}")


def test_threshold_edges():
    # an unusable bound (overflowed fp16 operand: E = +inf) lets every row through
    assert threshold(1.0, np.inf, 0.0, 3.0, "l2") == np.inf
    assert threshold(1.0, np.inf, 0.0, 0.0, "ip") == np.inf
    # rounded up, never down
    T = threshold(1.0, 1e-9, 0.0, 0.25, "l2")
    assert float(T) >= 1.0 - 0.25 + 1e-9 and T.dtype == np.float32


# ---------------------------------------------------------------------------
# callers over a numpy stand-in for the index
# ---------------------------------------------------------------------------
class _RangeIndex:
    """IndexFlatL2.range_search restated in numpy (exact arithmetic: the rows
    come from the integer-grid generator)."""
    metric_type = 1

    def __init__(self, xb):
        self.xb = np.ascontiguousarray(xb, dtype=np.float32)
        self.calls = 0

    @property
    def d(self):
        return self.xb.shape[1]

    @property
    def ntotal(self):
        return self.xb.shape[0]

    def add(self, x):
        self.xb = np.vstack([self.xb, np.ascontiguousarray(x, dtype=np.float32)])

    def range_search(self, x, radius):
        self.calls += 1
        x = np.atleast_2d(np.asarray(x, dtype=np.float32))
        assert x.shape[1] == self.xb.shape[1], "dimension mismatch"
        D = ((x[:, None, :].astype(np.float64) - self.xb[None].astype(np.float64)) ** 2).sum(-1).astype(np.float32)
        hit = D < np.float32(radius)
        lims = np.concatenate([[0], np.cumsum(hit.sum(1))]).astype(np.uint64)
        qi, ri = np.nonzero(hit)
        return lims, D[qi, ri], ri.astype(np.int64)


class _CountingStore(R.DocumentStore):
    fetches = 0

    def fetch_many(self, ids):
        self.fetches += 1
        return super().fetch_many(ids)


def _db(n):
    conn = sqlite3.connect(":memory:")
    conn.execute("CREATE TABLE documents (id INTEGER PRIMARY KEY, url TEXT UNIQUE, title TEXT, content TEXT,"
                 " created_at TEXT, updated_at TEXT)")
    conn.executemany("INSERT INTO documents VALUES (?,?,?,?,?,?)",
                     [(i, f"u{i}", f"t{i}", f"c{i}", "2024", "2024") for i in range(1, n + 1)])
    return conn


@pytest.fixture(scope="module")
def corpus():
    xb = synth(7, 0, 60, 32)
    xb[40] = xb[3]  # an exact tie in distance to any query: order falls back to the row
    xq = synth(11, 0, 3, 32)
    D = ((xq[:, None, :].astype(np.float64) - xb[None].astype(np.float64)) ** 2).sum(-1).astype(np.float32)
    return xb, xq, D


def test_min_score_maps_to_radius():
    assert R.radius_for_score(1.0) == 0.0
    assert R.radius_for_score(0.5) == 1.0
    assert R.radius_for_score(0.25) == 3.0
    for bad in (0.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            R.radius_for_score(bad)


def test_documents_within_matches_a_host_filter(corpus):
    xb, xq, D = corpus
    doc_ids = list(range(101, 101 + 50))   # rows 50..59 have no id: filtered like search
    store = _CountingStore(_db(140))       # ids 141..150 have no document: dropped
    index = _RangeIndex(xb)
    radius = float(np.sort(D.ravel())[40])
    got = R.documents_within(index, doc_ids, store, xq, max_distance=radius)
    assert index.calls == 1 and store.fetches == 1
    assert len(got) == 3 and sum(len(g) for g in got) > 0
    for qi, row in enumerate(got):
        want = sorted((float(D[qi, r]), r) for r in range(60)
                      if D[qi, r] < np.float32(radius) and r < 50 and doc_ids[r] <= 140)
        assert [d["id"] for d in row] == [doc_ids[r] for _, r in want]
        assert [d["distance"] for d in row] == [dv for dv, _ in want]
        assert [d["score"] for d in row] == [R.similarity(dv) for dv, _ in want]
        assert [d["distance"] for d in row] == sorted(d["distance"] for d in row)
    # min_score s is the radius 1/s - 1
    s = 1.0 / (1.0 + radius)
    assert R.documents_within(index, doc_ids, store, xq, min_score=s) == \
        R.documents_within(index, doc_ids, store, xq, max_distance=R.radius_for_score(s))


def test_documents_within_ties_order_by_row():
    xb = synth(7, 0, 60, 32)
    xb[40] = xb[3]
    index = _RangeIndex(xb)
    got = R.documents_within(index, list(range(1, 61)), R.DocumentStore(_db(60)), xb[3:4], max_distance=1e-3)
    assert [d["id"] for d in got[0]] == [4, 41] and [d["distance"] for d in got[0]] == [0.0, 0.0]


def test_documents_within_swallows_errors(corpus):
    xb, xq, _ = corpus
    index, store = _RangeIndex(xb), R.DocumentStore(_db(10))
    ids = list(range(1, 61))
    assert R.documents_within(index, ids, store, xq) == [[], [], []]                                 # neither given
    assert R.documents_within(index, ids, store, xq, max_distance=1.0, min_score=0.5) == [[], [], []]  # both given
    assert R.documents_within(index, ids, store, xq, min_score=0.0) == [[], [], []]
    assert R.documents_within(index, ids, store, xq[:, :5], max_distance=1.0) == [[], [], []]        # dimension
    index.metric_type = 0
    assert R.documents_within(index, ids, store, xq, min_score=0.5) == [[], [], []]                  # score needs L2


def test_engine_search_within(corpus):
    xb, xq, D = corpus

    class _Vec:
        def generate_embeddings(self, texts):
            return xq[: len(texts)]

    eng = R.RetrievalEngine(_Vec(), _RangeIndex(xb), list(range(1, 61)), R.DocumentStore(_db(60)))
    radius = float(np.sort(D.ravel())[25])
    assert eng.search_within([], max_distance=radius) == []
    got = eng.search_within(["a", "b"], max_distance=radius)
    assert got == R.documents_within(eng.index, eng.doc_ids, eng.store, xq[:2], max_distance=radius)
    assert sum(len(g) for g in got) == int((D[:2] < np.float32(radius)).sum())


@pytest.fixture()
def store_mod(monkeypatch):
    fs = importlib.import_module("rag_faiss_embedding_amd.faiss_store")

    class _FakeFx:
        @staticmethod
        def IndexFlatL2(d, dtype="float32", device=0):
            return _RangeIndex(np.zeros((0, d), np.float32))

    monkeypatch.setattr(fs, "_fx", _FakeFx)
    monkeypatch.setattr(fs.FAISSVectorStore, "_instance", None)
    monkeypatch.setattr(fs.FAISSVectorStore, "_initialized", False)
    return fs


def test_store_search_radius(store_mod, corpus, tmp_path):
    xb, xq, D = corpus
    store = store_mod.FAISSVectorStore(dimension=32, index_path=str(tmp_path / "none.bin"))
    store.add_vectors(xb, list(range(500, 550)))  # 50 ids for 60 rows, as the reference allows
    radius = float(np.sort(D[0])[20])
    dist, ids = store.search_radius(xq[0], radius)
    want = sorted((float(D[0, r]), r) for r in range(50) if D[0, r] < np.float32(radius))
    assert ids == [500 + r for _, r in want] and len(ids) > 0
    np.testing.assert_array_equal(dist, np.float32([dv for dv, _ in want]))
    assert dist.dtype == np.float32
    d2, ids2 = store.search_radius(list(map(float, xq[0])), radius)     # a list, as search takes
    assert ids2 == ids and (d2 == dist).all()
    dist, ids = store.search_radius(xq[0], 0.0)                         # nothing inside
    assert ids == [] and dist.size == 0
    dist, ids = store.search_radius(xq[0][:5], radius)                  # error -> swallowed
    assert ids == [] and dist.size == 0 and dist.dtype == np.float64

"""GPU checks of what IndexScalarQuantizer, IndexPQ, IndexIVFFlat and
IndexIVFScalarQuantizer share on the host side (the handle core, the code-row
store, the counts and the profile), on the paths no other test reaches: the
profile's bookkeeping, counts left pending by a device search, a switch of
streams between searches, growth across the first capacity and its 1.5x step,
and the search of an empty index.

One shape for every kind: d = 32, 300 rows (two 128-row tiles and a partial
one), 3 queries, k = 4, seeded normal data; PQ with M = 4 (dsub = 8: the gather
scan), the inverted files with 4 lists (four centroids in a flat quantizer) and
nprobe = 2.  References: tests/_sq_ref.py and tests/_pq_ref.py for the decoded
rows, the oracle's exact k-NN over them (restricted, for the inverted files, to
the rows of each query's two nearest lists); ids equal, distances within
1e-5 * max(1, |D_ref|)."""
import numpy as np
import pytest

from oracle import cpu as C
from tests import _pq_ref as P
from tests import _sq_ref as S

pytestmark = pytest.mark.gpu

KINDS = ["sq", "pq", "ivf", "ivfsq"]
D_, N, NQ, K, M, NLIST, NPROBE = 32, 300, 3, 4, 4, 4, 2
FLT_MAX = np.finfo(np.float32).max


@pytest.fixture(scope="module")
def fx():
    from rag_faiss_embedding_amd import _lib, faiss
    if _lib.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    return faiss


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def data():
    """Rows, queries, centroids, the trainings, and per kind the expected (D, I)
    of the L2 search (ids: row numbers; the inverted files' are 1000 + row)."""
    rng = np.random.default_rng(0)
    xb = rng.standard_normal((N, D_)).astype(np.float32)
    xq = rng.standard_normal((NQ, D_)).astype(np.float32)
    cents = rng.standard_normal((NLIST, D_)).astype(np.float32)
    tables = S.train(xb)
    books = P.sampled_centroids(xb, M)
    dec = {"sq": S.decode(S.encode(xb, tables), tables), "pq": P.decode(P.encode(xb, books), books), "ivf": xb}
    dec["ivfsq"] = dec["sq"]  # (by_residual = False: the rows themselves are quantised)
    row_list = C.knn_exact(xb, cents, 1)[1][:, 0]
    probes = C.knn_exact(xq, cents, NPROBE)[1]
    want = {}
    for kind in KINDS:
        if kind in ("sq", "pq"):
            want[kind] = S.search(xq, dec[kind], K)
            continue
        Dr, Ir = np.empty((NQ, K), np.float32), np.empty((NQ, K), np.int64)
        for i in range(NQ):
            rows = np.flatnonzero(np.isin(row_list, probes[i]))
            assert rows.size >= K
            Di, Ii = S.search(xq[i:i + 1], dec[kind][rows], K)
            Dr[i], Ir[i] = Di[0], 1000 + rows[Ii[0]]
        want[kind] = (Dr, Ir)
    return {"xb": xb, "xq": xq, "cents": cents, "tables": tables, "books": books, "want": want}


def trained(fx, data, kind, l2=True):
    """A trained index of `kind` that holds no rows."""
    metric = fx.METRIC_L2 if l2 else fx.METRIC_INNER_PRODUCT
    if kind == "sq":
        ix = fx.IndexScalarQuantizer(D_, fx.ScalarQuantizer.QT_8bit, metric)
        ix.set_trained(data["tables"])
        return ix
    if kind == "pq":
        ix = fx.IndexPQ(D_, M, 8, metric)
        ix.pq.centroids = data["books"]
        return ix
    quant = (fx.IndexFlatL2 if l2 else fx.IndexFlatIP)(D_)
    quant.add(data["cents"])
    if kind == "ivf":
        ix = fx.IndexIVFFlat(quant, D_, NLIST, metric)
    else:
        ix = fx.IndexIVFScalarQuantizer(quant, D_, NLIST, fx.ScalarQuantizer.QT_8bit, metric, by_residual=False)
        ix.set_trained(data["tables"])
    ix.nprobe = NPROBE
    return ix


def filled(fx, data, kind, steps=(N,)):
    """... with the rows added in `steps`."""
    ix, r0 = trained(fx, data, kind), 0
    for n in steps:
        if kind in ("sq", "pq"):
            ix.add(data["xb"][r0:r0 + n])
        else:
            ix.add_with_ids(data["xb"][r0:r0 + n], 1000 + np.arange(r0, r0 + n, dtype=np.int64))
        r0 += n
    assert ix.ntotal == sum(steps)
    return ix


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(got, want, what):
    assert (got[1] == want[1]).all(), f"{what}: ids differ"
    assert (bits(got[0]) == bits(want[0])).all(), f"{what}: distance bits differ"


@pytest.mark.parametrize("kind", KINDS)
def test_profile(fx, data, kind):
    ix = filled(fx, data, kind)
    ix.profile(True)
    ix.search(data["xq"], K)
    ix.search(data["xq"], K)
    r = ix.profile_read()
    assert r.pop("passes") == 2, r
    assert len(r) == (3 if kind in ("sq", "pq") else 4)
    assert all(np.isfinite(v) and v >= 0 for v in r.values()), r
    again = ix.profile_read()
    assert again.pop("passes") == 0 and all(v == 0 for v in again.values()), again
    ix.profile(False)
    ix.search(data["xq"], K)
    assert ix.profile_read()["passes"] == 0


@pytest.mark.parametrize("kind", KINDS)
def test_counts_after_device_search(fx, torch, data, kind):
    ix = filled(fx, data, kind)
    ix.search(torch.from_numpy(data["xq"]).cuda(), K)  # (leaves the counts pending)
    assert ix.last_fallbacks() >= 0 and ix.last_exact_fallbacks() >= 0
    assert ix.last_dropped_candidates() == 0


@pytest.mark.parametrize("kind", KINDS)
def test_stream_switch(fx, torch, data, kind):
    ix = filled(fx, data, kind)
    first = ix.search(data["xq"], K)
    xq = torch.from_numpy(data["xq"]).cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        Dd, Id = ix.search(xq, K)
    s.synchronize()
    third = ix.search(data["xq"], K)
    same((Dd.cpu().numpy(), Id.cpu().numpy()), first, f"{kind}: device search on another stream")
    same(third, first, f"{kind}: host search after it")
    Dr, Ir = data["want"][kind]
    assert (first[1] == Ir).all(), f"{kind}: ids differ from the reference: {first[1]} vs {Ir}"
    err = np.abs(first[0].astype(np.float64) - Dr.astype(np.float64))
    assert (err <= 1e-5 * np.maximum(1.0, np.abs(Dr))).all(), f"{kind}: distances off by {err.max()}"
    assert ix.last_dropped_candidates() == 0


@pytest.mark.parametrize("kind", KINDS)
def test_growth(fx, data, kind):
    # capacities 256 -> 384 -> 640 rows: the second add outgrows the first, the third takes the 1.5x step
    parts, whole = filled(fx, data, kind, (100, 100, 100)), filled(fx, data, kind)
    same(parts.search(data["xq"], K), whole.search(data["xq"], K), f"{kind}: three adds against one")
    if kind in ("sq", "pq"):
        assert (bits(parts.reconstruct_n()) == bits(whole.reconstruct_n())).all(), f"{kind}: reconstruct_n differs"


@pytest.mark.parametrize("l2", [True, False], ids=["L2", "IP"])
@pytest.mark.parametrize("kind", KINDS)
def test_empty_index(fx, torch, data, kind, l2):
    ix = trained(fx, data, kind, l2)
    fill = FLT_MAX if l2 else -FLT_MAX
    Dh, Ih = ix.search(data["xq"], K)
    Dd, Id = ix.search(torch.from_numpy(data["xq"]).cuda(), K)
    for what, D, I in (("host", Dh, Ih), ("device", Dd.cpu().numpy(), Id.cpu().numpy())):
        assert D.shape == (NQ, K) and (I == -1).all() and (D == fill).all(), f"{kind} {what}: {D} {I}"

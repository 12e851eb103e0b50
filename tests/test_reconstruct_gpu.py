"""GPU checks of reconstruct_batch / search_and_reconstruct /
compute_distance_subset (fx_recon.hip through the C ABI and the Python layers).

The corpora are the integer-grid generator's (every value k/64, |k| <= 255:
exact in fp32, bf16 and fp16), so a gathered vector must equal the input row
bit for bit in every storage dtype, and N = sum (dk)^2 in int64 gives the
library's distance float32(N / 4096) exactly (fp64 sum of multiples of 1/4096
below 2^53, one rounding).  The gaussian case is held to the project's bar
1e-5 * max(1, |D|) against an fp64 numpy value from the index's own rows.

One case of the issue is not expressible: "after remove_ids of the LATER
duplicate, reconstruct(dup) returns the earlier one".  On a labelled index a
selector speaks labels, so two rows sharing a label are always removed
together; test_labels removes other rows instead and checks that the label
still answers with its last row (now renumbered)."""
import ctypes

import numpy as np
import pytest

from oracle.flat_l2 import synth
from tests._data import gaussian_small

pytestmark = pytest.mark.gpu

RTOL = 1e-5
FLT_MAX = np.finfo(np.float32).max
GATHER = [(384, "float32"), (768, "bfloat16"), (64, "bfloat16"), (100, "float16")]
NT = 5000


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
def corpus():
    """d -> the read-only 5000 x d grid corpus, computed once."""
    cache = {}

    def get(d):
        if d not in cache:
            cache[d] = synth(7, 0, NT, d)
            cache[d].setflags(write=False)
        return cache[d]
    return get


@pytest.fixture(scope="module")
def indexes(fx, corpus):
    """(d, dtype[, metric]) -> one 5000-row index, shared by the read-only tests."""
    cache = {}

    def get(d, dtype, ip=False):
        key = (d, dtype, ip)
        if key not in cache:
            ix = (fx.IndexFlatIP if ip else fx.IndexFlatL2)(d, dtype=dtype)
            ix.add(corpus(d))
            cache[key] = ix
        return cache[key]
    return get


def grid_dist(xq, xb):
    """Exact squared distances of integer-grid rows: float32(N / 4096)."""
    a = np.rint(xq.astype(np.float64) * 64).astype(np.int64)
    b = np.rint(xb.astype(np.float64) * 64).astype(np.int64)
    N = (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2 * (a @ b.T)
    assert (N >= 0).all()
    return (N.astype(np.float64) / 4096.0).astype(np.float32), N


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    assert a.dtype == b.dtype == np.float32 and a.shape == b.shape
    np.testing.assert_array_equal(bits(a), bits(b))


def tdtype(torch, name):
    return getattr(torch, name)


def raw16(torch, t):
    """A tensor's bytes as integers (bitwise comparison of any float dtype)."""
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def make_keys(n, ntotal, seed):
    keys = np.random.default_rng(seed).integers(0, ntotal, size=n).astype(np.int64)
    if n >= 1:
        keys[-1] = ntotal - 1
    if n >= 2:
        keys[0] = 0
    if n >= 4:
        keys[n // 2] = keys[1]  # a repeat
    return keys


# ---- gather --------------------------------------------------------------------
@pytest.mark.parametrize("d,dtype", GATHER)
def test_gather_bitwise(fx, torch, corpus, indexes, d, dtype):
    xb, ix = corpus(d), indexes(d, dtype)
    full = ix.reconstruct_n(0, NT)
    same_bits(full, xb)  # (the grid is exact in the storage dtype)
    stored = torch.tensor(xb).to(tdtype(torch, dtype)).cuda()
    for n in (0, 1, 63, 64, 65, 1000):
        keys = make_keys(n, NT, seed=n)
        host = ix.reconstruct_batch(keys)
        assert host.shape == (n, d)
        same_bits(host, xb[keys])
        same_bits(host, full[keys])
        tk = torch.from_numpy(keys).cuda()
        dev = ix.reconstruct_batch(tk)
        assert dev.is_cuda and dev.dtype == torch.float32 and tuple(dev.shape) == (n, d)
        same_bits(dev.cpu().numpy(), xb[keys])
        st = ix.reconstruct_batch(tk, dtype="storage")
        assert st.dtype == tdtype(torch, dtype) and tuple(st.shape) == (n, d)
        assert torch.equal(raw16(torch, st), raw16(torch, stored[tk]))
    same_bits(ix.reconstruct(NT - 1), xb[NT - 1])


@pytest.mark.parametrize("d,dtype", [(100, "float16"), (384, "float32")])
def test_gather_one_row_and_after_removal(fx, torch, corpus, d, dtype):
    xb = corpus(d)
    one = fx.IndexFlatL2(d, dtype=dtype)
    one.add(xb[:1])
    same_bits(one.reconstruct_batch([0, 0]), xb[[0, 0]])
    same_bits(one.reconstruct_batch(torch.zeros(3, dtype=torch.int64, device="cuda")).cpu().numpy(), xb[[0, 0, 0]])
    ix = fx.IndexFlatL2(d, dtype=dtype)
    ix.add(xb[:300])
    gone = [0, 5, 128, 299]
    assert ix.remove_ids(np.array(gone, dtype=np.int64)) == 4
    kept = np.delete(np.arange(300), gone)
    full = ix.reconstruct_n(0, ix.ntotal)
    same_bits(full, xb[kept])
    keys = make_keys(65, ix.ntotal, seed=3)  # keys mean the NEW row numbers
    same_bits(ix.reconstruct_batch(keys), full[keys])
    same_bits(ix.reconstruct_batch(torch.from_numpy(keys).cuda()).cpu().numpy(), full[keys])
    with pytest.raises(RuntimeError):
        ix.reconstruct_batch([296])  # a row number of before the removal


# ---- bounds -----------------------------------------------------------------------
BAD = [-1, NT, -2 ** 63, 2 ** 40, 3]


@pytest.mark.parametrize("d,dtype", [(384, "float32"), (768, "bfloat16"), (100, "float16")])
def test_bad_device_keys_give_nan_rows(fx, torch, corpus, indexes, d, dtype):
    xb, ix = corpus(d), indexes(d, dtype)
    tk = torch.tensor(BAD, dtype=torch.int64, device="cuda")
    out = ix.reconstruct_batch(tk).cpu().numpy()  # (returns: the call's code was 0)
    assert (bits(out[:4]) == 0xFFFFFFFF).all() and np.isnan(out[:4]).all()
    same_bits(out[4], xb[3])
    st = ix.reconstruct_batch(tk, dtype="storage")
    raw = raw16(torch, st).cpu().numpy()
    assert (raw[:4] == -1).all()  # every bit set: 0xFFFF / 0xFFFFFFFF
    assert torch.equal(raw16(torch, st[4]), raw16(torch, torch.tensor(xb[3]).to(st.dtype).cuda()))


def test_bad_host_keys_are_an_argument_error(fx, corpus, indexes):
    from rag_faiss_embedding_amd import _lib
    ix = indexes(384, "float32")
    keys = np.array(BAD, dtype=np.int64)
    out = np.full((5, 384), 7.5, dtype=np.float32)
    rc = ix._lib.fx_index_reconstruct_batch(ix._h, 5, ctypes.c_void_p(keys.ctypes.data), _lib.MEM_HOST,
                                            ctypes.c_void_p(out.ctypes.data), _lib.F32, _lib.MEM_HOST)
    assert rc == -1 and "key -1 " in _lib.last_error()  # the first bad key is named
    assert (out == 7.5).all()  # nothing was written
    with pytest.raises(RuntimeError, match="key 5000 "):
        ix.reconstruct_batch([3, NT])
    # out_dtype: fp32 or the storage dtype only
    rc = ix._lib.fx_index_reconstruct_batch(ix._h, 1, ctypes.c_void_p(keys[4:].ctypes.data), _lib.MEM_HOST,
                                            ctypes.c_void_p(out.ctypes.data), _lib.F16, _lib.MEM_HOST)
    assert rc == -4 and (out == 7.5).all()


def test_id_offset_shifts_the_keys(fx, torch, corpus):
    xb = corpus(64)[:300]
    ix = fx.IndexFlatL2(64, dtype="bfloat16")
    ix.add(xb)
    ix.set_id_offset(1000)
    same_bits(ix.reconstruct_batch([1000, 1299]), xb[[0, 299]])
    with pytest.raises(RuntimeError, match="key 0 "):
        ix.reconstruct_batch([0])
    out = ix.reconstruct_batch(torch.tensor([1000, 0, 1299, 1300, 999], dtype=torch.int64, device="cuda")).cpu().numpy()
    same_bits(out[[0, 2]], xb[[0, 299]])
    assert (bits(out[[1, 3, 4]]) == 0xFFFFFFFF).all()
    # search_and_reconstruct and compute_distance_subset speak the shifted ids too
    D, I, R = ix.search_and_reconstruct(xb[:3], 2)
    assert I[:, 0].tolist() == [1000, 1001, 1002] and (D[:, 0] == 0).all()
    same_bits(R, xb[I - 1000])
    same_bits(ix.compute_distance_subset(xb[:3], I), D)


# ---- labels -------------------------------------------------------------------------
def test_labels(fx, torch, corpus):
    d, n = 64, 200
    xb = corpus(d)[:n]
    assert len({r.tobytes() for r in xb}) == n  # distinct rows
    labels = np.arange(n, dtype=np.int64) * 3 + 11
    labels[0], labels[1] = -5, 2 ** 40 + 3
    dup, unknown = 777, 123456
    labels[10] = labels[150] = dup  # one label on two different rows
    idx = fx.IndexIDMap2(fx.IndexFlatL2(d))
    idx.add_with_ids(xb, labels)
    plain = fx.IndexFlatL2(d)
    plain.add(xb)
    # reconstruct_batch: the last row added with a label; an unknown label: NaN
    keys = np.array([dup, -5, 2 ** 40 + 3, unknown, dup, labels[199]], dtype=np.int64)
    want = xb[[150, 0, 1, 0, 150, 199]]
    for got in (idx.reconstruct_batch(keys), idx.reconstruct_batch(torch.from_numpy(keys).cuda()).cpu().numpy()):
        same_bits(got[[0, 1, 2, 4, 5]], want[[0, 1, 2, 4, 5]])
        assert (bits(got[3]) == 0xFFFFFFFF).all()
    same_bits(idx.reconstruct(dup), xb[150])
    with pytest.raises(RuntimeError, match="not found"):
        idx.reconstruct(unknown)
    # search_and_reconstruct: the vector of the ROW that ranked, also where its label repeats
    xq = np.concatenate([xb[10:11], xb[150:151], synth(11, 0, 5, d)])
    D, I, R = idx.search_and_reconstruct(xq, 6)
    Dp, Ip = plain.search(xq, 6)
    same_bits(D, Dp)
    np.testing.assert_array_equal(I, labels[Ip])
    same_bits(R, xb[Ip])
    assert D[0, 0] == 0 and I[0, 0] == dup and Ip[0, 0] == 10  # the EARLIER duplicate's own vector
    same_bits(R[0, 0], xb[10])
    Dl, Il = idx.search(xq, 6)  # ... and exactly search's D and I
    same_bits(D, Dl)
    np.testing.assert_array_equal(I, Il)
    # compute_distance_subset with labels as keys
    G, _ = grid_dist(xq, xb)
    ck = np.array([[dup, -5, unknown, -1]] * len(xq), dtype=np.int64)
    want = np.stack([G[:, 150], G[:, 0], np.full(len(xq), FLT_MAX, np.float32), np.full(len(xq), FLT_MAX, np.float32)], 1)
    same_bits(idx.compute_distance_subset(xq, ck), want)
    same_bits(idx.compute_distance_subset(torch.from_numpy(xq).cuda(), torch.from_numpy(ck).cuda()).cpu().numpy(), want)
    # rows removed below and between the duplicates: the label still answers with its last row
    assert idx.remove_ids(np.array([-5, labels[100]], dtype=np.int64)) == 2
    same_bits(idx.reconstruct(dup), xb[150])
    same_bits(idx.index.reconstruct_n(148, 1)[0], xb[150])  # (row 150 is row 148 now)
    assert idx.remove_ids(np.array([dup], dtype=np.int64)) == 2  # both rows of the label go together
    with pytest.raises(RuntimeError, match="not found"):
        idx.reconstruct(dup)


# ---- search_and_reconstruct -------------------------------------------------------
def check_sar(ix, xb, xq, k, params=None, id_offset=0):
    D, I, R = ix.search_and_reconstruct(xq, k, params=params)
    Ds, Is = ix.search(xq, k, params=params)
    same_bits(D, Ds)
    np.testing.assert_array_equal(I, Is)
    miss = I < 0
    assert R.shape == (len(xq), k, xb.shape[1])
    same_bits(R[~miss], xb[I[~miss] - id_offset])
    assert (bits(R[miss]) == 0xFFFFFFFF).all()  # NaN exactly where I == -1
    assert not np.isnan(R[~miss]).any()
    return D, I, R


@pytest.mark.parametrize("d,dtype", [(384, "float32"), (768, "bfloat16")])
@pytest.mark.parametrize("nq", [1, 129])
def test_search_and_reconstruct(fx, corpus, indexes, d, dtype, nq):
    xb, ix = corpus(d), indexes(d, dtype)
    xq = synth(11, 0, nq, d)
    for k in (1, 10, 40):
        D, I, _ = check_sar(ix, xb, xq, k)
        assert (I >= 0).all()


def test_search_and_reconstruct_padding_selector_and_huge_k(fx, torch, corpus, indexes):
    d = 384
    xb, xq = corpus(d), synth(11, 0, 129, d)
    small = fx.IndexFlatL2(d, dtype="float16")
    small.add(xb[:300])
    D, I, R = check_sar(small, xb, xq[:9], 305)  # k = ntotal + 5: five padded slots per query
    assert (I[:, 300:] == -1).all() and (I[:, :300] >= 0).all() and (D[:, 300:] == FLT_MAX).all()
    ix = indexes(d, "float32")
    params = fx.SearchParameters(sel=fx.IDSelectorRange(100, 140))
    D, I, _ = check_sar(ix, xb, xq, 40, params=params)  # exactly the selection
    assert sorted(I[0].tolist()) == list(range(100, 140))
    D, I, _ = check_sar(ix, xb, xq, 41, params=params)  # ... and one padded slot
    assert (I[:, 40] == -1).all() and (I[:, :40] >= 0).all()
    with pytest.raises(RuntimeError):  # a selector takes k <= MAX_K, as search
        ix.search_and_reconstruct(xq[:2], fx._lib.MAX_K + 1, params=params)
    big = fx.IndexFlatL2(d, dtype="bfloat16")
    big.add(xb[:2000])
    check_sar(big, xb, xq[:3], fx._lib.MAX_K + 1)  # the exact sort path, unfiltered
    # device tensors in and out, fp32 and the storage dtype
    tq = torch.from_numpy(xq).cuda()
    Dh, Ih, Rh = ix.search_and_reconstruct(xq, 10)
    Dt, It, Rt = ix.search_and_reconstruct(tq, 10)
    assert Dt.is_cuda and It.is_cuda and Rt.is_cuda and tuple(Rt.shape) == (129, 10, d)
    same_bits(Dt.cpu().numpy(), Dh)
    np.testing.assert_array_equal(It.cpu().numpy(), Ih)
    same_bits(Rt.cpu().numpy(), Rh)
    _, Ib, Rb = big.search_and_reconstruct(tq[:5].to(torch.bfloat16), 7, dtype="storage")
    assert Rb.dtype == torch.bfloat16
    assert torch.equal(raw16(torch, Rb), raw16(torch, torch.tensor(xb).to(torch.bfloat16).cuda()[Ib]))


def test_plain_search_is_untouched_afterwards(fx, corpus):
    d = 384
    xb, xq = corpus(d), synth(11, 0, 129, d)
    used, fresh = fx.IndexFlatL2(d), fx.IndexFlatL2(d)
    for ix in (used, fresh):
        ix.add(xb)
    used.search_and_reconstruct(xq, 40)
    used.search_and_reconstruct(xq[:5], 10)
    used.compute_distance_subset(xq, np.zeros((129, 3), dtype=np.int64))
    used.reconstruct_batch(np.arange(100))
    for graph in (0, 1):
        for ix in (used, fresh):
            ix.set_option("search_graph", graph)
        for q, k in ((xq[:5], 10), (xq[:5], 10), (xq, 10)):  # (the second small one replays a captured graph)
            Du, Iu = used.search(q, k)
            Df, If = fresh.search(q, k)
            same_bits(Du, Df)
            np.testing.assert_array_equal(Iu, If)
            used.search_and_reconstruct(q, k)  # in between: never recorded, never replayed


# ---- compute_distance_subset --------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float16"])
@pytest.mark.parametrize("ip", [False, True])
def test_subset_reproduces_a_padded_search(fx, torch, corpus, dtype, ip):
    d = 384
    xb, xq = corpus(d)[:30], synth(11, 0, 9, d)
    ix = (fx.IndexFlatIP if ip else fx.IndexFlatL2)(d, dtype=dtype)
    ix.add(xb)
    D, I = ix.search(xq, 40)
    assert (I[:, 30:] == -1).all() and (D[:, 30:] == (-FLT_MAX if ip else FLT_MAX)).all()
    same_bits(ix.compute_distance_subset(xq, I), D)
    got = ix.compute_distance_subset(torch.from_numpy(xq).cuda(), torch.from_numpy(I).cuda())
    same_bits(got.cpu().numpy(), D)


@pytest.mark.parametrize("d,dtype", [(384, "float32"), (768, "bfloat16"), (100, "float16")])
def test_subset_of_arbitrary_keys_is_exact(fx, corpus, indexes, d, dtype):
    xb, ix = corpus(d), indexes(d, dtype)
    xq = synth(11, 0, 129, d)
    keys = np.random.default_rng(2).integers(0, NT, size=(129, 7)).astype(np.int64)
    keys[0, 0], keys[128, 6], keys[5, 3], keys[6, 3] = 0, NT - 1, -1, NT
    G, _ = grid_dist(xq, xb)
    want = np.take_along_axis(G, np.clip(keys, 0, NT - 1), 1)
    want[5, 3] = want[6, 3] = FLT_MAX
    same_bits(ix.compute_distance_subset(xq, keys), want)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("ip", [False, True])
def test_subset_on_gaussian_data_meets_the_bar(fx, dtype, ip):
    xb, xq = gaussian_small()
    ix = (fx.IndexFlatIP if ip else fx.IndexFlatL2)(384, dtype=dtype)
    ix.add(xb)
    rows = ix.reconstruct_n(0, ix.ntotal).astype(np.float64)  # the index's own (rounded) rows
    keys = np.random.default_rng(4).integers(0, len(xb), size=(64, 16)).astype(np.int64)
    y, x = rows[keys], xq.astype(np.float64)[:, None, :]
    ref = (x * y).sum(-1) if ip else ((x - y) ** 2).sum(-1)
    got = ix.compute_distance_subset(xq, keys)
    err = np.abs(got.astype(np.float64) - ref)
    print(f"compute_distance_subset {dtype} ip={ip}: max err / bar = {(err / (RTOL * np.maximum(1, np.abs(ref)))).max():.3g}")
    assert (err <= RTOL * np.maximum(1.0, np.abs(ref))).all()

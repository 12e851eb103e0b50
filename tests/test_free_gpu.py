"""fx_index_free / fx_selector_free release everything an index acquired: four
create -> use every feature -> free cycles, each on a fresh index, must not
lower the device's free memory.

A cycle's index holds 65,536 x 128 fp32 rows (a 32 MiB code matrix) and runs
every call family that owns workspace: host- and device-output search, the
k > 1024 sort path, range_search, a filtered search, remove_ids,
reconstruct_batch, search_and_reconstruct and one fx_kmeans_step.  Cycle 1
absorbs the pools of the runtime and of torch; after that the free memory may
drop by at most 16 MiB (half the code matrix) up to cycle 4, so a leaked main
buffer or workspace shows.  A double free shows as a crash here and in the
host-sanitizer drivers (tests/test_native_asan.py, tests/test_idmap_native.py).
"""
import ctypes
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, D, CYCLES = 65_536, 128, 4
SLACK = 16 << 20


def cycle(fx, _lib, torch, xb, xq):
    ix = fx.IndexFlatL2(D)
    ix.add(xb)
    xq_dev = torch.from_numpy(xq).to("cuda:0")
    ix.search(xq, 10)        # host output
    ix.search(xq_dev, 10)    # device output
    ix.search(xq[:4], 2048)  # k > 1024: the exact sort path
    lims, _, _ = ix.range_search(xq[:16], 200.0)  # (|x - y|^2 ~ 256 +- 32: a few per cent of the rows)
    assert lims[-1] > 0
    sel = fx.IDSelectorRange(1000, 40_000)
    ix.search(xq, 10, params=fx.SearchParameters(sel=sel))
    assert ix.remove_ids(fx.IDSelectorRange(0, 1000)) == 1000
    ix.reconstruct_batch(np.arange(0, 5000, 7, dtype=np.int64))
    ix.search_and_reconstruct(xq[:32], 5)
    # one k-means step over 4,096 rows, the index's rows as the centroids
    k = ix.ntotal
    ix._bind_stream(True)
    x = torch.from_numpy(xb[:4096]).to("cuda:0")
    sums = torch.empty((k, D), dtype=torch.float64, device="cuda:0")
    counts = torch.empty((k,), dtype=torch.int64, device="cuda:0")
    obj = torch.zeros((1,), dtype=torch.float64, device="cuda:0")
    ptr = lambda a: ctypes.c_void_p(a.data_ptr())  # noqa: E731
    ix._check(ix._lib.fx_kmeans_step(ix._h, 4096, ptr(x), _lib.F32, _lib.MEM_DEVICE, None, None, ptr(sums),
                                     ptr(counts), ptr(obj), 0))
    torch.cuda.synchronize()
    assert int(counts.sum().item()) == 4096
    del sel  # the selector first, then the index
    del ix, x, sums, counts, obj, xq_dev
    gc.collect()
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def test_cycles_do_not_leak():
    import torch

    from rag_faiss_embedding_amd import _lib, faiss as fx
    if _lib.device_count() == 0:
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")
    rng = np.random.default_rng(7)
    xb = rng.standard_normal((N, D)).astype(np.float32)
    xq = rng.standard_normal((64, D)).astype(np.float32)
    free = [cycle(fx, _lib, torch, xb, xq) for _ in range(CYCLES)]
    print("free bytes after each cycle:", free, "drop cycle 1 -> 4 (MiB):", (free[0] - free[-1]) / 2**20)
    assert free[0] - free[-1] <= SLACK, f"free memory fell by {(free[0] - free[-1]) / 2**20:.1f} MiB over cycles 2-4"

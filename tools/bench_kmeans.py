#!/usr/bin/env python
"""K-means iterations on the device: 1M x 768 bfloat16 rows (seeded gaussian
blobs) clustered to k = 1024 and k = 16384, --iters Lloyd
iterations (fx_kmeans_step + fx_kmeans_finish) from given initial centroids,
after --warmup iterations.

Per k it reports the wall-clock milliseconds per iteration (a host clock
around the iterations and one synchronise) and, from HIP events the library
records around each part (fx_index_profile / fx_kmeans_profile_read), the
split into assign (the k = 1 search), key build + sort + segments, sum + fold,
and finish; the bytes of x over the sum + fold time against the 8 TB/s HBM
peak; and a same-box comparator for the update alone (key build + sort + sum +
fold), an update built on float atomics:

    torch.zeros(k, d).index_add_(0, assign, x.float()); torch.bincount(assign)

timed with events, median of --iters runs.  Prints one JSON line and writes
it to profiles/bench_kmeans.json.  Single-box numbers, not gated by any test.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import amd_fx  # noqa: E402,F401
from rag_faiss_embedding_amd import _lib  # noqa: E402
from rag_faiss_embedding_amd import faiss as fx  # noqa: E402

CORPUS_SEED = 1234
N, D, KS = 1_000_000, 768, (1024, 16384)
HBM_PEAK = 8e12


def ptr(a):
    return ctypes.c_void_p(a.data_ptr())


def event_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def run(x, k, iters, warmup, dev):
    n, d = x.shape
    rows = np.random.RandomState(CORPUS_SEED + 1).permutation(n)[:k]
    init = x[torch.from_numpy(rows).to(dev)].float()
    ix = fx.IndexFlatL2(d)
    ix.add(init)
    ix._bind_stream(True)
    lib, h = _lib.lib, ix._h
    sums = torch.empty((k, d), dtype=torch.float64, device=dev)
    counts = torch.empty(k, dtype=torch.int64, device=dev)
    obj = torch.zeros(iters + warmup, dtype=torch.float64, device=dev)
    nsplit = torch.zeros(iters + warmup, dtype=torch.int64, device=dev)
    cent = torch.empty((k, d), dtype=torch.float32, device=dev)
    assign = torch.empty(n, dtype=torch.int64, device=dev)
    dist = torch.empty(n, dtype=torch.float32, device=dev)

    def iteration(i):
        ix._check(lib.fx_kmeans_step(h, n, ptr(x), _lib.BF16, _lib.MEM_DEVICE, ptr(assign), ptr(dist), ptr(sums),
                                     ptr(counts), ptr(obj[i:]), 0))
        ix._check(lib.fx_kmeans_finish(h, ptr(sums), ptr(counts), 0, ptr(cent), ptr(nsplit[i:])))

    parts = [ctypes.c_double(0) for _ in range(4)]
    ix.profile(True)
    for i in range(warmup):
        iteration(i)
    ix._check(lib.fx_kmeans_profile_read(h, *(ctypes.byref(p) for p in parts)))  # (waits; drops the warm-up's events)
    t0 = time.perf_counter()
    for i in range(warmup, warmup + iters):
        iteration(i)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3 / iters
    ix._check(lib.fx_kmeans_profile_read(h, *(ctypes.byref(p) for p in parts)))
    ix.profile(False)
    assign_ms, sort_ms, sum_ms, finish_ms = (p.value / iters for p in parts)
    bad = ctypes.c_int64(0)
    ix._check(lib.fx_kmeans_status(h, ctypes.byref(bad)))

    # the comparator, on the last iteration's assignment
    def atomics():
        torch.zeros((k, d), dtype=torch.float32, device=dev).index_add_(0, assign, x.float())
        torch.bincount(assign, minlength=k)
    cmp_ms = event_ms(atomics, iters, warmup)
    update_ms = sort_ms + sum_ms
    events_ms = assign_ms + update_ms + finish_ms
    xbytes = n * d * x.element_size()
    return {
        "k": k, "ms_per_iter_wall": round(wall, 3), "ms_per_iter_events": round(events_ms, 3),
        "assign_ms": round(assign_ms, 3), "keys_sort_ms": round(sort_ms, 3), "sum_fold_ms": round(sum_ms, 3),
        "finish_ms": round(finish_ms, 3), "update_ms": round(update_ms, 3),
        "assign_share": round(assign_ms / events_ms, 3),
        "sum_fold_x_bytes_per_s": round(xbytes / (sum_ms * 1e-3), 0),
        "sum_fold_fraction_of_8TBps": round(xbytes / (sum_ms * 1e-3) / HBM_PEAK, 3),
        "index_add_update_ms": round(cmp_ms, 3), "update_over_index_add": round(update_ms / cmp_ms, 3),
        "obj_first": obj[warmup].item(), "obj_last": obj[warmup + iters - 1].item(),
        "nsplit_total": int(nsplit.sum().item()),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, default=N)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bench_kmeans.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_kmeans: no GPU visible (measurements need the MI355X)")
    dev = torch.device("cuda", 0)
    # clusterable rows, as embeddings are: 4,096 gaussian blob centres (sigma 2) plus noise (sigma 0.5)
    g = torch.Generator(device=dev)
    g.manual_seed(CORPUS_SEED)
    centres = torch.randn((4096, D), generator=g, device=dev) * 2
    x = torch.empty((args.rows, D), dtype=torch.bfloat16, device=dev)
    step = 1 << 17
    for r0 in range(0, args.rows, step):
        nr = min(step, args.rows - r0)
        which = torch.randint(0, 4096, (nr,), generator=g, device=dev)
        x[r0:r0 + nr] = (centres[which] + torch.randn((nr, D), generator=g, device=dev) * 0.5).to(torch.bfloat16)
    res = {"bench": "kmeans", "rows": args.rows, "d": D, "dtype": "bfloat16", "iters": args.iters,
           "warmup": args.warmup, "kmeans_chunk": fx.KMEANS_CHUNK, "device": torch.cuda.get_device_name(0),
           "runs": [run(x, k, args.iters, args.warmup, dev) for k in KS]}
    line = json.dumps(res)
    print(line)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()

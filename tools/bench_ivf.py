#!/usr/bin/env python
"""IndexIVFFlat against the flat index on one box, in one run: 1M x 768
bfloat16 rows (seeded gaussian blobs), nlist = 1024 trained with the library's
k-means, k = 10; nq in {1, 256, 10000} x nprobe in {1, 8, 32, 128}.

Per cell, event-timed after --warmup calls (median of --reps): the IVF search;
its split into coarse / pairs + query preparation / list scan / refine + exact
fallback from the HIP events the library records around each part
(fx_ivf_profile, mean of --reps further calls); recall@10 against the flat
index's result on the same rows; the flat index's search at that nq; and the
bytes the list scan must read when every probed list is read once per
128-query group, over the list scan's time, against 8 TB/s.  Also the regroup
time of the 1M rows (the first list access after the add).  Prints one JSON
line and writes it to profiles/bench_ivf.json.  Single-box numbers, not gated by any test.
"""
from __future__ import annotations

import argparse
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
from rag_faiss_embedding_amd import faiss as fx  # noqa: E402

CORPUS_SEED = 1234
N, D, NLIST, K = 1_000_000, 768, 1024, 10
NQS, NPROBES = (1, 256, 10000), (1, 8, 32, 128)
HBM_PEAK = 8e12


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, default=N)
    ap.add_argument("--nlist", type=int, default=NLIST)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bench_ivf.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ivf: no GPU visible (measurements need the MI355X)")
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(CORPUS_SEED)
    centres = torch.randn((4096, D), generator=g, device=dev) * 2
    x = torch.empty((args.rows, D), dtype=torch.bfloat16, device=dev)
    step = 1 << 17
    for r0 in range(0, args.rows, step):
        nr = min(step, args.rows - r0)
        which = torch.randint(0, 4096, (nr,), generator=g, device=dev)
        x[r0:r0 + nr] = (centres[which] + torch.randn((nr, D), generator=g, device=dev) * 0.5).to(torch.bfloat16)
    which = torch.randint(0, 4096, (max(NQS),), generator=g, device=dev)
    xq_all = (centres[which] + torch.randn((max(NQS), D), generator=g, device=dev) * 0.5).to(torch.bfloat16)

    flat = fx.IndexFlatL2(D, dtype="bfloat16")
    flat.add(x)
    ivf = fx.IndexIVFFlat(fx.IndexFlatL2(D), D, args.nlist, dtype="bfloat16")
    t0 = time.perf_counter()
    ivf.train(x)
    torch.cuda.synchronize()
    train_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    ivf.add(x)
    torch.cuda.synchronize()
    add_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    sizes = ivf.list_sizes()  # the regroup
    regroup_ms = (time.perf_counter() - t0) * 1e3
    row_bytes = D * 2

    cells = []
    for nq in NQS:
        xq = xq_all[:nq].contiguous()
        Df = torch.empty((nq, K), dtype=torch.float32, device=dev)
        If = torch.empty((nq, K), dtype=torch.int64, device=dev)
        flat_ms = event_ms(lambda: flat.search(xq, K, D=Df, I=If), args.reps, args.warmup)
        If_h = If.cpu().numpy()
        for nprobe in NPROBES:
            ivf.nprobe = nprobe
            Dv = torch.empty((nq, K), dtype=torch.float32, device=dev)
            Iv = torch.empty((nq, K), dtype=torch.int64, device=dev)
            ms = event_ms(lambda: ivf.search(xq, K, D=Dv, I=Iv), args.reps, args.warmup)
            ivf.profile(True)
            for _ in range(args.reps):
                ivf.search(xq, K, D=Dv, I=Iv)
            parts = ivf.profile_read()
            ivf.profile(False)
            parts = {key: round(parts[key] / args.reps, 4) for key in ("coarse", "pairs", "scan", "refine")}
            Ic = ivf.quantizer.search(xq, nprobe)[1]  # the probed lists, for the byte count
            Iv_h = Iv.cpu().numpy()
            recall = float(np.mean([len(set(a.tolist()) & set(b.tolist())) / K for a, b in zip(Iv_h, If_h)]))
            per_list = np.bincount(Ic.cpu().numpy().ravel(), minlength=args.nlist)
            scan_bytes = float((((per_list + 127) // 128) * sizes).sum()) * row_bytes
            scan_ms = max(parts["scan"], 1e-6)
            plan = ivf.last_ivf_plan()
            cells.append({"nq": nq, "nprobe": nprobe, "ivf_ms": round(ms, 4), "coarse_ms": parts["coarse"],
                          "pairs_prep_ms": parts["pairs"], "scan_ms": parts["scan"], "refine_ms": parts["refine"],
                          "dominant": max(parts, key=parts.get), "flat_ms": round(flat_ms, 4),
                          "flat_over_ivf": round(flat_ms / ms, 3), "recall_at_10": round(recall, 4),
                          "scan_bytes": scan_bytes,
                          "scan_fraction_of_8TBps": round(scan_bytes / (scan_ms * 1e-3) / HBM_PEAK, 4),
                          "fallbacks": ivf.last_fallbacks(), "dropped": ivf.last_dropped_candidates(), "plan": plan})
    res = {"bench": "ivf", "rows": args.rows, "d": D, "dtype": "bfloat16", "nlist": args.nlist, "k": K,
           "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
           "train_s": round(train_s, 3), "add_s": round(add_s, 3), "regroup_ms": round(regroup_ms, 3),
           "longest_list": int(sizes.max()), "empty_lists": int((sizes == 0).sum()), "cells": cells}
    line = json.dumps(res)
    print(line)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()

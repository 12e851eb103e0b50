#!/usr/bin/env python
"""IndexIVFScalarQuantizer beside its two parents on one box, in one run: the 1M x 768 seeded
gaussian blobs of tools/bench_ivf.py (bfloat16-representable values), nlist = 1024 trained once with
the library's k-means (every inverted file gets the same centroids), k = 10; nq in {1, 256, 10000} x
nprobe in {1, 8, 32, 128}.

Per cell, event-timed after --warmup calls (median of --reps): the 8-bit inverted file's search with
by_residual on and off; its split into coarse / pairs + operand preparation / list scan / refine +
exact fallback from the HIP events the library records (fx_ivfsq_profile, mean of --reps further
calls); the queries flagged; recall@10 of each against the fp32 flat index's result; IndexIVFFlat
(bfloat16) at the same nprobe with its list scan's time; and, per nq, IndexScalarQuantizer's flat
search.  Bytes per row are what each layout defines.  One expectation is recorded, not asserted: at
nq = 10000, nprobe = 8 the 8-bit inverted file's search takes less time than IndexScalarQuantizer's
flat search of the same run.  Prints one JSON line and writes it to profiles/bench_ivfsq.json.
Single-box numbers, not gated by any test.
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


def round_up(a, m):
    return (a + m - 1) // m * m


def recall(I, If):
    return float(np.mean([len(set(a.tolist()) & set(b.tolist())) / K for a, b in zip(I, If)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, default=N)
    ap.add_argument("--nlist", type=int, default=NLIST)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bench_ivfsq.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ivfsq: no GPU visible (measurements need the MI355X)")
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

    f32 = fx.IndexFlatL2(D, dtype="float32")
    f32.add(x)
    sq = fx.IndexScalarQuantizer(D)
    sq.train(x)
    sq.add(x)
    ivf = fx.IndexIVFFlat(fx.IndexFlatL2(D), D, args.nlist, dtype="bfloat16")
    t0 = time.perf_counter()
    ivf.train(x)
    torch.cuda.synchronize()
    kmeans_s = time.perf_counter() - t0
    ivf.add(x)
    cent = ivf.quantizer.reconstruct_n(0, args.nlist)
    ivfsq, build = {}, {}
    for name, by_residual in (("residual", True), ("plain", False)):
        q = fx.IndexFlatL2(D)
        q.add(cent)
        ix = fx.IndexIVFScalarQuantizer(q, D, args.nlist, fx.ScalarQuantizer.QT_8bit, fx.METRIC_L2, by_residual)
        t0 = time.perf_counter()
        ix.train(x)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        ix.add(x)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        sizes = ix.list_sizes()  # the regroup
        build[name] = {"train_s": round(t1 - t0, 3), "add_s": round(t2 - t1, 3),
                       "regroup_ms": round((time.perf_counter() - t2) * 1e3, 3)}
        ivfsq[name] = ix
    ivf.list_sizes()
    per_row = {"ivfsq8": round_up(D, 128) + 4 + 8 + 4, "ivf_bfloat16": round_up(2 * D, 128) + 4 + 8 + 4,
               "sq8": round_up(D, 128) + 4}

    cells, flat_cells = [], []
    for nq in NQS:
        xq = xq_all[:nq].contiguous()

        def outs():
            return (torch.empty((nq, K), dtype=torch.float32, device=dev),
                    torch.empty((nq, K), dtype=torch.int64, device=dev))

        Df, If = outs()
        f32.search(xq, K, D=Df, I=If)
        If_h = If.cpu().numpy()
        Ds, Is = outs()
        sq_ms = event_ms(lambda: sq.search(xq, K, D=Ds, I=Is), args.reps, args.warmup)
        flat_cells.append({"nq": nq, "sq_flat_ms": round(sq_ms, 4), "sq_flagged": sq.last_fallbacks(),
                           "sq_recall_at_10_vs_f32": round(recall(Is.cpu().numpy(), If_h), 4)})
        for nprobe in NPROBES:
            cell = {"nq": nq, "nprobe": nprobe, "sq_flat_ms": round(sq_ms, 4)}
            Dv, Iv = outs()
            ivf.nprobe = nprobe
            cell["ivf_bf16_ms"] = round(event_ms(lambda: ivf.search(xq, K, D=Dv, I=Iv), args.reps, args.warmup), 4)
            ivf.profile(True)
            for _ in range(args.reps):
                ivf.search(xq, K, D=Dv, I=Iv)
            cell["ivf_bf16_scan_ms"] = round(ivf.profile_read()["scan"] / args.reps, 4)
            ivf.profile(False)
            cell["ivf_bf16_recall_at_10_vs_f32"] = round(recall(Iv.cpu().numpy(), If_h), 4)
            for name, ix in ivfsq.items():
                ix.nprobe = nprobe
                ms = event_ms(lambda: ix.search(xq, K, D=Dv, I=Iv), args.reps, args.warmup)
                ix.profile(True)
                for _ in range(args.reps):
                    ix.search(xq, K, D=Dv, I=Iv)
                parts = ix.profile_read()
                ix.profile(False)
                parts = {key: round(parts[key] / args.reps, 4) for key in ("coarse", "pairs", "scan", "refine")}
                cell[name] = {"ms": round(ms, 4), "coarse_ms": parts["coarse"], "pairs_prep_ms": parts["pairs"],
                              "scan_ms": parts["scan"], "refine_ms": parts["refine"],
                              "dominant": max(parts, key=parts.get), "flagged": ix.last_fallbacks(),
                              "dropped": ix.last_dropped_candidates(),
                              "recall_at_10_vs_f32": round(recall(Iv.cpu().numpy(), If_h), 4),
                              "plan": ix.last_ivf_plan()}
            cells.append(cell)
    c = next(c for c in cells if c["nq"] == 10000 and c["nprobe"] == 8)
    res = {"bench": "ivfsq", "rows": args.rows, "d": D, "nlist": args.nlist, "k": K, "reps": args.reps,
           "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "kmeans_s": round(kmeans_s, 3),
           "build": build, "bytes_per_row": per_row, "longest_list": int(sizes.max()),
           "expectation_nq10000_nprobe8_faster_than_flat_sq": bool(c["residual"]["ms"] < c["sq_flat_ms"]),
           "flat": flat_cells, "cells": cells}
    line = json.dumps(res)
    print(line)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""IndexIVFPQ beside IndexIVFScalarQuantizer, IndexIVFFlat and IndexPQ on one box, in one run: the
1M x 768 seeded gaussian blobs of tools/bench_ivfsq.py (bfloat16-representable values), nlist = 1024
trained once with the library's k-means (every inverted file gets the same centroids), M = 96 (dsub =
8), k = 10; nq in {1, 256, 10000} x nprobe in {1, 8, 32, 128}.  The codebooks (IndexIVFPQ with
by_residual on and off, IndexPQ) are trained by the classes' own train on a 65,536-row sample.

Per cell, event-timed after --warmup calls (median of --reps): IndexIVFPQ's search with by_residual
on and off; its split into coarse / pairs + operand preparation / list scan / refine + exact fallback
from the HIP events the library records (fx_ivfpq_profile, mean of --reps further calls); the queries
flagged; recall@10 of each against the fp32 flat index's result; IndexIVFScalarQuantizer (8-bit,
by_residual) and IndexIVFFlat (bfloat16) at the same nprobe with their list scans' times; and, per nq,
IndexPQ's flat search.  Bytes per row are what each layout defines.  The one thing asserted is
IndexIVFPQ's footprint: the device bytes taken while it was built stay within its rows (roundup(M, 16)
code bytes, n_y, label and list number each, the last tile's remainder and one whole tile past it),
its codebooks, the coarse centroids and the bounded workspace of an add (one chunk of fp32 residuals,
at most 256 MiB, the chunk's assignments and the regroup's sort keys); the coarse quantizer's own
search workspace, which the caller's flat index keeps, is sized before the window opens and reported
beside it.  One expectation is recorded,
not asserted: at nq = 10000, nprobe = 8 the search takes less time than IndexPQ's flat search of the
same run.  Prints one JSON line and writes it to profiles/bench_ivfpq.json.  Single-box numbers, not
gated by any test.
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
N, D, NLIST, K, M = 1_000_000, 768, 1024, 10, 96
NQS, NPROBES = (1, 256, 10000), (1, 8, 32, 128)
TRAIN_ROWS = 65536
RESID_CHUNK = 256 << 20   # the add's residual chunk (fx_api_ivfpq.cpp)
ALLOC_SLACK = 64 << 20    # the chunk's assignments (12 B a row), the regroup's sort keys and temporaries (~24 B a
                          # row) and the allocator's granularity over a dozen allocations


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


def note(msg):
    print(f"bench_ivfpq: {msg}", file=sys.stderr, flush=True)


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
    ap.add_argument("--niter", type=int, default=10)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bench_ivfpq.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ivfpq: no GPU visible (measurements need the MI355X)")
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
    sample = x[:min(TRAIN_ROWS, args.rows)].contiguous()

    f32 = fx.IndexFlatL2(D, dtype="float32")
    f32.add(x)
    ivf = fx.IndexIVFFlat(fx.IndexFlatL2(D), D, args.nlist, dtype="bfloat16")
    t0 = time.perf_counter()
    ivf.train(x)
    torch.cuda.synchronize()
    kmeans_s = time.perf_counter() - t0
    ivf.add(x)
    ivf.list_sizes()
    cent = ivf.quantizer.reconstruct_n(0, args.nlist)
    note(f"coarse k-means {kmeans_s:.2f} s")

    def quantizer():
        q = fx.IndexFlatL2(D)
        q.add(cent)
        return q

    ivfsq = fx.IndexIVFScalarQuantizer(quantizer(), D, args.nlist, fx.ScalarQuantizer.QT_8bit, fx.METRIC_L2, True)
    ivfsq.train(x)
    ivfsq.add(x)
    ivfsq.list_sizes()
    pq = fx.IndexPQ(D, M, niter=args.niter)
    pq.train(sample)
    pq.add(x)
    note("siblings built")

    ivfpq, build, dev_bytes, quant_ws = {}, {}, {}, {}
    for name, by_residual in (("residual", True), ("plain", False)):
        # the codebook, trained apart from the footprint measurement (k-means takes workspace of its own)
        trainer = fx.IndexIVFPQ(quantizer(), D, args.nlist, M, 8, fx.METRIC_L2, by_residual, pq_niter=args.niter)
        t0 = time.perf_counter()
        trainer.train(sample)
        torch.cuda.synchronize()
        train_s = time.perf_counter() - t0
        cents = trainer.pq.centroids
        del trainer
        torch.cuda.empty_cache()
        # the quantizer is the caller's flat index and its search workspace its own: one k = 1 search of a
        # full add chunk sizes it before the window opens, so the window holds what the IVFPQ index takes
        q = quantizer()
        torch.cuda.synchronize()
        free_q = torch.cuda.mem_get_info()[0]
        q.search(x[:fx.KMEANS_CHUNK], 1)
        torch.cuda.synchronize()
        quant_ws[name] = free_q - torch.cuda.mem_get_info()[0]
        free0 = torch.cuda.mem_get_info()[0]
        ix = fx.IndexIVFPQ(q, D, args.nlist, M, 8, fx.METRIC_L2, by_residual)
        ix.pq.centroids = cents
        t1 = time.perf_counter()
        ix.add(x)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        sizes = ix.list_sizes()  # the regroup
        t3 = time.perf_counter()
        torch.cuda.synchronize()
        dev_bytes[name] = free0 - torch.cuda.mem_get_info()[0]
        build[name] = {"train_s": round(train_s, 3), "add_s": round(t2 - t1, 3), "regroup_ms": round((t3 - t2) * 1e3, 3)}
        ivfpq[name] = ix
        note(f"ivfpq {name}: {build[name]}, {dev_bytes[name]} device bytes")
    per_row = {"ivfpq": round_up(M, 16) + 4 + 8 + 4, "ivfsq8": round_up(D, 128) + 4 + 8 + 4,
               "ivf_bfloat16": round_up(2 * D, 128) + 4 + 8 + 4, "pq": round_up(M, 16) + 4}
    dsub = D // M
    codebooks = M * 256 * dsub * 4 + 2 * (M * 256 * dsub + 8) * 2
    centroid_bytes = 2 * args.nlist * D * 4  # the quantizer's rows and the index's fp32 copy
    bound = ((round_up(args.rows, 128) + 128) * per_row["ivfpq"] + codebooks + centroid_bytes + RESID_CHUNK +
             ALLOC_SLACK)
    for name, b in dev_bytes.items():
        assert b <= bound, (name, b, bound)

    cells, flat_cells = [], []
    for nq in NQS:
        xq = xq_all[:nq].contiguous()

        def outs():
            return (torch.empty((nq, K), dtype=torch.float32, device=dev),
                    torch.empty((nq, K), dtype=torch.int64, device=dev))

        Df, If = outs()
        f32.search(xq, K, D=Df, I=If)
        If_h = If.cpu().numpy()
        Dp, Ip = outs()
        pq_ms = event_ms(lambda: pq.search(xq, K, D=Dp, I=Ip), args.reps, args.warmup)
        flat_cells.append({"nq": nq, "pq_flat_ms": round(pq_ms, 4), "pq_flagged": pq.last_fallbacks(),
                           "pq_recall_at_10_vs_f32": round(recall(Ip.cpu().numpy(), If_h), 4)})
        for nprobe in NPROBES:
            cell = {"nq": nq, "nprobe": nprobe, "pq_flat_ms": round(pq_ms, 4)}
            Dv, Iv = outs()
            for key, sib in (("ivf_bf16", ivf), ("ivfsq8", ivfsq)):
                sib.nprobe = nprobe
                cell[key + "_ms"] = round(event_ms(lambda: sib.search(xq, K, D=Dv, I=Iv), args.reps, args.warmup), 4)
                sib.profile(True)
                for _ in range(args.reps):
                    sib.search(xq, K, D=Dv, I=Iv)
                cell[key + "_scan_ms"] = round(sib.profile_read()["scan"] / args.reps, 4)
                sib.profile(False)
                cell[key + "_recall_at_10_vs_f32"] = round(recall(Iv.cpu().numpy(), If_h), 4)
            for name, ix in ivfpq.items():
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
            note(f"nq={nq} nprobe={nprobe}: {cell}")
    c = next(c for c in cells if c["nq"] == 10000 and c["nprobe"] == 8)
    res = {"bench": "ivfpq", "rows": args.rows, "d": D, "nlist": args.nlist, "M": M, "k": K, "reps": args.reps,
           "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "kmeans_s": round(kmeans_s, 3),
           "train_rows": int(sample.shape[0]), "niter": args.niter, "build": build, "bytes_per_row": per_row,
           "codebook_bytes": codebooks, "device_bytes": dev_bytes, "device_bytes_bound": bound,
           "quantizer_search_workspace_bytes": quant_ws,
           "longest_list": int(sizes.max()),
           "expectation_nq10000_nprobe8_faster_than_flat_pq": bool(c["residual"]["ms"] < c["pq_flat_ms"]),
           "flat": flat_cells, "cells": cells}
    line = json.dumps(res)
    print(line)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()

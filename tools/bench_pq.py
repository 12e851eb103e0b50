#!/usr/bin/env python
"""IndexPQ beside IndexScalarQuantizer and the bfloat16 flat index on one box, in
one run: the 1M x 768 blobs of tools/bench_sq.py (every index gets the same
bfloat16-representable values), M = 96 (dsub = 8), k = 10, nq in {1, 16, 256,
10000}.  The codebook is trained by IndexPQ.train on a 65,536-row sample.

Per cell, event-timed after --warmup calls (median of --reps): each index's
search; the PQ search's split into query preparation / scan / refine + exact
fallback from the HIP events the library records (fx_pq_profile, mean of --reps
further calls); the bytes the scan GATHERS from the codebook image through
LDS-DMA (two bf16 planes of roundup(d, 32) values per row and query tile) over
the scan's time, beside the code bytes it reads from HBM; the queries flagged;
and recall@10 of each result against the fp32 flat result (the quantisation's
own loss, for information).  Also the device bytes each index took while it was
built.  The one thing asserted is PQ's footprint: roundup(M, 16) + 4 bytes per
row of the rows, the last tile's remainder and one whole tile past it, plus the
codebooks (fp32 and the two bf16 planes) and the allocator's granularity.
Nothing is asserted about time.  Prints one JSON line and writes it to
profiles/bench_pq.json.  Single-box numbers, not gated by any test.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import amd_fx  # noqa: E402,F401
from rag_faiss_embedding_amd import faiss as fx  # noqa: E402

CORPUS_SEED = 1234
N, D, K, M = 1_000_000, 768, 10, 96
NQS = (1, 16, 256, 10000)
TRAIN_ROWS = 65536
ALLOC_SLACK = 8 << 20  # four allocations (codes, n_y, centroids, image) rounded up by the allocator


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
    print(f"bench_pq: {msg}", file=sys.stderr, flush=True)


def round_up(a, m):
    return (a + m - 1) // m * m


def built(make):
    """(index, device bytes taken while it was built)."""
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    ix = make()
    torch.cuda.synchronize()
    return ix, free0 - torch.cuda.mem_get_info()[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, default=N)
    ap.add_argument("--niter", type=int, default=10)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bench_pq.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pq: no GPU visible (measurements need the MI355X)")
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

    # the codebook, trained apart from the footprint measurement (k-means takes workspace of its own)
    t0 = torch.cuda.Event(enable_timing=True)
    t1 = torch.cuda.Event(enable_timing=True)
    trainer = fx.IndexPQ(D, M, niter=args.niter)
    t0.record()
    trainer.train(x[:min(TRAIN_ROWS, args.rows)].contiguous())
    t1.record()
    t1.synchronize()
    train_ms = t0.elapsed_time(t1)
    cents = trainer.pq.centroids
    note(f"trained in {train_ms:.0f} ms")
    del trainer
    torch.cuda.empty_cache()

    def make_pq():
        ix = fx.IndexPQ(D, M)
        ix.pq.centroids = cents
        ix.add(x)
        return ix

    def make_sq():
        ix = fx.IndexScalarQuantizer(D)
        ix.train(x)
        ix.add(x)
        return ix

    def make_flat(dtype):
        ix = fx.IndexFlatL2(D, dtype=dtype)
        ix.add(x)
        return ix

    a0, a1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a0.record()
    pq, pq_bytes = built(make_pq)
    a1.record()
    a1.synchronize()
    add_ms = a0.elapsed_time(a1)
    sq, sq_bytes = built(make_sq)
    bf, bf_bytes = built(lambda: make_flat("bfloat16"))
    f32, f32_bytes = built(lambda: make_flat("float32"))
    note(f"indexes built (pq add {add_ms:.0f} ms)")
    dsub, kp = D // M, round_up(D, 32)
    per_row = {"pq": round_up(M, 16) + 4, "sq8": round_up(D, 128) + 4, "bfloat16": round_up(2 * D, 128) + 4,
               "float32": round_up(4 * D, 128) + 4}
    codebooks = M * 256 * dsub * 4 + 2 * (M * 256 * dsub + 8) * 2
    # the footprint
    bound = (round_up(args.rows, 128) + 128) * per_row["pq"] + codebooks + ALLOC_SLACK
    assert pq_bytes <= bound, (pq_bytes, bound)

    cells = []
    for nq in NQS:
        xq = xq_all[:nq].contiguous()
        out = {name: (torch.empty((nq, K), dtype=torch.float32, device=dev),
                      torch.empty((nq, K), dtype=torch.int64, device=dev)) for name in ("pq", "sq", "bf", "f32")}
        f32_ms = event_ms(lambda: f32.search(xq, K, D=out["f32"][0], I=out["f32"][1]), args.reps, args.warmup)
        bf_ms = event_ms(lambda: bf.search(xq, K, D=out["bf"][0], I=out["bf"][1]), args.reps, args.warmup)
        sq_ms = event_ms(lambda: sq.search(xq, K, D=out["sq"][0], I=out["sq"][1]), args.reps, args.warmup)
        pq_ms = event_ms(lambda: pq.search(xq, K, D=out["pq"][0], I=out["pq"][1]), args.reps, args.warmup)
        pq.profile(True)
        for _ in range(args.reps):
            pq.search(xq, K, D=out["pq"][0], I=out["pq"][1])
        parts = pq.profile_read()
        pq.profile(False)
        parts = {key: round(parts[key] / args.reps, 4) for key in ("prep", "scan", "refine")}
        plan = pq.last_pq_plan()
        If = out["f32"][1].cpu().numpy()

        def recall(name):
            Ix = out[name][1].cpu().numpy()
            return round(float(np.mean([len(set(a.tolist()) & set(b.tolist())) / K for a, b in zip(Ix, If)])), 4)

        qtiles = (nq + 127) // 128
        gathered = float(args.rows) * 2 * kp * 2 * qtiles
        scan_s = max(parts["scan"], 1e-6) * 1e-3
        cells.append({"nq": nq, "pq_ms": round(pq_ms, 4), "sq_ms": round(sq_ms, 4), "bf16_flat_ms": round(bf_ms, 4),
                      "f32_flat_ms": round(f32_ms, 4), "prep_ms": parts["prep"], "scan_ms": parts["scan"],
                      "refine_ms": parts["refine"], "dominant": max(parts, key=parts.get),
                      "gathered_bytes": gathered, "gathered_TBps": round(gathered / scan_s / 1e12, 4),
                      "code_bytes": float(args.rows) * round_up(M, 16) * qtiles,
                      "flagged": pq.last_fallbacks(), "dropped": pq.last_dropped_candidates(),
                      "recall_at_10_vs_f32": {"pq": recall("pq"), "sq8": recall("sq"), "bf16": recall("bf")},
                      "plan": plan})
        note(f"nq={nq}: {cells[-1]}")
    res = {"bench": "pq", "rows": args.rows, "d": D, "M": M, "k": K, "reps": args.reps, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0), "train_rows": min(TRAIN_ROWS, args.rows), "niter": args.niter,
           "train_ms": round(train_ms, 1), "add_ms": round(add_ms, 1), "bytes_per_row": per_row,
           "codebook_bytes": codebooks,
           "device_bytes": {"pq": pq_bytes, "sq8": sq_bytes, "bfloat16": bf_bytes, "float32": f32_bytes}, "cells": cells}
    line = json.dumps(res)
    print(line)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()

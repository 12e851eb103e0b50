#!/usr/bin/env python
"""IndexScalarQuantizer against the flat index on one box, in one run: 1M x 768
rows (seeded gaussian blobs, as tools/bench_ivf.py draws them; every index gets
the same bfloat16-representable values), k = 10, nq in {1, 16, 256, 10000}; the
8-bit index, a bfloat16 flat index and an fp32 flat index.

Per cell, event-timed after --warmup calls (median of --reps): each index's
search; the 8-bit search's split into query preparation / scan / refine + exact
fallback from the HIP events the library records (fx_sq_profile, mean of --reps
further calls); the bytes the scan must read when every query tile streams the
codes once, over the scan's time, against 8 TB/s; the queries flagged; and
recall@10 of the quantised result against the fp32 flat result (the
quantisation's own loss, for information).  Also the device bytes each index
took while it was built (hipMemGetInfo around the build) beside the bytes per
row its layout defines; the one thing asserted is that footprint: roundup(d,
128) + 4 bytes per row against roundup(2 d, 128) + 4.  Prints one JSON line and
writes it to profiles/bench_sq.json.  Single-box numbers, not gated by any test.
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
N, D, K = 1_000_000, 768, 10
NQS = (1, 16, 256, 10000)
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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bench_sq.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sq: no GPU visible (measurements need the MI355X)")
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

    def make_sq():
        ix = fx.IndexScalarQuantizer(D)
        ix.train(x)
        ix.add(x)
        return ix

    def make_flat(dtype):
        ix = fx.IndexFlatL2(D, dtype=dtype)
        ix.add(x)
        return ix

    sq, sq_bytes = built(make_sq)
    bf, bf_bytes = built(lambda: make_flat("bfloat16"))
    f32, f32_bytes = built(lambda: make_flat("float32"))
    per_row = {"sq8": round_up(D, 128) + 4, "bfloat16": round_up(2 * D, 128) + 4, "float32": round_up(4 * D, 128) + 4}
    assert per_row["sq8"] == sq.code_size + (-sq.code_size) % 128 + 4
    # the footprint: the codes and the row constants of the rows and of the tile(s) past them, to the
    # allocator's granularity; half the bfloat16 layout's
    assert sq_bytes <= (args.rows + 256) * per_row["sq8"] + (64 << 20), (sq_bytes, per_row)
    assert 2 * per_row["sq8"] <= per_row["bfloat16"] + 4

    cells = []
    for nq in NQS:
        xq = xq_all[:nq].contiguous()
        out = {name: (torch.empty((nq, K), dtype=torch.float32, device=dev),
                      torch.empty((nq, K), dtype=torch.int64, device=dev)) for name in ("sq", "bf", "f32")}
        f32_ms = event_ms(lambda: f32.search(xq, K, D=out["f32"][0], I=out["f32"][1]), args.reps, args.warmup)
        bf_ms = event_ms(lambda: bf.search(xq, K, D=out["bf"][0], I=out["bf"][1]), args.reps, args.warmup)
        sq_ms = event_ms(lambda: sq.search(xq, K, D=out["sq"][0], I=out["sq"][1]), args.reps, args.warmup)
        sq.profile(True)
        for _ in range(args.reps):
            sq.search(xq, K, D=out["sq"][0], I=out["sq"][1])
        parts = sq.profile_read()
        sq.profile(False)
        parts = {key: round(parts[key] / args.reps, 4) for key in ("prep", "scan", "refine")}
        plan = sq.last_sq_plan()
        Is, If = out["sq"][1].cpu().numpy(), out["f32"][1].cpu().numpy()
        recall = float(np.mean([len(set(a.tolist()) & set(b.tolist())) / K for a, b in zip(Is, If)]))
        scan_bytes = float(args.rows) * round_up(D, 128) * ((nq + 127) // 128)
        cells.append({"nq": nq, "sq_ms": round(sq_ms, 4), "bf16_flat_ms": round(bf_ms, 4),
                      "f32_flat_ms": round(f32_ms, 4), "bf16_over_sq": round(bf_ms / sq_ms, 3),
                      "prep_ms": parts["prep"], "scan_ms": parts["scan"], "refine_ms": parts["refine"],
                      "dominant": max(parts, key=parts.get), "scan_bytes": scan_bytes,
                      "scan_fraction_of_8TBps": round(scan_bytes / (max(parts["scan"], 1e-6) * 1e-3) / HBM_PEAK, 4),
                      "flagged": sq.last_fallbacks(), "dropped": sq.last_dropped_candidates(),
                      "recall_at_10_vs_f32": round(recall, 4), "plan": plan})
    res = {"bench": "sq", "rows": args.rows, "d": D, "k": K, "reps": args.reps, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0), "bytes_per_row": per_row,
           "device_bytes": {"sq8": sq_bytes, "bfloat16": bf_bytes, "float32": f32_bytes}, "cells": cells}
    line = json.dumps(res)
    print(line)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()

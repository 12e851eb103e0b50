#!/usr/bin/env python
"""range_search on BASELINE config (b) against the k-NN calls that could
stand in for it.

Workload: config (b)'s index (1M x 384 fp32, the synthetic corpus of bench.py)
and query batch (1,000 device-resident queries).  The radius is the median of
search(k=10)'s 10th distance, i.e. about 10 hits per query.  Reported per
call (median of --calls after --warmup, wall clock around a synchronised
call): range_search; search(k=10), for information; search(k=2048), the only
way to answer a radius query without range_search (host filter of a large
k).  Also the hits, the pairs the MFMA scan emitted, and the scan passes.

Prints one JSON line; "gate" is range_search faster than search(k=2048).
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

import torch  # noqa: E402

import amd_fx  # noqa: E402,F401
from rag_faiss_embedding_amd import faiss as fx  # noqa: E402

CORPUS_SEED, QUERY_SEED = 1234, 4321  # bench.py's
ROWS, DIM, DTYPE, NQ = 1_000_000, 384, "float32", 1_000  # BASELINE config (b)


def timed(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=ROWS)
    ap.add_argument("--nq", type=int, default=NQ)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--big-k", type=int, default=2048)
    args = ap.parse_args()

    dev = torch.device("cuda", 0)
    ix = fx.IndexFlatL2(DIM, dtype=DTYPE)
    ix.reserve(args.rows)
    chunk = 1 << 20
    buf = torch.empty((min(chunk, args.rows), DIM), dtype=torch.float32, device=dev)
    for r0 in range(0, args.rows, chunk):
        part = buf[: min(chunk, args.rows - r0)]
        fx.synth_fill(part, r0, CORPUS_SEED)
        ix.add(part)
    xq = torch.empty((args.nq, DIM), dtype=torch.float32, device=dev)
    fx.synth_fill(xq, 0, QUERY_SEED)
    torch.cuda.synchronize()

    D10, _ = ix.search(xq, 10)
    radius = float(D10[:, 9].median())

    lims, D, I = ix.range_search(xq, radius)
    stats = ix.last_range_stats()
    hits = int(lims[-1])
    # the same answer from the large-k call: every hit is within the top big-k
    Dk, Ik = ix.search(xq, args.big_k)
    per_q = (lims[1:] - lims[:-1])
    assert int(per_q.max()) <= args.big_k
    assert int((Dk < radius).sum()) == hits, (int((Dk < radius).sum()), hits)

    t_range = timed(lambda: ix.range_search(xq, radius), args.calls, args.warmup)
    t_k10 = timed(lambda: ix.search(xq, 10), args.calls, args.warmup)
    t_big = timed(lambda: ix.search(xq, args.big_k), args.calls, args.warmup)
    out = {
        "bench": "range_search", "config": "b", "rows": args.rows, "dim": DIM, "dtype": DTYPE, "nq": args.nq,
        "radius": radius, "hits": hits, "hits_per_query": hits / args.nq, "max_hits_per_query": int(per_q.max()),
        "scan_candidates": stats["candidates"], "candidates_per_hit": stats["candidates"] / max(hits, 1),
        "passes": stats["passes"], "calls": args.calls, "warmup": args.warmup,
        "range_search_ms": round(t_range[0], 4), "range_search_ms_min_max": [round(t_range[1], 4), round(t_range[2], 4)],
        "search_k10_ms": round(t_k10[0], 4),
        f"search_k{args.big_k}_ms": round(t_big[0], 4),
        "speedup_vs_big_k": round(t_big[0] / t_range[0], 2),
        "gate": bool(t_range[0] < t_big[0]),
        "device": torch.cuda.get_device_name(0),
    }
    print(json.dumps(out))
    return 0 if out["gate"] else 1


if __name__ == "__main__":
    sys.exit(main())

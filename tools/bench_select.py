#!/usr/bin/env python
"""Filtered search (search(x, k, params=SearchParameters(sel=...))) against
the unfiltered search of the same index.

Indexes: BASELINE config (b) as tools/bench_range.py builds it (1M x 384 fp32,
the synthetic corpus of bench.py) and a bfloat16 768-wide corpus of the same
row count.  For nq = 1000 and nq = 1 device-resident queries, k = 10, the
median wall clock of a synchronised call (--calls after --warmup) of:

  unfiltered       search(x, k): the index's normal scan (k_scan_v4 on the
                   split-fp32 image / k_scan_v5 on the centred bf16 rows)
  all              every row selected: the price of the generic filtered kernel
  random_10pct     a random 10 % of the rows (every tile stays live)
  random_1pct      a random 1 % (nearly every tile stays live: ~1.3 rows each)
  contiguous_1pct  rows [n/2, n/2 + n/100): ~1 % of the tiles live

with each selection's selected rows and live tiles.  Prints one JSON line.
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
ROWS, K = 1_000_000, 10
INDEXES = [("b_f32_384", 384, "float32"), ("bf16_768", 768, "bfloat16")]


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
    return round(statistics.median(ms), 4)


def build(rows, dim, dtype, dev):
    ix = fx.IndexFlatL2(dim, dtype=dtype)
    ix.reserve(rows)
    chunk = 1 << 19
    buf = torch.empty((min(chunk, rows), dim), dtype=torch.float32, device=dev)
    for r0 in range(0, rows, chunk):
        part = buf[: min(chunk, rows - r0)]
        fx.synth_fill(part, r0, CORPUS_SEED)
        ix.add(part)
    return ix


def selections(rows, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    perm = torch.randperm(rows, device=dev, generator=g)
    lo = rows // 2
    return [
        ("all", fx.IDSelectorRange(0, rows)),
        ("random_10pct", fx.IDSelectorBatch(perm[: rows // 10].contiguous())),
        ("random_1pct", fx.IDSelectorBatch(perm[: rows // 100].contiguous())),
        ("contiguous_1pct", fx.IDSelectorRange(lo, lo + rows // 100)),
    ]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=ROWS)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = {"bench": "filtered_search", "rows": args.rows, "k": K, "calls": args.calls, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0), "indexes": {}}
    for name, dim, dtype in INDEXES:
        ix = build(args.rows, dim, dtype, dev)
        sels = selections(args.rows, dev)
        res = {"dim": dim, "dtype": dtype, "selections": {n: s.stats(ix) for n, s in sels}}
        for nq in (1000, 1):
            xq = torch.empty((nq, dim), dtype=torch.float32, device=dev)
            fx.synth_fill(xq, 0, QUERY_SEED)
            torch.cuda.synchronize()
            r = {"unfiltered_ms": timed(lambda: ix.search(xq, K), args.calls, args.warmup)}
            r["unfiltered_plan"] = ix.last_scan_plan()
            for n, s in sels:
                p = fx.SearchParameters(sel=s)
                r[n + "_ms"] = timed(lambda: ix.search(xq, K, params=p), args.calls, args.warmup)
                r[n + "_fallbacks"] = ix.last_fallbacks()
            r["filtered_plan"] = ix.last_scan_plan()
            r["all_vs_unfiltered"] = round(r["all_ms"] / r["unfiltered_ms"], 3)
            r["contiguous_1pct_vs_all"] = round(r["contiguous_1pct_ms"] / r["all_ms"], 4)
            res[f"nq{nq}"] = r
        out["indexes"][name] = res
        del ix, sels
        torch.cuda.empty_cache()
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python
"""Stored vectors by key: reconstruct_batch, search_and_reconstruct and
compute_distance_subset on a 1M x 384 fp32 and a 1M x 768 bfloat16 index (the
synthetic corpus of bench.py), device tensors in and out, median wall clock of
a synchronised call (--calls after --warmup):

  reconstruct_batch   100,000 uniform-random keys and 100,000 contiguous keys,
                      fp32 out (and the storage dtype on the 16-bit index).
                      Yardsticks: a torch device-to-device copy moving the same
                      bytes (read + written: the stored rows' bytes without their
                      padding plus the output's) -- the ceiling -- and
                      reconstruct_n(0, 100000) to the host, the only read-back
                      before this call existed
  search_and_reconstruct   nq = 1000, k = 10 against search alone
  compute_distance_subset  1000 x 100 keys (no yardstick)

Prints one JSON line and writes it to profiles/bench_reconstruct.json.
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

import torch  # noqa: E402

import amd_fx  # noqa: E402,F401
from rag_faiss_embedding_amd import faiss as fx  # noqa: E402

CORPUS_SEED, QUERY_SEED = 1234, 4321  # bench.py's
INDEXES = [("f32_384_1m", 1_000_000, 384, "float32"), ("bf16_768_1m", 1_000_000, 768, "bfloat16")]
N_KEYS, NQ, K, SUBSET = 100_000, 1000, 10, 100


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
    return statistics.median(ms)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="", help="run one index by name")
    ap.add_argument("--rows", type=int, default=0, help="override the row counts (testing)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bench_reconstruct.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = {"bench": "reconstruct", "calls": args.calls, "warmup": args.warmup, "keys": N_KEYS,
           "device": torch.cuda.get_device_name(0), "indexes": {}}
    for name, rows, dim, dtype in INDEXES:
        if args.only and name != args.only:
            continue
        rows = args.rows or rows
        nkeys = min(N_KEYS, rows)
        ix = build(rows, dim, dtype, dev)
        g = torch.Generator(device=dev)
        g.manual_seed(7)
        key_sets = {"random": torch.randint(0, rows, (nkeys,), device=dev, generator=g),
                    "contiguous": torch.arange(nkeys, device=dev)}
        es = 4 if dtype == "float32" else 2
        res = {"rows": rows, "dim": dim, "dtype": dtype}
        outs = ["float32"] + (["storage"] if dtype != "float32" else [])
        for od in outs:
            oes = 4 if od == "float32" else es
            moved = nkeys * dim * (es + oes)  # bytes read (without row padding) + bytes written
            src = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
            dst = torch.empty_like(src)
            copy_ms = timed(lambda: dst.copy_(src), args.calls, args.warmup)
            copy_gbs = moved / copy_ms / 1e6
            for kname, keys in key_sets.items():
                ms = timed(lambda: ix.reconstruct_batch(keys, dtype=od), args.calls, args.warmup)
                gbs = moved / ms / 1e6
                res[f"reconstruct_batch_{kname}_{od}"] = {
                    "ms": round(ms, 4), "gb_s": round(gbs, 1), "copy_ms": round(copy_ms, 4),
                    "copy_gb_s": round(copy_gbs, 1), "fraction_of_copy": round(gbs / copy_gbs, 4)}
            del src, dst
        # the only read-back before: contiguous rows to the host (blocking)
        n_ms = timed(lambda: ix.reconstruct_n(0, nkeys), max(3, args.calls // 4), 1)
        res["reconstruct_n_host"] = {"ms": round(n_ms, 3),
                                     "over_batch_contiguous": round(
                                         n_ms / res["reconstruct_batch_contiguous_float32"]["ms"], 1)}
        xq = torch.empty((NQ, dim), dtype=torch.float32, device=dev)
        fx.synth_fill(xq, 0, QUERY_SEED)
        torch.cuda.synchronize()
        s_ms = timed(lambda: ix.search(xq, K), args.calls, args.warmup)
        r_ms = timed(lambda: ix.search_and_reconstruct(xq, K), args.calls, args.warmup)
        res["search_and_reconstruct_nq1000_k10"] = {"ms": round(r_ms, 4), "search_ms": round(s_ms, 4),
                                                    "ratio": round(r_ms / s_ms, 4)}
        sub = torch.randint(0, rows, (NQ, SUBSET), device=dev, generator=g)
        c_ms = timed(lambda: ix.compute_distance_subset(xq, sub), args.calls, args.warmup)
        res["compute_distance_subset_1000x100"] = {"ms": round(c_ms, 4),
                                                   "pairs_per_us": round(NQ * SUBSET / c_ms / 1e3, 2)}
        out["indexes"][name] = res
        del ix
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if not args.only and not args.rows:
        Path(args.out).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

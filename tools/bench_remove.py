#!/usr/bin/env python
"""remove_ids (the in-place compaction, fx_remove.hip) against today's
alternative: the kept rows in a second device tensor, reset(), add().

Indexes: BASELINE config (b) (1M x 384 fp32) and one GPU's share of config (d)
(1.25M x 768 bfloat16), the synthetic corpus of bench.py.  Patterns:

  scattered_1pct   a random 1 % of the rows
  scattered_10pct  a random 10 %
  block_1pct       rows [n/100, 2n/100): one contiguous block near the start
  last_1pct        the last n/100 rows (nothing moves)

Every timed call runs on a freshly built index (a removal is destructive) that
has seen one removal of the same ids and an add of as many rows, so that its
staging and prefix buffers exist (remove_cold_ms: one call without that); the
median wall clock of --calls synchronised calls after --warmup is reported,
the selector built from device-resident ids inside the timed call.  Per
pattern: remove_ms; the plan (first removed row, rows moved in place and
through staging, chunks); bytes_moved counted from the plan (a row and its
norm: read + written once when moved in place, twice when staged);
hbm_fraction = bytes_moved / remove_ms / 8 TB/s; reset_add_ms, the same rows
put back by reset() + add() of a device tensor that already holds the kept
rows (building that tensor is not timed); and their ratio.  Prints one JSON
line.
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

CORPUS_SEED = 1234  # bench.py's
HBM_BYTES_PER_S = 8e12
INDEXES = [("b_f32_384", 1_000_000, 384, "float32"), ("d_bf16_768", 1_250_000, 768, "bfloat16")]
TORCH_DT = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}


def corpus(rows, dim, dtype, dev):
    """The synthetic rows as one device tensor in the index's storage dtype."""
    x = torch.empty((rows, dim), dtype=TORCH_DT[dtype], device=dev)
    chunk = 1 << 19
    for r0 in range(0, rows, chunk):
        fx.synth_fill(x[r0:min(rows, r0 + chunk)], r0, CORPUS_SEED)
    return x


def build(x, dtype):
    ix = fx.IndexFlatL2(x.shape[1], dtype=dtype)
    ix.reserve(x.shape[0])
    ix.add(x)
    return ix


def patterns(rows, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    perm = torch.randperm(rows, device=dev, generator=g)
    pct = rows // 100
    return [
        ("scattered_1pct", perm[:pct].contiguous()),
        ("scattered_10pct", perm[:10 * pct].contiguous()),
        ("block_1pct", torch.arange(pct, 2 * pct, device=dev)),
        ("last_1pct", torch.arange(rows - pct, rows, device=dev)),
    ]


def median_ms(setup, fn, calls, warmup):
    ms = []
    for i in range(warmup + calls):
        state = setup()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(state)
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ms), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rows-scale", type=float, default=1.0, help="scale both indexes' row counts")
    ap.add_argument("--remove-stage", type=int, default=0, help="the index option remove_stage (bytes; 0: default)")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = {"bench": "remove_ids", "calls": args.calls, "warmup": args.warmup, "remove_stage": args.remove_stage,
           "device": torch.cuda.get_device_name(0), "indexes": {}}
    for name, rows, dim, dtype in INDEXES:
        rows = max(1000, int(rows * args.rows_scale))
        x = corpus(rows, dim, dtype, dev)
        row_bytes = (dim * x.element_size() + 127) // 128 * 128
        res = {"rows": rows, "dim": dim, "dtype": dtype, "row_bytes": row_bytes, "patterns": {}}
        for pname, ids in patterns(rows, dev):
            def fresh():
                ix = build(x, dtype)
                if args.remove_stage:
                    ix.set_option("remove_stage", args.remove_stage)
                return ix

            last = {}

            def remove(ix):
                last["n"] = ix.remove_ids(ids)
                last["stats"] = ix.last_remove_stats()
                last["ntotal"] = ix.ntotal

            def warm():
                # one removal and an add of as many rows first: the timed call finds its buffers allocated
                ix = fresh()
                ix.remove_ids(ids)
                ix.add(x[:ids.numel()])
                return ix

            r = {"remove_cold_ms": median_ms(fresh, remove, 1, 0),
                 "remove_ms": median_ms(warm, remove, args.calls, args.warmup)}
            st = last["stats"]
            r.update(removed=last["n"], **st)
            moved = (2 * st["direct_rows"] + 4 * st["staged_rows"]) * (row_bytes + 4)
            r["bytes_moved"] = moved
            r["bytes_above_first"] = (rows - st["first"]) * (row_bytes + 4)
            r["hbm_fraction"] = round(moved / (r["remove_ms"] * 1e-3) / HBM_BYTES_PER_S, 4)
            # today's route: the kept rows already in a second device tensor, reset(), add()
            try:
                keep = torch.ones(rows, dtype=torch.bool, device=dev)
                keep[ids] = False
                kept = x[keep].contiguous()
                assert kept.shape[0] == last["ntotal"]

                def reset_add(ix):
                    ix.reset()
                    ix.add(kept)

                r["reset_add_ms"] = median_ms(fresh, reset_add, args.calls, args.warmup)
                r["reset_add_over_remove"] = round(r["reset_add_ms"] / r["remove_ms"], 3)
                del kept, keep
            except torch.OutOfMemoryError:  # the second copy does not fit
                r["reset_add_ms"] = None
            res["patterns"][pname] = r
        out["indexes"][name] = res
        del x
        torch.cuda.empty_cache()
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())

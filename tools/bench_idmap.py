#!/usr/bin/env python
"""Stable ids (IndexIDMap2 / add_with_ids) against the same operations on a
twin index without labels.

Indexes: BASELINE config (b) as tools/bench_select.py builds it (1M x 384 fp32,
the synthetic corpus of bench.py) and 10M x 768 bfloat16.  Labels are a random
permutation of [0, rows) times 7 (unique, unordered, none equal to its row).
Median wall clock of a synchronised call (--calls after --warmup), k = 10:

  search            nq = 1000 and nq = 1 device-resident queries on the labelled
                    index against the twin (the label load at the writers of I)
  selector build    IDSelectorRange / IDSelectorBitmap / IDSelectorBatch of 1 %
                    and 10 % of the ids, by label against the same selector by
                    row on the twin (fx_selector_create + its counts read back)
  remove_ids        1 % scattered ids removed, with and without labels (one
                    call each on a fresh copy: the rows are rebuilt in between)
  rows_of_ids       1 and 10,000 labels -> rows (labelled index only)

Prints one JSON line and writes it to profiles/bench_idmap.json.  Single-box
numbers, not gated by any test.
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
K = 10
INDEXES = [("b_f32_384", 1_000_000, 384, "float32"), ("bf16_768_10m", 10_000_000, 768, "bfloat16")]


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


def build(rows, dim, dtype, dev, labels=None):
    flat = fx.IndexFlatL2(dim, dtype=dtype)
    flat.reserve(rows)
    ix = fx.IndexIDMap2(flat) if labels is not None else flat
    chunk = 1 << 19
    buf = torch.empty((min(chunk, rows), dim), dtype=torch.float32, device=dev)
    for r0 in range(0, rows, chunk):
        part = buf[: min(chunk, rows - r0)]
        fx.synth_fill(part, r0, CORPUS_SEED)
        if labels is not None:
            ix.add_with_ids(part, labels[r0:r0 + part.shape[0]].contiguous())
        else:
            ix.add(part)
    return ix


def selector_builds(rows, perm, labels):
    """name -> (selector by row for the twin, the same selection by label)."""
    bits = torch.zeros((rows * 7 + 7) // 8, dtype=torch.uint8)
    half = labels[: rows // 2].cpu()  # the labels of the first half of the rows
    bits.index_put_((half >> 3,), (1 << (half & 7)).to(torch.uint8), accumulate=True)  # (labels are unique)
    row_bits = torch.full((rows // 16,), 0xff, dtype=torch.uint8)  # rows [0, rows / 2)
    out = {
        "range": (fx.IDSelectorRange(rows // 4, rows // 2), fx.IDSelectorRange(7 * (rows // 4), 7 * (rows // 2))),
        "bitmap": (fx.IDSelectorBitmap(row_bits.cuda()), fx.IDSelectorBitmap(bits.cuda())),
    }
    for pct in (1, 10):
        r = perm[: rows * pct // 100].contiguous()
        out[f"ids_{pct}pct"] = (fx.IDSelectorBatch(r), fx.IDSelectorBatch(labels[r].contiguous()))
    return out


def build_ms(make, index, calls, warmup):
    """fx_selector_create on `index` + its counts (a fresh selector object per call: nothing cached)."""
    def once():
        make().stats(index)
    return timed(once, calls, warmup)


def clone_sel(sel):
    if isinstance(sel, fx.IDSelectorRange):
        return fx.IDSelectorRange(sel.imin, sel.imax)
    if isinstance(sel, fx.IDSelectorBitmap):
        return fx.IDSelectorBitmap(sel.bitmap)
    return fx.IDSelectorBatch(sel.ids)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="", help="run one index by name")
    ap.add_argument("--rows", type=int, default=0, help="override the row counts (testing)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bench_idmap.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = {"bench": "idmap", "k": K, "calls": args.calls, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0), "indexes": {}}
    for name, rows, dim, dtype in INDEXES:
        if args.only and name != args.only:
            continue
        rows = args.rows or rows
        g = torch.Generator(device=dev)
        g.manual_seed(7)
        perm = torch.randperm(rows, device=dev, generator=g)
        labels = (torch.randperm(rows, device=dev, generator=g) * 7).contiguous()
        idx = build(rows, dim, dtype, dev, labels)
        twin = build(rows, dim, dtype, dev)
        res = {"rows": rows, "dim": dim, "dtype": dtype}
        # 1. search
        for nq in (1000, 1):
            xq = torch.empty((nq, dim), dtype=torch.float32, device=dev)
            fx.synth_fill(xq, 0, QUERY_SEED)
            torch.cuda.synchronize()
            a = timed(lambda: idx.search(xq, K), args.calls, args.warmup)
            b = timed(lambda: twin.search(xq, K), args.calls, args.warmup)
            res[f"search_nq{nq}"] = {"labelled_ms": a, "twin_ms": b, "ratio": round(a / b, 4)}
        # 2. selector builds
        sb = {}
        for sname, (by_row, by_label) in selector_builds(rows, perm, labels).items():
            a = build_ms(lambda: clone_sel(by_label), idx, args.calls, args.warmup)
            b = build_ms(lambda: clone_sel(by_row), twin, args.calls, args.warmup)
            sb[sname] = {"by_label_ms": a, "by_row_ms": b, "ratio": round(a / b, 4),
                         "rows_selected": (by_label.stats(idx)["rows"], by_row.stats(twin)["rows"])}
        res["selector_build"] = sb
        # 4. rows_of_ids (before the removal)
        for n in (1, 10_000):
            ask = labels[perm[:n]].contiguous()
            res[f"rows_of_ids_{n}"] = {"ms": timed(lambda: idx.index.rows_of_ids(ask), args.calls, args.warmup)}
        # 3. remove_ids of 1 % scattered ids: one timed call each (it changes the index)
        gone_rows = perm[: rows // 100].contiguous()
        gone_labels = labels[gone_rows].contiguous()
        rm = {}
        for key, index, ids in (("labelled", idx, gone_labels), ("twin", twin, gone_rows)):
            sel = fx.IDSelectorBatch(ids)
            sel.stats(index)  # the selector's build is item 2's; time the removal alone
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = index.remove_ids(sel)
            torch.cuda.synchronize()
            rm[key] = {"ms": round((time.perf_counter() - t0) * 1e3, 4), "removed": n}
        rm["ratio"] = round(rm["labelled"]["ms"] / rm["twin"]["ms"], 4)
        res["remove_1pct"] = rm
        out["indexes"][name] = res
        del idx, twin
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if not args.only and not args.rows:
        Path(args.out).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

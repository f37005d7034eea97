#!/usr/bin/env python3
"""GPU timing of filtered top-k (ops.similarity_topk_filtered) beside the unfiltered call on the same bf16 gallery, one JSON line per
case, appended to profiles/topk_filtered_bench.jsonl.
    python tools/topk_filtered_bench.py                 # the cases below
    python tools/topk_filtered_bench.py 512x1000000 100 # one eq / 16-uniform-class call shape, 20 calls (for rocprofv3 --kernel-trace)
Time = every launch of one call, calls enqueued back to back (HIP events on the launch stream), as tools/topk_wide_bench.py measures it."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from cor_amd import ops, _native as nat
dev = "cuda:0"
OUT = os.path.join(ROOT, "profiles", "topk_filtered_bench.jsonl")


def timed(fn, n):
    for _ in range(2):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def gallery(Bq, Ng):
    g = torch.Generator(device=dev).manual_seed(Bq + Ng)
    Q = torch.nn.functional.normalize(torch.randn((Bq, 256), device=dev, generator=g), dim=-1)
    G = torch.nn.functional.normalize(torch.randn((Ng, 256), device=dev, generator=g), dim=-1).to(torch.bfloat16)
    return Q, G, g


def labels(layout, Bq, Ng, g):
    if layout == "uniform16":
        return torch.randint(0, 16, (Ng,), device=dev, generator=g, dtype=torch.int32), torch.randint(0, 16, (Bq,), device=dev, generator=g, dtype=torch.int32)
    if layout == "blocks16":
        return (torch.arange(Ng, device=dev) * 16 // Ng).to(torch.int32), torch.randint(0, 16, (Bq,), device=dev, generator=g, dtype=torch.int32)
    rl = torch.repeat_interleave(torch.arange(Ng, device=dev), torch.randint(1, 9, (Ng,), device=dev, generator=g))[:Ng].to(torch.int32)   # runs
    return rl, rl[torch.randint(0, Ng, (Bq,), device=dev, generator=g)]


CASES = [(512, 1000000, k, lay, "eq") for k in (10, 100) for lay in ("uniform16", "blocks16")] + [(512, 1000000, 100, "runs", "ne")] + \
        [(512, 125000, k, "uniform16", "eq") for k in (10, 100)] + [(512, 12500, 10, "uniform16", "eq")]
one = len(sys.argv) > 2
if one:
    Bq, Ng = (int(v) for v in sys.argv[1].split("x"))
    CASES = [(Bq, Ng, int(sys.argv[2]), "uniform16", "eq")]
rows = []
for Bq, Ng, k, lay, mode in CASES:
    Q, G, g = gallery(Bq, Ng)
    rl, ql = labels(lay, Bq, Ng, g)
    n = 20 if one else 10
    us = timed(lambda: ops.similarity_topk_filtered(Q, G, k, rl, ql, mode=mode), n)
    if one:
        continue
    base = timed(lambda: ops.similarity_topk(Q, G, k), n)
    us2 = timed(lambda: ops.similarity_topk_filtered(Q, G, k, rl, ql, mode=mode), n)       # again, after the unfiltered calls
    _, raw = ops.similarity_topk_filtered(Q, G, k, rl, ql, mode=mode, flags=nat.TOPK_NO_FALLBACK)
    r = dict(Bq=Bq, Ng=Ng, k=k, dtype="torch.bfloat16", labels=lay, mode=mode, us_filtered=[us, us2], us_unfiltered=base,
             ratio=min(us, us2) / base, queries_overflowed=int((raw == -2).any(dim=1).sum()))
    print(json.dumps(r), flush=True)
    rows.append(r)
if rows:
    with open(OUT, "a") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")

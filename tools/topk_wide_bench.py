#!/usr/bin/env python3
"""GPU timing of wide-k cor_similarity_topk (33 <= k <= 256) beside the k = 10 call on the same shapes, one JSON line per (shape, k).
    python tools/topk_wide_bench.py                  # the shapes below, k = 10 / 100 / 256 as listed
    python tools/topk_wide_bench.py 512x125000 100   # one bf16 shape and k (for rocprofv3 --kernel-trace passes), 20 calls
    python tools/topk_wide_bench.py fallback         # the overflow path: 32 queries against 1M identical rows at k = 100
Time = every launch of one call, calls enqueued back to back (HIP events on the launch stream), as tools/sim_bench.py measures it."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from cor_amd import ops, _native as nat
dev = "cuda:0"
CASES = ((512, 1000000, (10, 100, 256)), (512, 125000, (10, 100)), (32, 100000, (10, 100)))


def timed(Q, G, k, n, flags=0):
    for _ in range(2):
        ops.similarity_topk(Q, G, k, flags=flags)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        ops.similarity_topk(Q, G, k, flags=flags)
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def gallery(Bq, Ng):
    g = torch.Generator(device=dev).manual_seed(Bq + Ng)
    Q = torch.nn.functional.normalize(torch.randn((Bq, 256), device=dev, generator=g), dim=-1)
    G = torch.nn.functional.normalize(torch.randn((Ng, 256), device=dev, generator=g), dim=-1).to(torch.bfloat16)
    return Q, G


if len(sys.argv) > 1 and sys.argv[1] == "fallback":
    Q, _ = gallery(32, 1)
    row = torch.nn.functional.normalize(torch.randn((1, 256), device=dev), dim=-1)
    G = row.repeat(1000000, 1).to(torch.bfloat16)
    _, raw = ops.similarity_topk(Q, G, 100, flags=nat.TOPK_NO_FALLBACK)
    print(json.dumps(dict(Bq=32, Ng=1000000, k=100, dtype="torch.bfloat16", what="every query overflows: exact in-kernel fallback",
                          queries_flagged=int((raw == -2).all(dim=1).sum()), us_per_call=timed(Q, G, 100, 2))), flush=True)
    sys.exit(0)
if len(sys.argv) > 2:
    Bq, Ng = (int(v) for v in sys.argv[1].split("x"))
    CASES = ((Bq, Ng, (int(sys.argv[2]),)),)
for Bq, Ng, ks in CASES:
    Q, G = gallery(Bq, Ng)
    base = None
    for k in ks:
        us = timed(Q, G, k, 20 if len(sys.argv) > 2 else 10)
        base = us if k == 10 else base
        _, raw = ops.similarity_topk(Q, G, k, flags=nat.TOPK_NO_FALLBACK)
        print(json.dumps(dict(Bq=Bq, Ng=Ng, k=k, dtype="torch.bfloat16", us_back_to_back=us, vs_k10=us / base if base else None,
                              queries_overflowed=int((raw == -2).any(dim=1).sum()))), flush=True)

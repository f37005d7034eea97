#!/usr/bin/env python3
"""GPU timing of distinct-group top-k (ops.similarity_topk_distinct), grouped only and grouped + `ne` (the query's own image excluded), beside
three yardsticks taken from ANOTHER build of the library (the parent commit's libcor_amd.so, loaded next to this one in the same process):
(i) its similarity_topk at the same k, (ii) its similarity_topk_filtered `ne` at the same k, (iii) what a user did before this call
existed: its similarity_topk(k=256), the copy to the host and a torch dedupe by image id. One JSON line per case, appended to
profiles/topk_distinct_bench.jsonl; bf16, image ids in runs of 1-8 rows.
    python tools/topk_distinct_bench.py PARENT_LIB.so                  # the cases below
    python tools/topk_distinct_bench.py PARENT_LIB.so 512x1000000 100  # one shape, 20 grouped calls only (for rocprofv3 --kernel-trace)
    python tools/topk_distinct_bench.py PARENT_LIB.so fallback         # the paging fallback on 20 000 rows with 5 000 identical ones
Time = every launch of one call, calls enqueued back to back (HIP events on the launch stream), as tools/topk_filtered_bench.py measures
it, over a window of >= 50 ms (at least 20 calls) after warm-up; (iii) is host wall time per call (it ends on the host). The new call and
the yardsticks (i) / (ii) are all called through ctypes with preallocated outputs, so the two sides carry the same host work."""
import ctypes as C
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from cor_amd import ops, _native as nat
dev = "cuda:0"
OUT = os.path.join(ROOT, "profiles", "topk_distinct_bench.jsonl")

nat.load()
parent = C.CDLL(os.path.abspath(sys.argv[1]))
for name in ("cor_topk_workspace_bytes", "cor_similarity_topk", "cor_topk_filtered_workspace_bytes", "cor_similarity_topk_filtered"):
    fn = getattr(parent, name)
    fn.argtypes = nat.SIGNATURES[name]
    fn.restype = C.c_long if name.endswith("_bytes") else C.c_int


def parent_topk(Q, G, k, out):
    Bq, Ng = Q.shape[0], G.shape[0]
    ws = torch.empty((parent.cor_topk_workspace_bytes(Bq, Ng, k),), dtype=torch.uint8, device=dev)
    s, i = out
    rc = parent.cor_similarity_topk(Q.data_ptr(), G.data_ptr(), nat.BF16, Bq, Ng, 256, k, 0, s.data_ptr(), i.data_ptr(), ws.data_ptr(), 0,
                                    torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    return s, i


def parent_filtered(Q, G, k, rl, ql, out):
    Bq, Ng = Q.shape[0], G.shape[0]
    ws = torch.empty((parent.cor_topk_filtered_workspace_bytes(Bq, Ng, k),), dtype=torch.uint8, device=dev)
    s, i = out
    rc = parent.cor_similarity_topk_filtered(Q.data_ptr(), G.data_ptr(), nat.BF16, Bq, Ng, 256, k, 0, rl.data_ptr(), ql.data_ptr(), nat.FILTER_NE,
                                             s.data_ptr(), i.data_ptr(), ws.data_ptr(), 0, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    return s, i


def new_distinct(Q, G, k, groups, rl, ql, out, flags=0):
    lib = nat.load()
    Bq, Ng = Q.shape[0], G.shape[0]
    ws = torch.empty((lib.cor_topk_distinct_workspace_bytes(Bq, Ng, k),), dtype=torch.uint8, device=dev)
    s, i = out
    rc = lib.cor_similarity_topk_distinct(Q.data_ptr(), G.data_ptr(), nat.BF16, Bq, Ng, 256, k, 0, groups.data_ptr(), rl.data_ptr() if rl is not None else None,
                                          ql.data_ptr() if ql is not None else None, nat.FILTER_NE, s.data_ptr(), i.data_ptr(), ws.data_ptr(), flags,
                                          torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    return s, i


def today(Q, G, k, groups_host, out):
    """(iii): top-256 rows, to the host, first row of each image, first k (may come back short: no guarantee of k images)"""
    s, i = parent_topk(Q, G, 256, out)
    s, i = s.cpu(), i.cpu()
    g = groups_host[i]
    order = torch.sort(g, dim=1, stable=True).indices
    gs = torch.gather(g, 1, order)
    head = torch.ones_like(gs, dtype=torch.bool)
    head[:, 1:] = gs[:, 1:] != gs[:, :-1]
    keep = torch.zeros_like(head).scatter_(1, order, head)
    first = torch.sort((~keep).to(torch.int8), dim=1, stable=True).indices[:, :k]
    return torch.gather(s, 1, first), torch.gather(i, 1, first)


def timed(fn, n=None):
    """us per call; n = None: as many calls as fill ~50 ms (at least 20), sized from a first window of 5"""
    def window(m):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(m):
            fn()
        e1.record(); e1.synchronize()
        return e0.elapsed_time(e1) / m * 1e3
    for _ in range(3):
        fn()
    if n is None:
        n = max(20, min(1000, int(50e3 / max(window(5), 1.0))))
    return window(n)


def timed_host(fn, n):
    fn(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    return (time.perf_counter() - t0) / n * 1e6


def gallery(Bq, Ng):
    g = torch.Generator(device=dev).manual_seed(Bq + Ng)
    Q = torch.nn.functional.normalize(torch.randn((Bq, 256), device=dev, generator=g), dim=-1)
    G = torch.nn.functional.normalize(torch.randn((Ng, 256), device=dev, generator=g), dim=-1).to(torch.bfloat16)
    groups = torch.repeat_interleave(torch.arange(Ng, device=dev), torch.randint(1, 9, (Ng,), device=dev, generator=g))[:Ng].to(torch.int32)
    own = groups[torch.randint(0, Ng, (Bq,), device=dev, generator=g)].contiguous()
    return Q, G, groups, own


if len(sys.argv) > 2 and sys.argv[2] == "fallback":
    Q, G, groups, own = gallery(16, 20000)
    dup = torch.randperm(20000, device=dev)[:5000]
    G[dup] = G[dup[0]].clone()
    Q[0] = G[dup[0]].float()
    rows = []
    # fewer groups than k in a larger shard: no finite threshold, the fallback pages through the WHOLE shard (Ng / 2048 pages)
    Q8, G8, _, _ = gallery(8, 100000)
    few = torch.randint(0, 5, (100000,), device=dev, dtype=torch.int32)
    out8 = (torch.empty((8, 10), device=dev), torch.empty((8, 10), dtype=torch.int64, device=dev))
    rows.append(dict(case="fallback_5_groups", Bq=8, Ng=100000, k=10, us_call=timed(lambda: new_distinct(Q8, G8, 10, few, None, None, out8), 3),
                     queries_overflowed=int((new_distinct(Q8, G8, 10, few, None, None, out8, nat.TOPK_NO_FALLBACK)[1] == -2).any(dim=1).sum())))
    print(json.dumps(rows[-1]), flush=True)
    for name, gr in (("one_group", groups.clone().index_fill_(0, dup, 1 << 20)), ("5000_groups", groups.clone().index_copy_(0, dup, (1 << 20) + torch.arange(5000, device=dev, dtype=torch.int32)))):
        for k in (10, 100):
            us = timed(lambda: ops.similarity_topk_distinct(Q, G, k, gr), 5)
            _, raw = ops.similarity_topk_distinct(Q, G, k, gr, flags=nat.TOPK_NO_FALLBACK)
            rows.append(dict(case="fallback_" + name, Bq=16, Ng=20000, k=k, us_call=us, queries_overflowed=int((raw == -2).any(dim=1).sum())))
            print(json.dumps(rows[-1]), flush=True)
else:
    CASES = [(Bq, Ng, k) for Bq, Ng in ((512, 1000000), (512, 125000), (32, 100000)) for k in (10, 100)]
    one = len(sys.argv) > 3
    if one:
        Bq, Ng = (int(v) for v in sys.argv[2].split("x"))
        CASES = [(Bq, Ng, int(sys.argv[3]))]
    rows = []
    for Bq, Ng, k in CASES:
        Q, G, groups, own = gallery(Bq, Ng)
        if one:
            timed(lambda: ops.similarity_topk_distinct(Q, G, k, groups), 20)
            continue
        out_k = (torch.empty((Bq, k), device=dev), torch.empty((Bq, k), dtype=torch.int64, device=dev))
        out_256 = (torch.empty((Bq, 256), device=dev), torch.empty((Bq, 256), dtype=torch.int64, device=dev))
        gh = groups.cpu().long()
        out_n = (torch.empty((Bq, k), device=dev), torch.empty((Bq, k), dtype=torch.int64, device=dev))
        us_g = [timed(lambda: new_distinct(Q, G, k, groups, None, None, out_n))]
        us_gn = [timed(lambda: new_distinct(Q, G, k, groups, groups, own, out_n))]
        us_i = timed(lambda: parent_topk(Q, G, k, out_k))
        us_ii = timed(lambda: parent_filtered(Q, G, k, groups, own, out_k))
        us_256 = timed(lambda: parent_topk(Q, G, 256, out_256))
        us_iii = timed_host(lambda: today(Q, G, k, gh, out_256), 10)
        us_g.append(timed(lambda: new_distinct(Q, G, k, groups, None, None, out_n)))          # again, after the yardsticks
        us_gn.append(timed(lambda: new_distinct(Q, G, k, groups, groups, own, out_n)))
        _, raw = ops.similarity_topk_distinct(Q, G, k, groups, groups, own, mode="ne", flags=nat.TOPK_NO_FALLBACK)
        r = dict(Bq=Bq, Ng=Ng, k=k, dtype="torch.bfloat16", groups="runs1-8", us_distinct=us_g, us_distinct_ne=us_gn, us_parent_topk=us_i,
                 us_parent_filtered_ne=us_ii, us_parent_topk256=us_256, us_today_topk256_host_dedupe=us_iii,
                 ratio_vs_topk=min(us_g) / us_i, ratio_ne_vs_filtered_ne=min(us_gn) / us_ii, ratio_vs_today=min(us_g) / us_iii,
                 queries_overflowed=int((raw == -2).any(dim=1).sum()))
        print(json.dumps(r), flush=True)
        rows.append(r)
if rows:
    with open(OUT, "a") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")

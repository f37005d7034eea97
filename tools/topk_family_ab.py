#!/usr/bin/env python3
"""Same-process A/B of the wide top-k family (similarity_topk at k > 32, _filtered `ne`, _distinct) between ANOTHER build of the library
(the parent commit's libcor_amd.so) and this one, for changes that must leave results and speed as they are.
    python tools/topk_family_ab.py PARENT_LIB.so [ROUNDS=5] [OUT=profiles/topk_family_ab.jsonl]
"This one" is the library cor_amd loads (COR_AMD_LIB selects another build of it).
Both sides are called through ctypes with preallocated outputs and workspace, so they carry the same host work. Per case: the results of
the two builds must be bitwise equal (scores and indices), then ROUNDS rounds alternate parent / new; a round is one window of >= 50 ms
(at least 20 calls, HIP events on the launch stream) after warm-up. The yardstick is the parent's own round-to-round spread: the run
fails if a case's new median exceeds the parent median by more than the parent's (max - min). One JSON line per case; OUT is written
afresh by every run, so it holds one run."""
import ctypes as C
import json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from cor_amd import _native as nat
dev = "cuda:0"
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "topk_family_ab.jsonl")
DT = {torch.float32: nat.F32, torch.bfloat16: nat.BF16, torch.float16: nat.F16}

new = nat.load()
parent = C.CDLL(os.path.abspath(sys.argv[1]))
for name, sig in nat.SIGNATURES.items():
    if "topk" in name and hasattr(parent, name):
        getattr(parent, name).argtypes = sig
        getattr(parent, name).restype = C.c_long if name.endswith("_bytes") else C.c_int


def caller(lib, route, Q, G, k, groups, own):
    """(fn, scores, idx): fn() enqueues one search of `route` on the current stream"""
    Bq, Ng, Cc = Q.shape[0], G.shape[0], Q.shape[1]
    bytes_fn = {"wide": "cor_topk_workspace_bytes", "filtered_ne": "cor_topk_filtered_workspace_bytes", "distinct": "cor_topk_distinct_workspace_bytes"}[route]
    ws = torch.empty((getattr(lib, bytes_fn)(Bq, Ng, k),), dtype=torch.uint8, device=dev)
    s, i = torch.empty((Bq, k), device=dev), torch.empty((Bq, k), dtype=torch.int64, device=dev)
    head = (Q.data_ptr(), G.data_ptr(), DT[G.dtype], Bq, Ng, Cc, k, 0)
    tail = (s.data_ptr(), i.data_ptr(), ws.data_ptr(), 0)
    if route == "wide":
        args, f = head + tail, lib.cor_similarity_topk
    elif route == "filtered_ne":
        args, f = head + (groups.data_ptr(), own.data_ptr(), nat.FILTER_NE) + tail, lib.cor_similarity_topk_filtered
    else:
        args, f = head + (groups.data_ptr(), None, None, nat.FILTER_EQ) + tail, lib.cor_similarity_topk_distinct

    def fn():
        rc = f(*args, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
        return ws                                            # keeps the buffers alive with the closure
    return fn, s, i


def window(fn, m):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(m):
        fn()
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) / m * 1e3


def gallery(Bq, Ng, Cc, dt):
    g = torch.Generator(device=dev).manual_seed(Bq + Ng)
    Q = torch.nn.functional.normalize(torch.randn((Bq, Cc), device=dev, generator=g), dim=-1)
    G = torch.nn.functional.normalize(torch.randn((Ng, Cc), device=dev, generator=g), dim=-1).to(dt)
    groups = torch.repeat_interleave(torch.arange(Ng, device=dev), torch.randint(1, 9, (Ng,), device=dev, generator=g))[:Ng].to(torch.int32)
    own = groups[torch.randint(0, Ng, (Bq,), device=dev, generator=g)].contiguous()
    return Q, G, groups, own


CASES = [("wide", 512, 1000000, 100, 256, torch.bfloat16), ("wide", 512, 125000, 100, 256, torch.bfloat16), ("wide", 64, 20000, 50, 128, torch.float32),
         ("filtered_ne", 512, 1000000, 100, 256, torch.bfloat16), ("distinct", 512, 1000000, 100, 256, torch.bfloat16),
         ("distinct", 512, 1000000, 10, 256, torch.bfloat16)]
rows, data = [], None
for route, Bq, Ng, k, Cc, dt in CASES:
    if data is None or data[0] != (Bq, Ng, Cc, dt):
        data = ((Bq, Ng, Cc, dt), gallery(Bq, Ng, Cc, dt))
    Q, G, groups, own = data[1]
    fp, sp, ip = caller(parent, route, Q, G, k, groups, own)
    fn, sn, inn = caller(new, route, Q, G, k, groups, own)
    for f in (fp, fn, fp, fn, fp, fn):                       # warm-up, and the results to compare
        f()
    torch.cuda.synchronize()
    assert torch.equal(ip, inn) and torch.equal(sp.view(torch.int32), sn.view(torch.int32)), f"{route} {Bq}x{Ng} k={k}: parent and new differ"
    m = max(20, min(1000, int(50e3 / max(window(fp, 5), 1.0))))
    us_p, us_n = [], []
    for _ in range(ROUNDS):
        us_p.append(window(fp, m)); us_n.append(window(fn, m))
    mp, mn, spread = statistics.median(us_p), statistics.median(us_n), max(us_p) - min(us_p)
    r = dict(route=route, Bq=Bq, Ng=Ng, k=k, C=Cc, dtype=str(dt), calls_per_round=m, us_parent=us_p, us_new=us_n, median_parent=mp, median_new=mn,
             parent_spread=spread, bitwise_equal=True, within_margin=mn <= mp + spread)
    print(json.dumps(r), flush=True)
    rows.append(r)
with open(OUT, "w") as f:
    for r in rows:
        f.write(json.dumps(r) + "\n")
bad = [r for r in rows if not r["within_margin"]]
assert not bad, f"slower than the parent beyond its own spread: {[(r['route'], r['Bq'], r['Ng'], r['k']) for r in bad]}"

#!/usr/bin/env python3
"""Filtered threshold search, ops.similarity_range_filtered / cor_similarity_range_filtered, against the two calls it combines. GPU only,
called by no test.
Shapes: 512 x 1M, 512 x 125k and 32 x 100k, bf16 rows (the scan form) and fp32 rows (the tile form), C = 256, k = 100, mode "eq" over 16
classes, uniform and class-sorted (`blocks16`). Floors:
  kth    each query's 100th best ALLOWED score: count ~ 100;
  zero   0.0: count ~ half the allowed rows, the counting path at full load;
  inf    +inf: nothing counts, nothing is listed.
Yardsticks: cor_similarity_topk_filtered at k = 100 (same labels) and the unfiltered cor_similarity_range (same floors) of the PARENT
commit's library when --parent-lib names one (make -C cor_amd/csrc in a checkout of the parent), else of this build, whose kernels for
those calls tools/kernel_disasm_diff.py shows to be the parent's instruction for instruction. Same box, one process, the three sides
alternating over --reps windows of back-to-back calls after --warmup windows; medians and min / max with the mean shader clock over the
timed region. Every filtered range result is checked for fallback markers (COR_TOPK_NO_FALLBACK) before it is timed. One JSON line per
measurement, printed and appended to --out (default profiles/range_filtered_bench.jsonl).
    python tools/range_filtered_bench.py [--reps 7] [--warmup 2] [--parent-lib PATH] [--out FILE] [--only 512x1000000:bf16:uniform16:kth]"""
import argparse, ctypes, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from cor_amd import ops, _native as nat
from cor_amd.utils import ClockSampler

K = 100
SHAPES = ((512, 1000000), (512, 125000), (32, 100000))
DTYPES = ("bf16", "f32")
LAYOUTS = ("uniform16", "blocks16")
FLOORS = ("kth", "zero", "inf")
DT = dict(bf16=torch.bfloat16, f32=torch.float32)
dev = "cuda:0"


def window_us(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def alternate(fns, n, warmup, reps):
    for _ in range(warmup):
        for f in fns:
            window_us(f, n)
    t = [[] for _ in fns]
    for _ in range(reps):
        for j, f in enumerate(fns):
            t[j].append(window_us(f, n))
    return t


def gallery(Bq, Ng, dt):
    g = torch.Generator(device=dev).manual_seed(Bq + Ng)
    Q = torch.nn.functional.normalize(torch.randn((Bq, 256), device=dev, generator=g), dim=-1)
    G = torch.nn.functional.normalize(torch.randn((Ng, 256), device=dev, generator=g), dim=-1).to(dt)
    return Q, G


def labels(layout, Bq, Ng):
    g = torch.Generator(device=dev).manual_seed(Ng + 7 * Bq)
    ql = torch.randint(0, 16, (Bq,), device=dev, generator=g, dtype=torch.int32)
    if layout == "uniform16":
        return torch.randint(0, 16, (Ng,), device=dev, generator=g, dtype=torch.int32), ql
    return ((torch.arange(Ng, device=dev, dtype=torch.int64) * 16) // Ng).to(torch.int32), ql


def parent_calls(path):
    """cor_similarity_topk_filtered and cor_similarity_range of another build of the library, with buffers of their own (the launches only)."""
    lib = ctypes.CDLL(path)
    for name in ("cor_similarity_topk_filtered", "cor_similarity_range", "cor_topk_filtered_workspace_bytes", "cor_range_workspace_bytes"):
        getattr(lib, name).argtypes = nat.SIGNATURES[name]
    lib.cor_topk_filtered_workspace_bytes.restype = lib.cor_range_workspace_bytes.restype = ctypes.c_long
    code = {torch.float32: nat.F32, torch.bfloat16: nat.BF16, torch.float16: nat.F16}

    def buffers(nbytes, Bq, k):
        return (torch.empty((nbytes,), dtype=torch.uint8, device=dev), torch.empty((Bq, k), dtype=torch.float32, device=dev),
                torch.empty((Bq, k), dtype=torch.int64, device=dev))

    def topk_filtered(Q, G, k, rl, ql):
        Bq, Ng = Q.shape[0], G.shape[0]
        ws, s, i = buffers(lib.cor_topk_filtered_workspace_bytes(Bq, Ng, k), Bq, k)
        nat.check(lib.cor_similarity_topk_filtered(Q.data_ptr(), G.data_ptr(), code[G.dtype], Bq, Ng, 256, k, 0, rl.data_ptr(), ql.data_ptr(),
                                                   nat.FILTER_EQ, s.data_ptr(), i.data_ptr(), ws.data_ptr(), 0,
                                                   torch.cuda.current_stream().cuda_stream), "parent cor_similarity_topk_filtered")

    def range_(Q, G, thr, k):
        Bq, Ng = Q.shape[0], G.shape[0]
        ws, s, i = buffers(lib.cor_range_workspace_bytes(Bq, Ng, k), Bq, k)
        c = torch.empty((Bq,), dtype=torch.int32, device=dev)
        nat.check(lib.cor_similarity_range(Q.data_ptr(), G.data_ptr(), code[G.dtype], Bq, Ng, 256, thr.data_ptr(), k, 0, s.data_ptr(), i.data_ptr(),
                                           c.data_ptr(), ws.data_ptr(), 0, torch.cuda.current_stream().cuda_stream), "parent cor_similarity_range")
    return topk_filtered, range_


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--only", default=None, help="BqxNg:dtype:layout:floor, one measurement (for a rocprofv3 --kernel-trace run of its own)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "range_filtered_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("range_filtered_bench.py measures on the GPU (no CPU path)")
    med = statistics.median
    if a.parent_lib:
        topk_filtered, range_ = parent_calls(a.parent_lib)
    else:
        topk_filtered = lambda Q, G, k, rl, ql: ops.similarity_topk_filtered(Q, G, k, rl, ql)
        range_ = lambda Q, G, thr, k: ops.similarity_range(Q, G, thr, k)
    only = a.only.split(":") if a.only else None
    rows = []
    for Bq, Ng in SHAPES:
        for dn in DTYPES:
            if only and only[:2] != [f"{Bq}x{Ng}", dn]:
                continue
            Q, G = gallery(Bq, Ng, DT[dn])
            for layout in LAYOUTS:
                if only and only[2] != layout:
                    continue
                rl, ql = labels(layout, Bq, Ng)
                kth = ops.similarity_topk_filtered(Q, G, K, rl, ql)[0][:, K - 1].contiguous()
                for fl in FLOORS:
                    if only and only[3] != fl:
                        continue
                    thr = dict(kth=kth, zero=torch.zeros_like(kth), inf=torch.full_like(kth, float("inf")))[fl]
                    _, raw, cnt = ops.similarity_range_filtered(Q, G, thr, K, rl, ql, flags=nat.TOPK_NO_FALLBACK)
                    n = 10 if Ng >= 500000 else 40
                    clock = ClockSampler(dev).start()
                    tf, tt, tr = alternate((lambda: ops.similarity_range_filtered(Q, G, thr, K, rl, ql), lambda: topk_filtered(Q, G, K, rl, ql),
                                            lambda: range_(Q, G, thr, K)), n, a.warmup, a.reps)
                    clock = clock.stop()
                    r = dict(bench="range_filtered", Bq=Bq, Ng=Ng, C=256, k=K, dtype=dn, labels=layout, mode="eq", floor=fl,
                             range_filtered_us=med(tf), range_filtered_us_min_max=[min(tf), max(tf)],
                             topk_filtered_us=med(tt), topk_filtered_us_min_max=[min(tt), max(tt)],
                             range_us=med(tr), range_us_min_max=[min(tr), max(tr)],
                             over_topk_filtered=med(tf) / med(tt), over_range=med(tf) / med(tr), over_sum=med(tf) / (med(tt) + med(tr)),
                             yardstick="parent library" if a.parent_lib else "this build (those calls' kernels identical to the parent's)",
                             count_mean=float(cnt.float().mean()), count_min_max=[int(cnt.min()), int(cnt.max())],
                             queries_on_fallback=int((raw == -2).any(dim=1).sum()), calls_per_window=n, reps=a.reps,
                             sclk_mhz_mean=clock.get("sclk_mhz_mean"))
                    print(json.dumps(r), flush=True)
                    rows.append(r)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

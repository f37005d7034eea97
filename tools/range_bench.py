#!/usr/bin/env python3
"""Threshold (range) search, ops.similarity_range / cor_similarity_range, against the wide top-k it extends. GPU only, called by no test.
Shapes: 512 x 1M, 512 x 125k and 32 x 100k, bf16 rows at C = 256 (the scan form), and 512 x 1M fp32 (the tile form); k = 100. Floors:
  kth    each query's 100th best score: count ~ 100, the scan does the top-k's work plus the floor compares;
  zero   0.0: count ~ Ng / 2, the counting path at full load;
  inf    +inf: nothing counts, nothing is listed.
Yardstick: cor_similarity_topk at k = 100 (the wide route on both sides) of the PARENT commit's library when --parent-lib names one
(make -C cor_amd/csrc in a checkout of the parent), else of this build, whose top-k kernels tools/kernel_disasm_diff.py shows to be the
parent's instruction for instruction. Same box, one process, the two sides alternating over --reps windows of back-to-back calls after
--warmup windows; medians and min / max with the mean shader clock over the timed region. Every range result is checked for fallback
markers (COR_TOPK_NO_FALLBACK) before it is timed. `fallback`: 32 queries against 1M identical rows, every query on the in-kernel chain
pass that ranks and counts. One JSON line per measurement, printed and appended to --out (default profiles/range_bench.jsonl).
    python tools/range_bench.py [--reps 7] [--warmup 2] [--parent-lib PATH] [--out FILE] [--only 512x1000000:bf16:kth] [--fallback]"""
import argparse, ctypes, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from cor_amd import ops, _native as nat
from cor_amd.utils import ClockSampler

K = 100
SHAPES = ((512, 1000000, "bf16"), (512, 125000, "bf16"), (32, 100000, "bf16"), (512, 1000000, "f32"))
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


def alternate(fa, fb, n, warmup, reps):
    for _ in range(warmup):
        window_us(fa, n); window_us(fb, n)
    ta, tb = [], []
    for _ in range(reps):
        ta.append(window_us(fa, n)); tb.append(window_us(fb, n))
    return ta, tb


def gallery(Bq, Ng, dt):
    g = torch.Generator(device=dev).manual_seed(Bq + Ng)
    Q = torch.nn.functional.normalize(torch.randn((Bq, 256), device=dev, generator=g), dim=-1)
    G = torch.nn.functional.normalize(torch.randn((Ng, 256), device=dev, generator=g), dim=-1).to(dt)
    return Q, G


def parent_topk(path):
    """cor_similarity_topk of another build of the library, with buffers of its own: (Q, G, k) -> None (the launches only)."""
    lib = ctypes.CDLL(path)
    lib.cor_similarity_topk.argtypes = nat.SIGNATURES["cor_similarity_topk"]
    lib.cor_topk_workspace_bytes.argtypes = nat.SIGNATURES["cor_topk_workspace_bytes"]
    lib.cor_topk_workspace_bytes.restype = ctypes.c_long
    code = {torch.float32: nat.F32, torch.bfloat16: nat.BF16, torch.float16: nat.F16}

    def call(Q, G, k):
        Bq, Ng = Q.shape[0], G.shape[0]
        ws = torch.empty((lib.cor_topk_workspace_bytes(Bq, Ng, k),), dtype=torch.uint8, device=dev)
        s = torch.empty((Bq, k), dtype=torch.float32, device=dev)
        i = torch.empty((Bq, k), dtype=torch.int64, device=dev)
        nat.check(lib.cor_similarity_topk(Q.data_ptr(), G.data_ptr(), code[G.dtype], Bq, Ng, 256, k, 0, s.data_ptr(), i.data_ptr(), ws.data_ptr(), 0,
                                          torch.cuda.current_stream().cuda_stream), "parent cor_similarity_topk")
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--only", default=None, help="BqxNg:dtype:floor, one measurement (for a rocprofv3 --kernel-trace run of its own)")
    ap.add_argument("--fallback", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "range_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("range_bench.py measures on the GPU (no CPU path)")
    med = statistics.median
    topk = parent_topk(a.parent_lib) if a.parent_lib else (lambda Q, G, k: ops.similarity_topk(Q, G, k))
    rows = []

    def emit(r):
        print(json.dumps(r), flush=True)
        rows.append(r)

    if a.fallback:
        Q, _ = gallery(32, 1, torch.bfloat16)
        G = torch.nn.functional.normalize(torch.randn((1, 256), device=dev), dim=-1).repeat(1000000, 1).to(torch.bfloat16)
        _, raw, cnt = ops.similarity_range(Q, G, 0.0, K, flags=nat.TOPK_NO_FALLBACK)
        s, i, c = ops.similarity_range(Q, G, -1.0, K)
        t = [window_us(lambda: ops.similarity_range(Q, G, -1.0, K), 2) for _ in range(3)]
        tk = [window_us(lambda: ops.similarity_topk(Q, G, K), 2) for _ in range(3)]
        emit(dict(bench="range_fallback", Bq=32, Ng=1000000, k=K, dtype="bf16", what="every query overflows: in-kernel chain pass that ranks and counts",
                  queries_flagged=int((raw == -2).all(dim=1).sum()), counts_flagged=int((cnt == -2).sum()), counts_all_rows=bool((c == 1000000).all()),
                  range_ms_per_call=med(t) / 1e3, topk_fallback_ms_per_call=med(tk) / 1e3, ms_per_query=med(t) / 1e3 / 32))
    else:
        for Bq, Ng, dn in SHAPES:
            if a.only and a.only.split(":")[:2] != [f"{Bq}x{Ng}", dn]:
                continue
            Q, G = gallery(Bq, Ng, DT[dn])
            kth = ops.similarity_topk(Q, G, K)[0][:, K - 1].contiguous()
            for fl in FLOORS:
                if a.only and a.only.split(":")[2] != fl:
                    continue
                thr = dict(kth=kth, zero=torch.zeros_like(kth), inf=torch.full_like(kth, float("inf")))[fl]
                _, raw, cnt = ops.similarity_range(Q, G, thr, K, flags=nat.TOPK_NO_FALLBACK)
                n = 10 if Ng >= 500000 else 40
                clock = ClockSampler(dev).start()
                tr, tt = alternate(lambda: ops.similarity_range(Q, G, thr, K), lambda: topk(Q, G, K), n, a.warmup, a.reps)
                clock = clock.stop()
                emit(dict(bench="range", Bq=Bq, Ng=Ng, C=256, k=K, dtype=dn, floor=fl, range_us=med(tr), range_us_min_max=[min(tr), max(tr)],
                          topk_us=med(tt), topk_us_min_max=[min(tt), max(tt)], range_over_topk=med(tr) / med(tt), yardstick="parent library" if
                          a.parent_lib else "this build (top-k kernels identical to the parent's)", count_mean=float(cnt.float().mean()),
                          count_min_max=[int(cnt.min()), int(cnt.max())], queries_on_fallback=int((raw == -2).any(dim=1).sum()), calls_per_window=n,
                          reps=a.reps, sclk_mhz_mean=clock.get("sclk_mhz_mean")))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Query expansion (ops.expand_queries) against what a user writes today and against the bytes it must move. GPU only.
Shapes, C = 256, a 1M-row gallery in bf16 and fp32, lists of random present rows with scores in [0.1, 1], alpha = 3:
  query expansion   Bq = 512, m in {10, 100}, query_weight = 1, fp32 result;
  DBA               Bq = 65536 (one batch of gallery rows), m = 10, query_weight = 0, result in the gallery dtype.
  kernel_us    ops.expand_queries, device events around a window of back-to-back launches;
  torch_us     yardstick 1, the same device, the same window: F.normalize(w * Q + (s.clamp(min=0) ** alpha)[:, :, None] * G[idx].float()).sum(1))
               (torch's reduction order: not the same bits; it materialises [Bq, m, C] in fp32);
  floor_us     yardstick 2: the bytes the call must gather (Bq * m rows of C values) over the measured copy bandwidth of the project
               (6.29 TB/s); kernel_over_floor = kernel_us / floor_us.
The two timed sides alternate over --reps windows after --warmup windows; medians and min/max are reported, with the largest relative
difference between the two results. One JSON line per measurement, printed and appended to --out (default profiles/expand_bench.jsonl).
    python tools/expand_bench.py [--reps 7] [--warmup 2] [--rows 1000000] [--out FILE]"""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from cor_amd import ops
from cor_amd.utils import ClockSampler

COPY_TBS = 6.29          # measured float4 copy bandwidth, TB/s
C, ALPHA = 256, 3
SHAPES = (("aqe", 512, 10), ("aqe", 512, 100), ("dba", 65536, 10))
dev = "cuda:0"


def window_us(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def alternate(fa, fb, na, nb, warmup, reps):
    for _ in range(warmup):
        window_us(fa, na); window_us(fb, nb)
    ta, tb = [], []
    for _ in range(reps):
        ta.append(window_us(fa, na)); tb.append(window_us(fb, nb))
    return ta, tb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "expand_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("expand_bench.py measures on the GPU (no CPU path)")
    gen = torch.Generator(device=dev).manual_seed(1)
    G32 = torch.nn.functional.normalize(torch.randn((a.rows, C), device=dev, generator=gen), dim=-1)
    G16 = G32.to(torch.bfloat16)
    med = statistics.median
    rows = []
    for name, G in (("bf16", G16), ("fp32", G32)):
        for kind, Bq, m in SHAPES:
            Q = torch.nn.functional.normalize(torch.randn((Bq, C), device=dev, generator=gen), dim=-1)
            idx = torch.randint(0, a.rows, (Bq, m), device=dev, generator=gen)
            s = torch.rand((Bq, m), device=dev, generator=gen) * 0.9 + 0.1
            qw, odt = (1.0, torch.float32) if kind == "aqe" else (0.0, G.dtype)

            def kernel():
                return ops.expand_queries(Q if qw else None, [(G, 0)], s, idx, m, alpha=ALPHA, query_weight=qw, out_dtype=odt)

            def eager():
                v = ((s.clamp(min=0) ** ALPHA)[:, :, None] * G[idx].float()).sum(1)
                if qw:
                    v = v + qw * Q
                return torch.nn.functional.normalize(v, dim=-1).to(odt)

            k, e = kernel().float(), eager().float()
            torch.cuda.synchronize()
            diff = float(((k - e).abs().max() / e.abs().max()))
            n_k = max(10, min(2000, int(4e6 / (Bq * m))))        # windows of a few ms
            n_e = max(3, n_k // 4)
            clock = ClockSampler(dev).start()
            tk, te = alternate(kernel, eager, n_k, n_e, a.warmup, a.reps)
            clock = clock.stop()
            nbytes = Bq * m * C * G.element_size()
            floor = nbytes / (COPY_TBS * 1e12) * 1e6
            r = dict(bench="expand", kind=kind, gallery=name, rows=a.rows, Bq=Bq, m=m, C=C, alpha=ALPHA, query_weight=qw, out_dtype=str(odt),
                     kernel_us=med(tk), kernel_us_min_max=[min(tk), max(tk)], torch_us=med(te), torch_us_min_max=[min(te), max(te)],
                     torch_over_kernel=med(te) / med(tk), gather_bytes=nbytes, floor_us=floor, kernel_over_floor=med(tk) / floor,
                     launches_per_window=[n_k, n_e], reps=a.reps, max_rel_diff_to_torch=diff,
                     sclk_mhz_mean=clock.get("sclk_mhz_mean"))
            print(json.dumps(r), flush=True)
            rows.append(r)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

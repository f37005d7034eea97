#!/usr/bin/env python3
"""The list stages over an int8 gallery against their float counterparts and against the bytes they must move. GPU only, called by no
test. 512 queries, C = 256, lists out of a 1M-row gallery (int8 rows + fp32 scales, and the bf16 / fp32 rows they were quantised from):
  rescore      ops.rescore_topk_i8 against ops.rescore_topk over bf16 and over fp32 rows, kin in {100, 256, 1024, 4096} random rows per
               query, k = 10; floor_us = the bytes gathered (Bq * kin * C bytes of int8) over the project's measured copy bandwidth
               (6.29 TB/s);
  expand       ops.expand_queries over an int8 segment against a bf16 segment, m in {10, 100}, lists of random present rows with scores in
               [0.1, 1], alpha = 3, query_weight = 1, fp32 result; and the shape of one augmentation batch, 65536 lists of m = 10 with
               query_weight = 0 (at 512 queries the call is bound by the host's launch rate, tools/expand_bench.py found the same);
               *_graph_us: the same calls captured 50 to a graph and replayed, i.e. the kernels without the host's part of a call;
  dequantize   ops.dequantize_rows_i8 of all rows into fp32 and bf16 against the bytes it reads and writes;
  resident     the bytes an int8-only gallery keeps resident with its neighbour graph (width 20) against the bf16 equivalent (arithmetic on
               the tensors' sizes: the graph's size does not depend on the row dtype).
Device events around windows of back-to-back calls, the two sides alternating over --reps windows after --warmup windows; medians and
min/max are reported with the mean shader clock over each measurement. One JSON line per measurement, printed and appended to --out
(default profiles/i8_lists_bench.jsonl).
    python tools/i8_lists_bench.py [--reps 7] [--warmup 2] [--rows 1000000] [--out FILE]"""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from cor_amd import ops
from cor_amd.utils import ClockSampler

COPY_TBS = 6.29          # measured float4 copy bandwidth, TB/s
BQ, C, K, ALPHA, K1 = 512, 256, 10, 3, 20
KINS = (100, 256, 1024, 4096)
dev = "cuda:0"


def window_us(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def alternate(fns, ns, warmup, reps):
    for _ in range(warmup):
        for f, n in zip(fns, ns):
            window_us(f, n)
    ts = [[] for _ in fns]
    for _ in range(reps):
        for t, f, n in zip(ts, fns, ns):
            t.append(window_us(f, n))
    return ts


def graphed(fn, n):
    """n back-to-back calls of fn captured in ONE graph on one stream: replaying it times the kernels without the host's part of a call."""
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(n):
            fn()
    return g.replay


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "i8_lists_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("i8_lists_bench.py measures on the GPU (no CPU path)")
    gen = torch.Generator(device=dev).manual_seed(1)
    G32 = torch.nn.functional.normalize(torch.randn((a.rows, C), device=dev, generator=gen), dim=-1)
    G16 = G32.to(torch.bfloat16)
    Gq, gs = ops.quantize_rows_i8(G32)
    Q = torch.nn.functional.normalize(torch.randn((BQ, C), device=dev, generator=gen), dim=-1)
    med = statistics.median
    rows = []

    def emit(r):
        print(json.dumps(r), flush=True)
        rows.append(r)

    def mm(t):
        return [min(t), max(t)]

    for kin in KINS:
        cand = torch.randint(0, a.rows, (BQ, kin), device=dev, generator=gen)
        fns = (lambda: ops.rescore_topk_i8(Q, Gq, gs, cand, K), lambda: ops.rescore_topk(Q, G16, cand, K), lambda: ops.rescore_topk(Q, G32, cand, K))
        for f in fns:
            f()
        torch.cuda.synchronize()
        n = max(20, min(2000, int(2e5 / (5 + kin))))
        clock = ClockSampler(dev).start()
        t8, t16, t32 = alternate(fns, (n, n, n), a.warmup, a.reps)
        clock = clock.stop()
        nbytes = BQ * kin * C
        floor = nbytes / (COPY_TBS * 1e12) * 1e6
        emit(dict(bench="rescore_i8", rows=a.rows, Bq=BQ, kin=kin, k=K, C=C, i8_us=med(t8), i8_us_min_max=mm(t8), bf16_us=med(t16),
                  bf16_us_min_max=mm(t16), fp32_us=med(t32), fp32_us_min_max=mm(t32), bf16_over_i8=med(t16) / med(t8), fp32_over_i8=med(t32) / med(t8),
                  gather_bytes=nbytes, floor_us=floor, i8_over_floor=med(t8) / floor, launches_per_window=n, reps=a.reps,
                  sclk_mhz_mean=clock.get("sclk_mhz_mean")))

    for Bq, m in ((BQ, 10), (BQ, 100), (65536, 10)):
        idx = torch.randint(0, a.rows, (Bq, m), device=dev, generator=gen)
        sc = torch.rand((Bq, m), device=dev, generator=gen) * 0.9 + 0.1
        Qe, qw = (Q, 1.0) if Bq == BQ else (None, 0.0)
        out = torch.empty((Bq, C), device=dev)
        fns = (lambda: ops.expand_queries(Qe, [(Gq, gs, 0)], sc, idx, m, alpha=ALPHA, query_weight=qw, out=out),
               lambda: ops.expand_queries(Qe, [(G16, 0)], sc, idx, m, alpha=ALPHA, query_weight=qw, out=out))
        for f in fns:
            f()
        torch.cuda.synchronize()
        n = 500 if m == 10 and Bq == BQ else 200
        clock = ClockSampler(dev).start()
        t8, t16 = alternate(fns, (n, n), a.warmup, a.reps)
        clock = clock.stop()
        g8, g16 = alternate([graphed(f, 50) for f in fns], (4, 4), a.warmup, a.reps)      # the kernels alone: 50 captured calls per replay
        nbytes = Bq * m * C + Bq * C * 4                        # the int8 rows gathered and the fp32 result
        floor = nbytes / (COPY_TBS * 1e12) * 1e6
        emit(dict(bench="expand_i8", rows=a.rows, Bq=Bq, m=m, query_weight=qw, alpha=ALPHA, C=C, i8_us=med(t8), i8_us_min_max=mm(t8), bf16_us=med(t16),
                  bf16_us_min_max=mm(t16), bf16_over_i8=med(t16) / med(t8), i8_graph_us=med(g8) / 50, bf16_graph_us=med(g16) / 50,
                  bf16_over_i8_graph=med(g16) / med(g8), bytes=nbytes, floor_us=floor, i8_over_floor=med(t8) / floor,
                  launches_per_window=n, reps=a.reps, sclk_mhz_mean=clock.get("sclk_mhz_mean")))

    for name, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        out = torch.empty((a.rows, C), dtype=dt, device=dev)
        fn = lambda: ops.dequantize_rows_i8(Gq, gs, out_dtype=dt, out=out)
        fn()
        torch.cuda.synchronize()
        clock = ClockSampler(dev).start()
        (t,) = alternate((fn,), (20,), a.warmup, a.reps)
        clock = clock.stop()
        nbytes = a.rows * (C + 4 + C * out.element_size())
        emit(dict(bench="dequantize_i8", rows=a.rows, C=C, out=name, us=med(t), us_min_max=mm(t), bytes=nbytes, TBps=nbytes / med(t) / 1e6,
                  floor_us=nbytes / (COPY_TBS * 1e12) * 1e6, over_floor=med(t) / (nbytes / (COPY_TBS * 1e12) * 1e6), reps=a.reps,
                  sclk_mhz_mean=clock.get("sclk_mhz_mean")))
        del out

    graph = a.rows * (K1 * 8 + 4)
    i8, b16 = a.rows * (C + 4), a.rows * C * 2
    emit(dict(bench="resident_bytes", rows=a.rows, C=C, graph_width=K1, graph_bytes=graph, i8_rows_and_scales=i8, bf16_rows=b16,
              i8_gallery_with_graph=i8 + graph, bf16_gallery_with_graph=b16 + graph, bf16_over_i8=(b16 + graph) / (i8 + graph),
              i8_coarse_plus_bf16_rows_with_graph=i8 + b16 + graph))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

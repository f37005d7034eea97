#!/usr/bin/env python3
"""Candidate re-scoring (ops.rescore_topk) against what a user writes today and against the bytes it must move. GPU only.
512 queries x kin in {100, 256, 1024, 4096} candidates (random rows of a 1M-row gallery, C = 256, fp32 and bf16), k = 10:
  kernel_us    ops.rescore_topk, device events around a window of back-to-back launches;
  torch_us     yardstick 1, the same device, the same window: torch.bmm(G[idx].float(), Q[:, :, None]) + torch.sort (not the chain
               score: its order can differ in the last bits; no de-duplication, no range test);
  floor_us     yardstick 2: the bytes the call must gather (Bq * kin rows of C values) over the measured copy bandwidth of the project
               (6.29 TB/s); kernel_over_floor = kernel_us / floor_us.
The two timed sides alternate over --reps windows after --warmup windows; medians and min/max are reported.
End to end at 512 x 1M (yardstick 3): retrieval.two_stage_search(bf16 coarse, k_coarse = 100, fp32 fine, k = 10) against
ops.similarity_topk over the fp32 rows at k = 10, both times, and the share of queries whose two-stage top-10 equals the fp32 search's.
One JSON line per measurement, printed and appended to --out (default profiles/rescore_bench.jsonl).
    python tools/rescore_bench.py [--reps 7] [--warmup 2] [--rows 1000000] [--out FILE]"""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from cor_amd import ops, retrieval

COPY_TBS = 6.29          # measured float4 copy bandwidth, TB/s
BQ, C, K = 512, 256, 10
KINS = (100, 256, 1024, 4096)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rescore_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("rescore_bench.py measures on the GPU (no CPU path)")
    gen = torch.Generator(device=dev).manual_seed(1)
    G32 = torch.nn.functional.normalize(torch.randn((a.rows, C), device=dev, generator=gen), dim=-1)
    G16 = G32.to(torch.bfloat16)
    Q = torch.nn.functional.normalize(torch.randn((BQ, C), device=dev, generator=gen), dim=-1)
    med = statistics.median
    rows = []

    def emit(r):
        print(json.dumps(r), flush=True)
        rows.append(r)

    for name, G in (("fp32", G32), ("bf16", G16)):
        for kin in KINS:
            cand = torch.randint(0, a.rows, (BQ, kin), device=dev, generator=gen)

            def kernel():
                return ops.rescore_topk(Q, G, cand, K)

            def eager():
                s = torch.bmm(G[cand].float(), Q[:, :, None]).squeeze(-1)
                v, o = torch.sort(s, dim=1, descending=True)
                return v[:, :K], torch.gather(cand, 1, o[:, :K])

            ks, ki = kernel()
            es, ei = eager()
            torch.cuda.synchronize()
            same_idx = float((ki == ei).all(dim=1).float().mean())
            n_k = max(20, min(2000, int(2e5 / (5 + kin))))       # windows of a few ms up to a few hundred ms
            n_e = max(5, n_k // 4)
            tk, te = alternate(kernel, eager, n_k, n_e, a.warmup, a.reps)
            nbytes = BQ * kin * C * G.element_size()
            floor = nbytes / (COPY_TBS * 1e12) * 1e6
            emit(dict(bench="rescore", gallery=name, rows=a.rows, Bq=BQ, kin=kin, k=K, C=C, kernel_us=med(tk), kernel_us_min_max=[min(tk), max(tk)],
                      torch_us=med(te), torch_us_min_max=[min(te), max(te)], torch_over_kernel=med(te) / med(tk), gather_bytes=nbytes,
                      floor_us=floor, kernel_over_floor=med(tk) / floor, launches_per_window=[n_k, n_e], reps=a.reps,
                      share_queries_same_top10_as_torch=same_idx))

    coarse, fine = retrieval.GalleryShard(G16), retrieval.GalleryShard(G32)

    def two_stage():
        return retrieval.two_stage_search(Q, coarse, fine, K, 100)

    def full_fp32():
        return ops.similarity_topk(Q, G32, K)

    ts, ti = two_stage()
    fs, fi = full_fp32()
    torch.cuda.synchronize()
    equal = float((ti == fi).all(dim=1).float().mean())
    overlap = float(torch.stack([torch.isin(ti[b], fi[b]).float().mean() for b in range(BQ)]).mean())
    t2, tf = alternate(two_stage, full_fp32, 20, 10, a.warmup, a.reps)
    emit(dict(bench="two_stage", rows=a.rows, Bq=BQ, k=K, k_coarse=100, C=C, two_stage_us=med(t2), two_stage_us_min_max=[min(t2), max(t2)],
              fp32_search_us=med(tf), fp32_search_us_min_max=[min(tf), max(tf)], fp32_over_two_stage=med(tf) / med(t2),
              share_queries_same_top10=equal, mean_top10_overlap=overlap, reps=a.reps))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

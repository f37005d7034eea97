#!/usr/bin/env python3
"""Clustering (cor_kmeans_seed, cor_kmeans_update) against its yardsticks. GPU only, called by no test.
Workloads: 1 048 576 x 256 bf16 rows at K = 1024, the int8 copy of the same rows, and 102 400 bf16 rows at K = 256. The rows are unit
vectors around K planted directions; the assignment timed and fed to the update is that of the seeded centres.
  update_us      cor_kmeans_update (six launches) through ctypes, scores given, workspace allocated once;
  floor_us       the bytes the update must read (every row once, its assign and score entry) over the project's measured copy bandwidth
                 (6.29 TB/s); update_over_floor = update_us / floor_us;
  torch_us       what a user writes today on the same device: torch.zeros(K, C).index_add_(0, assign, rows.float()) and a normalise (for
                 int8 rows the dequantised copy is made inside the timed region: it is part of that route);
  assign_us      the assignment pass of the same iteration: centroids.search(rows, 1), 4096 rows at a time, the parent commit's search;
                 update_over_assign = update_us / assign_us (expected <= 1, not a gate);
  seed_us        cor_kmeans_seed (2K launches); seed_floor_us = K passes over the rows' bytes at the same bandwidth.
Device events around every window; update, torch and assignment alternate over --reps windows after --warmup windows in ONE process; the
seeding is timed alone over --seed-reps runs after one warm-up. Medians and min/max are reported with the mean shader clock. One JSON line
per workload, printed and appended to --out (default profiles/cluster_bench.jsonl).
    python tools/cluster_bench.py [--reps 7] [--warmup 2] [--seed-reps 3] [--small] [--out FILE]"""
import argparse, ctypes, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from cor_amd import _native as nat, ops
from cor_amd.retrieval import GalleryShard
from cor_amd.utils import ClockSampler

C = 256
COPY_TBS = 6.29            # measured copy bandwidth, SURVEY.md
dev = "cuda:0"


def timed_us(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed-reps", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="only the 102 400-row workload")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("cluster_bench.py measures on the GPU (no CPU path)")
    lib = nat.load()
    st = torch.cuda.current_stream().cuda_stream
    med = statistics.median
    work = [(102400, 256, "bf16")] if a.small else [(1 << 20, 1024, "bf16"), (1 << 20, 1024, "int8"), (102400, 256, "bf16")]
    out = []
    for n, K, kind in work:
        gen = torch.Generator(device=dev).manual_seed(n + K)
        modes = torch.nn.functional.normalize(torch.randn((K, C), device=dev, generator=gen), dim=-1)
        G32 = torch.nn.functional.normalize(modes[torch.randint(0, K, (n,), device=dev, generator=gen)]
                                            + 0.6 * torch.randn((n, C), device=dev, generator=gen) / C ** 0.5, dim=-1)
        if kind == "int8":
            rows, scales = ops.quantize_rows_i8(G32)
            dt, esize = nat.I8, 1
        else:
            rows, scales, dt, esize = G32.to(torch.bfloat16), None, nat.BF16, 2
        del G32
        seg = ((ctypes.c_void_p * 1)(rows.data_ptr()), (ctypes.c_void_p * 1)(scales.data_ptr() if scales is not None else None),
               (ctypes.c_longlong * 1)(0), (ctypes.c_int * 1)(n), (ctypes.c_int * 1)(dt))
        ws = torch.empty((lib.cor_kmeans_workspace_bytes(n, K, C),), dtype=torch.uint8, device=dev)
        ids = torch.empty((K,), dtype=torch.int64, device=dev)
        cent = torch.empty((K, C), device=dev)

        def seed():
            rc = lib.cor_kmeans_seed(*seg, 1, C, K, 0, ids.data_ptr(), cent.data_ptr(), ws.data_ptr(), st)
            assert rc == 0, rc

        ts = [timed_us(seed) for _ in range(1 + a.seed_reps)][1:]
        centres = GalleryShard(cent.clone())
        assign = torch.empty((n,), dtype=torch.int32, device=dev)
        score = torch.empty((n,), device=dev)

        def queries(lo):
            return ops.dequantize_rows_i8(rows[lo:lo + 4096], scales[lo:lo + 4096]) if kind == "int8" else rows[lo:lo + 4096]

        def assignment():
            for lo in range(0, n, 4096):
                s, i = centres.search(queries(lo), 1)
                assign[lo:lo + 4096] = i[:, 0]
                score[lo:lo + 4096] = s[:, 0]

        new, counts, sums = torch.empty((K, C), device=dev), torch.empty((K,), dtype=torch.int32, device=dev), torch.empty((K,), device=dev)
        seg_a, seg_s = (ctypes.c_void_p * 1)(assign.data_ptr()), (ctypes.c_void_p * 1)(score.data_ptr())

        def update():
            rc = lib.cor_kmeans_update(*seg, 1, seg_a, seg_s, C, K, cent.data_ptr(), new.data_ptr(), counts.data_ptr(), sums.data_ptr(),
                                       ws.data_ptr(), st)
            assert rc == 0, rc

        def torch_way():
            x = ops.dequantize_rows_i8(rows, scales) if kind == "int8" else rows.float()
            return torch.nn.functional.normalize(torch.zeros((K, C), device=dev).index_add_(0, assign.long(), x), dim=-1)

        assignment(); update(); ref = torch_way()
        torch.cuda.synchronize()
        err = (new - ref).abs().max().item()                   # the two routes agree to fp32 summation error
        for _ in range(a.warmup):
            timed_us(update); timed_us(torch_way); timed_us(assignment)
        clock = ClockSampler(dev).start()
        tu, tt, ta = [], [], []
        for _ in range(a.reps):
            tu.append(timed_us(update)); tt.append(timed_us(torch_way)); ta.append(timed_us(assignment))
        clock = clock.stop()
        floor = n * (C * esize + 8 + (4 if kind == "int8" else 0)) / (COPY_TBS * 1e12) * 1e6
        seed_floor = K * n * (C * esize) / (COPY_TBS * 1e12) * 1e6
        r = dict(bench="cluster", rows=n, K=K, C=C, gallery=kind, update_us=med(tu), update_us_min_max=[min(tu), max(tu)], floor_us=floor,
                 update_over_floor=med(tu) / floor, torch_us=med(tt), torch_us_min_max=[min(tt), max(tt)], update_over_torch=med(tu) / med(tt),
                 assign_us=med(ta), assign_us_min_max=[min(ta), max(ta)], update_over_assign=med(tu) / med(ta), seed_us=med(ts),
                 seed_us_min_max=[min(ts), max(ts)], seed_floor_us=seed_floor, seed_over_floor=med(ts) / seed_floor,
                 max_abs_diff_to_torch=err, empty_clusters=int((counts == 0).sum().item()), reps=a.reps, seed_reps=a.seed_reps,
                 sclk_mhz_mean=clock.get("sclk_mhz_mean"))
        print(json.dumps(r), flush=True)
        out.append(r)
        del rows, scales, ws, assign, score
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for r in out:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""List fusion (ops.fuse_lists, cor_fuse_lists) against its sibling kernel and against what a user does today. GPU only.
512 queries, P x kin in {2 x 100, 4 x 256, 8 x 256, 16 x 256}, k = 100; per query every list holds kin distinct ids drawn from a pool of
2 kin ids (so about half of a list's ids occur in any other list) with descending scores; reciprocal-rank fusion and CombSUM with min-max
normalisation.
  fuse_us      ops.fuse_lists, device events around a window of back-to-back calls;
  merge_us     yardstick 1, the same window shape: ops.merge_topk (cor_merge_topk) on the same stacked lists: the sibling kernel, ONE
               bitonic sort of the same npad keys where the fusion has two plus the walk; fuse_over_merge = fuse_us / merge_us. (The
               merge's answer is another one: it keeps a row that two lists name twice.)
  host_ms      yardstick 2, what there is without the kernel: both tensors copied to the host and the NumPy restatement of the definition
               (tests/fuse_refs.py, a Python dict per query), wall clock, run --host-reps times.
The two device sides alternate over --reps windows after --warmup windows; medians and min / max are reported with the mean shader clock
over the timed region. The fusion's ids are checked against the restatement before anything is timed. One JSON line per measurement,
printed and appended to --out (default profiles/fuse_bench.jsonl).
    python tools/fuse_bench.py [--reps 7] [--warmup 2] [--host-reps 1] [--out FILE]"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from cor_amd import ops
from cor_amd.utils import ClockSampler
from tests.fuse_refs import ref_fuse

BQ, K = 512, 100
SHAPES = ((2, 100), (4, 256), (8, 256), (16, 256))
MODES = (dict(mode="rrf"), dict(mode="sum", normalize="minmax"))
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


def lists_of(P, kin, gen):
    """(scores f32 [P,Bq,kin] descending along kin, idx i64 [P,Bq,kin], distinct inside a list): kin of a query's 2 kin pool ids per list."""
    pick = torch.rand((P, BQ, 2 * kin), device=dev, generator=gen).argsort(dim=-1)[..., :kin]
    base = torch.randint(0, 2 ** 20, (1, BQ, 1), device=dev, generator=gen) * 8192 + 2 ** 32
    s = torch.rand((P, BQ, kin), device=dev, generator=gen).sort(dim=-1, descending=True).values
    return s.contiguous(), (pick + base).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fuse_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("fuse_bench.py measures on the GPU (no CPU path)")
    gen = torch.Generator(device=dev).manual_seed(1)
    med = statistics.median
    rows = []
    for P, kin in SHAPES:
        s, idx = lists_of(P, kin, gen)
        for kw in MODES:
            def fuse():
                return ops.fuse_lists(s, idx, K, **kw)

            def merge():
                return ops.merge_topk(s, idx, K)

            got = fuse()
            torch.cuda.synchronize()
            host = []
            for _ in range(max(1, a.host_reps)):
                t0 = time.perf_counter()
                want = ref_fuse(s.cpu().numpy(), idx.cpu().numpy(), [1.0] * P, kw["mode"], 60.0, kw.get("normalize", "none"), "zero", K)
                host.append((time.perf_counter() - t0) * 1e3)
            same = bool(np.array_equal(got[1].cpu().numpy(), want[1]) and
                        np.array_equal(got[0].cpu().numpy().view(np.int32), want[0].view(np.int32)))
            n = 200
            clock = ClockSampler(dev).start()
            tf, tm = alternate(fuse, merge, n, a.warmup, a.reps)
            clock = clock.stop()
            r = dict(bench="fuse", Bq=BQ, P=P, kin=kin, k=K, mode=kw["mode"], normalize=kw.get("normalize", "none"), fuse_us=med(tf),
                     fuse_us_min_max=[min(tf), max(tf)], merge_us=med(tm), merge_us_min_max=[min(tm), max(tm)], fuse_over_merge=med(tf) / med(tm),
                     host_ms=med(host), host_over_fuse=med(host) * 1e3 / med(tf), launches_per_window=n, reps=a.reps,
                     bitwise_equal_to_restatement=same, sclk_mhz_mean=clock.get("sclk_mhz_mean"))
            print(json.dumps(r), flush=True)
            rows.append(r)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Diffusion re-ranking (cor_rerank_diffusion) against the parent build's cor_diversify_mmr on the same lists. GPU only.
Lists: the top-kin of Bq queries over a 262 144-row gallery at C = 256 (4 look-alikes per object), bf16 and fp32 rows;
kin in {64, 128, 256}, Bq in {32, 512}, kd = 8, kq = kin, gamma = 3, alpha = 0.9, iters = 20, k = kin.
  diffuse_us    cor_rerank_diffusion of this build, called through ctypes, device events around a window of back-to-back calls;
  yardstick_us  cor_diversify_mmr with k = kin, lam = 0.5, max_sim = +inf, called the same way, out of --parent-lib (the parent commit's
                libcor_amd.so loaded beside this one; without the option this build's own copy of that entry point, which
                tools/kernel_disasm_diff.py shows to be the parent's code). It runs about kin^2 / 2 chains per query in kin dependent steps;
                the diffusion runs kin^2 chains (the full square) with no dependency between them, so the expectation to check is
                ratio = diffuse_us / yardstick_us <= 2.
The two sides alternate over --reps windows after --warmup windows in ONE process; medians and min/max are reported with the mean shader
clock of the windows. One JSON line per measurement, printed and appended to --out (default profiles/diffuse_bench.jsonl).
    python tools/diffuse_bench.py [--parent-lib FILE] [--reps 7] [--warmup 2] [--rows 262144] [--out FILE]"""
import argparse, ctypes, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from cor_amd import _native as nat
from cor_amd.retrieval import GalleryShard
from cor_amd.utils import ClockSampler

C = 256
KD, GAMMA, ALPHA, ITERS, LAM = 8, 3, 0.9, 20, 0.5
SHAPES = [(kin, Bq) for kin in (64, 128, 256) for Bq in (32, 512)]
dev = "cuda:0"


def window_us(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, default=262144)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diffuse_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("diffuse_bench.py measures on the GPU (no CPU path)")
    lib = nat.load()
    if a.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(a.parent_lib))
        parent.cor_diversify_mmr.argtypes = nat.SIGNATURES["cor_diversify_mmr"]
        parent.cor_diversify_mmr.restype = ctypes.c_int
    else:
        parent = lib
    gen = torch.Generator(device=dev).manual_seed(1)
    base = torch.nn.functional.normalize(torch.randn((a.rows // 4, C), device=dev, generator=gen), dim=-1)
    G32 = torch.nn.functional.normalize(base.repeat_interleave(4, 0) + 0.3 * torch.randn((a.rows // 4 * 4, C), device=dev, generator=gen) / C ** 0.5, dim=-1)
    del base
    galleries = {"bf16": (G32.to(torch.bfloat16), nat.BF16), "fp32": (G32, nat.F32)}
    Qall = torch.nn.functional.normalize(torch.randn((512, C), device=dev, generator=gen)
                                         + 2.0 * G32[torch.randint(0, G32.shape[0], (512,), device=dev, generator=gen)], dim=-1)
    st = torch.cuda.current_stream().cuda_stream
    med = statistics.median
    rows = []
    for kind, (G, dt) in galleries.items():
        sh = GalleryShard(G)
        seg = ((ctypes.c_void_p * 1)(G.data_ptr()), None, (ctypes.c_longlong * 1)(0), (ctypes.c_int * 1)(G.shape[0]), (ctypes.c_int * 1)(dt))
        for kin, Bq in SHAPES:
            s, idx = sh.search(Qall[:Bq], kin)
            s, idx = s.contiguous(), idx.contiguous()
            out_s = torch.empty((Bq, kin), device=dev)
            out_i = torch.empty((Bq, kin), dtype=torch.int64, device=dev)

            def diffuse():
                rc = lib.cor_rerank_diffusion(*seg, 1, s.data_ptr(), idx.data_ptr(), Bq, kin, C, KD, kin, GAMMA, ALPHA, ITERS, kin, out_s.data_ptr(),
                                              out_i.data_ptr(), None, st)
                assert rc == 0, rc

            def yardstick():
                rc = parent.cor_diversify_mmr(*seg, 1, s.data_ptr(), idx.data_ptr(), Bq, kin, C, LAM, float("inf"), kin, out_s.data_ptr(),
                                              out_i.data_ptr(), None, None, st)
                assert rc == 0, rc

            diffuse(); yardstick()
            torch.cuda.synchronize()
            n = max(5, min(400, int(6e7 / (Bq * kin * kin))))        # windows of a few ms
            for _ in range(a.warmup):
                window_us(diffuse, n); window_us(yardstick, n)
            clock = ClockSampler(dev).start()
            td, ty = [], []
            for _ in range(a.reps):
                td.append(window_us(diffuse, n)); ty.append(window_us(yardstick, n))
            clock = clock.stop()
            r = dict(bench="diffuse", rows=G.shape[0], gallery=kind, C=C, Bq=Bq, kin=kin, kd=KD, gamma=GAMMA, alpha=ALPHA, iters=ITERS, k=kin,
                     diffuse_us=med(td), diffuse_us_min_max=[min(td), max(td)], yardstick_us=med(ty), yardstick_us_min_max=[min(ty), max(ty)],
                     ratio=med(td) / med(ty), yardstick="parent library" if a.parent_lib else "this build's cor_diversify_mmr",
                     chains_per_query=kin * kin, launches_per_window=n, reps=a.reps, sclk_mhz_mean=clock.get("sclk_mhz_mean"))
            print(json.dumps(r), flush=True)
            rows.append(r)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

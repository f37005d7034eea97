#!/usr/bin/env python3
"""Result diversification (ops.diversify_mmr) against what a user writes today and against the bytes it must move. GPU only.
512 queries, lists out of a 1M-row bf16 gallery at C = 256 (the search's top-kin; for kin = 1024 the list is filled up with random other
rows and their scores, sorted: the search stops at k = 256), (kin, k) in {(100, 10), (256, 10), (256, 50), (1024, 50)}, lam = 0.5, no
suppression.
  kernel_us    ops.diversify_mmr, device events around a window of back-to-back calls;
  torch_us     yardstick 1, the same device, the same window: R = rows[idx] widened to fp32, the [Bq, kin, kin] Gram matrix by torch.bmm,
               then k dependent steps of lam * s - (1 - lam) * m over the alive entries, argmax, gather of the winner's Gram column, maximum;
  floor_us     yardstick 2: the row bytes the k similarity passes read, k * kin * C * 2 per query, over the measured copy bandwidth of the
               project (6.29 TB/s); kernel_over_floor = kernel_us / floor_us. (The rows of one query fit in L2, so HBM sees
               them once; the floor is what the passes pull through the memory pipeline.)
The two timed sides alternate over --reps windows after --warmup windows; medians and min/max are reported, with the share of output ids
the two sides agree on (the torch side's Gram is a plain fp32 matmul, not the chain, and its argmax breaks ties by position: near-ties
may flip, so the share is reported, not asserted). One JSON line per measurement, printed and appended to --out (default
profiles/diversify_bench.jsonl).
    python tools/diversify_bench.py [--reps 7] [--warmup 2] [--rows 1000000] [--out FILE]"""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from cor_amd import ops
from cor_amd.retrieval import GalleryShard
from cor_amd.utils import ClockSampler

COPY_TBS = 6.29          # measured float4 copy bandwidth, TB/s
C, BQ, LAM = 256, 512, 0.5
SHAPES = ((100, 10), (256, 10), (256, 50), (1024, 50))
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


def lists_of(sh, Q, kin, gen):
    """(scores f32 [Bq,kin] descending, idx i64 [Bq,kin], ids pairwise different): the search's list, filled up past 256 with random rows."""
    s, i = sh.search(Q, min(kin, 256))
    if kin <= 256:
        return s.contiguous(), i.contiguous()
    n = len(sh)
    extra = torch.randint(0, n, (Q.shape[0], 2 * (kin - 256)), device=dev, generator=gen)
    fresh = (extra[:, :, None] != i[:, None, :]).all(-1)                       # not in the top-256 ..
    order = torch.sort(extra, dim=1)
    first = torch.ones_like(fresh)
    first[:, 1:] = order.values[:, 1:] != order.values[:, :-1]                 # .. and not drawn twice
    fresh &= torch.zeros_like(fresh).scatter_(1, order.indices, first)
    pick = torch.sort((~fresh).to(torch.int8), dim=1, stable=True).indices[:, :kin - 256]
    assert bool(fresh.sum(1).min() >= kin - 256)
    extra = extra.gather(1, pick)
    es = torch.einsum("bkc,bc->bk", sh.rows[extra].float(), Q)
    es, o = torch.sort(es, dim=1, descending=True)
    return torch.cat([s, torch.minimum(es, s[:, -1:])], 1).contiguous(), torch.cat([i, extra.gather(1, o)], 1).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diversify_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("diversify_bench.py measures on the GPU (no CPU path)")
    gen = torch.Generator(device=dev).manual_seed(1)
    # 4 look-alikes per object, so that the penalty has something to do
    base = torch.nn.functional.normalize(torch.randn((a.rows // 4, C), device=dev, generator=gen), dim=-1)
    G = torch.nn.functional.normalize(base.repeat_interleave(4, 0) + 0.3 * torch.randn((a.rows // 4 * 4, C), device=dev, generator=gen) / C ** 0.5,
                                      dim=-1).to(torch.bfloat16)
    del base
    sh = GalleryShard(G)
    Q = torch.nn.functional.normalize(torch.randn((BQ, C), device=dev, generator=gen) + 2.0 * G[torch.randint(0, len(sh), (BQ,), device=dev, generator=gen)].float(),
                                      dim=-1)
    med = statistics.median
    rows = []
    lists = {}
    for kin, k in SHAPES:
        if kin not in lists:
            lists[kin] = lists_of(sh, Q, kin, gen)
        s, idx = lists[kin]
        ar = torch.arange(BQ, device=dev)

        def kernel():
            return ops.diversify_mmr([(G, 0)], s, idx, k, lam=LAM)

        def eager():
            R = G[idx].float()                                                # [Bq, kin, C]
            gram = torch.bmm(R, R.transpose(1, 2))                            # [Bq, kin, kin]
            m = torch.zeros_like(s)
            alive = torch.ones_like(s, dtype=torch.bool)
            out_s, out_i = torch.empty((BQ, k), device=dev), torch.empty((BQ, k), dtype=torch.int64, device=dev)
            for t in range(k):
                f = torch.where(alive, LAM * s - (1.0 - LAM) * m, torch.full_like(s, float("-inf")))
                w = f.argmax(1)
                out_s[:, t], out_i[:, t] = s[ar, w], idx[ar, w]
                alive[ar, w] = False
                m = torch.maximum(m, gram[ar, :, w])
            return out_s, out_i

        k_out, e_out = kernel(), eager()
        torch.cuda.synchronize()
        agree = float((k_out[1] == e_out[1]).float().mean())
        same_lists = float((k_out[1] == e_out[1]).all(1).float().mean())
        n_k = max(5, min(1000, int(4e7 / (BQ * kin * k))))      # windows of a few ms
        n_e = max(3, n_k // 8)
        clock = ClockSampler(dev).start()
        tk, te = alternate(kernel, eager, n_k, n_e, a.warmup, a.reps)
        clock = clock.stop()
        nbytes = BQ * k * kin * C * 2
        floor = nbytes / (COPY_TBS * 1e12) * 1e6
        r = dict(bench="diversify", rows=len(sh), gallery="bf16", C=C, Bq=BQ, kin=kin, k=k, lam=LAM, kernel_us=med(tk), kernel_us_min_max=[min(tk), max(tk)],
                 torch_us=med(te), torch_us_min_max=[min(te), max(te)], torch_over_kernel=med(te) / med(tk), pass_bytes=nbytes, floor_us=floor,
                 kernel_over_floor=med(tk) / floor, launches_per_window=[n_k, n_e], reps=a.reps, ids_agreeing_with_torch=agree,
                 lists_agreeing_with_torch=same_lists, sclk_mhz_mean=clock.get("sclk_mhz_mean"))
        print(json.dumps(r), flush=True)
        rows.append(r)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""k-reciprocal re-ranking (ops.rerank_reciprocal) against what a user writes today and against the bytes it must move, and the cost of
building a neighbour graph. GPU only.
Re-ranking: 512 queries, lists out of a 1M-row bf16 gallery at C = 256 (the search's top-256; for kin = 1024 the list is filled up with
random other rows and their scores, sorted: the search stops at k = 256), a synthetic graph of width 20 over the 1M rows (random ids, about
a third of the slots -1, kth chosen so that about half of the first k1 entries enter A), kin in {100, 256, 1024}, k1 = 20, k = 10, lam = 0.3.
  kernel_us    ops.rerank_reciprocal, device events around a window of back-to-back calls;
  torch_us     yardstick 1, the same device, the same window: R = rnbr[idx]; the [Bq, kin, kg, k1] comparison against the query's set, sums,
               J, lam * s + (1 - lam) * J, torch.sort (stable, so equal f keep the list order instead of the id order);
  floor_us     yardstick 2: the bytes the call must gather (kin * kg * 8 per query) over the measured copy bandwidth of the project
               (6.29 TB/s); kernel_over_floor = kernel_us / floor_us.
The two timed sides alternate over --reps windows after --warmup windows; medians and min/max are reported, with the share of output ids the
two sides agree on. Graph build: GalleryShard.neighbour_graph(20) over --graph-rows rows (default 100k, bf16), once after one warm-up, beside
the plain search loop it consists of and the pruning launch alone. One JSON line per measurement, printed and appended to --out (default
profiles/rerank_bench.jsonl).
    python tools/rerank_bench.py [--reps 7] [--warmup 2] [--rows 1000000] [--graph-rows 100000] [--out FILE]"""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from cor_amd import ops
from cor_amd.retrieval import GalleryShard
from cor_amd.utils import ClockSampler

COPY_TBS = 6.29          # measured float4 copy bandwidth, TB/s
C, BQ, KG, K1, K, LAM = 256, 512, 20, 20, 10, 0.3
KINS = (100, 256, 1024)
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
    ap.add_argument("--graph-rows", type=int, default=100_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rerank_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("rerank_bench.py measures on the GPU (no CPU path)")
    gen = torch.Generator(device=dev).manual_seed(1)
    G = torch.nn.functional.normalize(torch.randn((a.rows, C), device=dev, generator=gen), dim=-1).to(torch.bfloat16)
    sh = GalleryShard(G)
    Q = torch.nn.functional.normalize(torch.randn((BQ, C), device=dev, generator=gen), dim=-1)
    rnbr = torch.randint(0, a.rows, (a.rows, KG), device=dev, generator=gen)
    rnbr[torch.rand((a.rows, KG), device=dev, generator=gen) < 0.3] = -1
    kth = (torch.rand((a.rows,), device=dev, generator=gen) >= 0.5).float() * 2.0          # half of the rows count any query among their nearest
    segs = [(rnbr, kth, 0)]
    med = statistics.median
    rows = []
    for kin in KINS:
        s, idx = lists_of(sh, Q, kin, gen)

        def kernel():
            return ops.rerank_reciprocal(s, idx, segs, K1, LAM, K)

        def eager():
            R = rnbr[idx]                                                     # [Bq, kin, kg]
            head = idx[:, :K1]
            in_a = s[:, :K1] >= kth[head]
            A = torch.where(in_a, head, torch.full_like(head, -2))            # [Bq, k1]
            valid = R >= 0
            I = ((R[:, :, :, None] == A[:, None, None, :]).any(-1) & valid).sum(-1)
            U = in_a.sum(1, keepdim=True) + valid.sum(-1) - I
            J = torch.where(U > 0, I.float() / U.float(), torch.zeros((), device=dev))
            f, o = torch.sort(LAM * s + (1.0 - LAM) * J, dim=1, descending=True, stable=True)
            return f[:, :K], idx.gather(1, o[:, :K])

        k_out, e_out = kernel(), eager()
        torch.cuda.synchronize()
        agree = float((k_out[1] == e_out[1]).float().mean())
        diff = float((k_out[0] - e_out[0]).abs().max())
        n_k = max(10, min(2000, int(2e6 / (BQ * kin))))         # windows of a few ms
        n_e = max(3, n_k // 8)
        clock = ClockSampler(dev).start()
        tk, te = alternate(kernel, eager, n_k, n_e, a.warmup, a.reps)
        clock = clock.stop()
        nbytes = BQ * kin * KG * 8
        floor = nbytes / (COPY_TBS * 1e12) * 1e6
        r = dict(bench="rerank", rows=a.rows, Bq=BQ, kin=kin, kg=KG, k1=K1, k=K, lam=LAM, kernel_us=med(tk), kernel_us_min_max=[min(tk), max(tk)],
                 torch_us=med(te), torch_us_min_max=[min(te), max(te)], torch_over_kernel=med(te) / med(tk), gather_bytes=nbytes, floor_us=floor,
                 kernel_over_floor=med(tk) / floor, launches_per_window=[n_k, n_e], reps=a.reps, ids_agreeing_with_torch=agree,
                 max_abs_score_diff_to_torch=diff, sclk_mhz_mean=clock.get("sclk_mhz_mean"))
        print(json.dumps(r), flush=True)
        rows.append(r)

    # the graph build, once: the search loop it consists of, the pruning launch, and the whole
    gsh = GalleryShard(G[:a.graph_rows].clone())

    def searches():
        out = None
        for lo in range(0, len(gsh), 4096):
            out = gsh.search(gsh.rows[lo:lo + 4096], K1)
        return out

    searches(); graph = gsh.neighbour_graph(K1)                 # warm-up
    nbr = torch.cat([gsh.search(gsh.rows[lo:lo + 4096], K1)[1] for lo in range(0, len(gsh), 4096)])
    torch.cuda.synchronize()
    clock = ClockSampler(dev).start()
    t_search = window_us(searches, 1)
    t_graph = window_us(lambda: gsh.neighbour_graph(K1), 1)
    t_prune = window_us(lambda: ops.knn_reciprocal([(nbr, 0)], 0), 1)
    clock = clock.stop()
    r = dict(bench="neighbour_graph", rows=a.graph_rows, C=C, k1=K1, batch=4096, gallery="bf16", graph_build_ms=t_graph / 1e3, search_loop_ms=t_search / 1e3,
             prune_ms=t_prune / 1e3, reciprocal_share=float((graph.rnbr[0] >= 0).float().mean()), sclk_mhz_mean=clock.get("sclk_mhz_mean"))
    print(json.dumps(r), flush=True)
    rows.append(r)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

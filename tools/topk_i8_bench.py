#!/usr/bin/env python3
"""Int8 gallery search (ops.similarity_topk_i8) beside the bf16 call it is meant to undercut, on one box in one process. GPU only.
Per shape (C = 256): the int8 call and the bf16 ops.similarity_topk call alternate over --reps windows of back-to-back calls after --warmup
windows (device events around each window; medians and min / max reported), then two_stage_search over fp32 master rows with the int8 and
with the bf16 coarse stage alternate the same way (k_coarse = max(k, 100), final k = 10). The quantisation of the 1M-row gallery is timed
once. The mean shader clock over each measurement is reported. One JSON line per measurement, printed and appended to --out (default
profiles/topk_i8_bench.jsonl).
    python tools/topk_i8_bench.py [--reps 7] [--warmup 2] [--out FILE]
    python tools/topk_i8_bench.py --one 512x1000000 10        # the int8 call alone, 20 calls (for a rocprofv3 --kernel-trace --stats run)
--filtered: the filtered int8 call (ops.similarity_topk_i8_filtered's entry point) instead, appended to profiles/topk_i8_filtered_bench.jsonl.
Per shape and label layout ("ne": image ids in runs of 1-8 rows, every query excludes its own image; "eq": 16 uniformly random classes) three
sides rotate, each through the C entry point with preallocated outputs and workspace: the new call, (a) cor_similarity_topk_filtered over
the bf16 copy of the same rows with the same labels, (b) the unfiltered cor_similarity_topk_i8. Then (c) two_stage_search (k_coarse = 100,
k = 10, fp32 master rows) with the int8 and with the bf16 coarse stage alternate, both filtered.
    python tools/topk_i8_bench.py --filtered [--reps 7] [--warmup 2] [--out FILE]
    python tools/topk_i8_bench.py --filtered --one 512x1000000 10 [--layout ne|eq]
--distinct: the distinct-group int8 call (ops.similarity_topk_i8_distinct's entry point), appended to profiles/topk_i8_distinct_bench.jsonl.
Shapes 512x1M, 512x125k and 32x100k at k = 10 and k = 100; groups = image ids in runs of 1-8 rows, unfiltered ("none") and with every query
excluding its own image through the same tensor ("ne"). Three sides rotate through the C entry points as above: the new call, (a)
cor_similarity_topk_distinct over the bf16 copy with the same groups, (b) the unfiltered cor_similarity_topk_i8 at the same k. Then
two_stage_search (k_coarse = 100, k = 10, fp32 master rows, distinct) with the int8 and with the bf16 coarse stage alternate.
    python tools/topk_i8_bench.py --distinct [--reps 7] [--warmup 2] [--out FILE]
    python tools/topk_i8_bench.py --distinct --one 512x1000000 10 [--layout ne|none]"""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from cor_amd import ops, _native as nat
from cor_amd.retrieval import GalleryShard, QuantizedShard, two_stage_search
from cor_amd.utils import ClockSampler

C = 256
CASES = ((512, 1_000_000, 10), (512, 1_000_000, 100), (512, 125_000, 10), (32, 100_000, 100))
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


def rotate(fns, n, warmup, reps):
    """alternate() for any number of sides"""
    for _ in range(warmup):
        for f in fns:
            window_us(f, n)
    ts = [[] for _ in fns]
    for _ in range(reps):
        for t, f in zip(ts, fns):
            t.append(window_us(f, n))
    return ts


def labels(layout, Bq, Ng):
    """(row labels i32[Ng], query labels i32[Bq], mode) on the device. ne: image ids in runs of 1-8 rows, query b is a region of the image
    of row b * Ng // Bq and excludes it; eq: 16 uniformly random classes, a random class per query."""
    g = torch.Generator(device=dev).manual_seed(Bq * 3 + Ng)
    if layout == "ne":
        runs = torch.randint(1, 9, (Ng,), device=dev, generator=g)
        rl = torch.repeat_interleave(torch.arange(Ng, device=dev), runs)[:Ng].to(torch.int32).contiguous()
        return rl, rl[(torch.arange(Bq, device=dev) * Ng) // Bq].contiguous(), "ne"
    rl = torch.randint(0, 16, (Ng,), device=dev, generator=g).to(torch.int32)
    return rl, torch.randint(0, 16, (Bq,), device=dev, generator=g).to(torch.int32), "eq"


def direct_calls(Q, Gb, q, sc, rl, ql, mode, k):
    """the three sides as closures over preallocated buffers: (int8 filtered, bf16 filtered, int8 unfiltered), and the int8 filtered outputs"""
    lib, st = nat.load(), torch.cuda.current_stream().cuda_stream
    Bq, Ng, m = Q.shape[0], q.shape[0], ops._FILTER_MODES[mode]
    w8f, s8f, i8f = ops._topk_buffers("cor_topk_i8_filtered_workspace_bytes", Q, Bq, Ng, k)
    wbf, sbf, ibf = ops._topk_buffers("cor_topk_filtered_workspace_bytes", Q, Bq, Ng, k)
    w8, s8, i8 = ops._topk_buffers("cor_topk_i8_workspace_bytes", Q, Bq, Ng, k)

    def i8_filtered(flags=0):
        nat.check(lib.cor_similarity_topk_i8_filtered(Q.data_ptr(), q.data_ptr(), sc.data_ptr(), Bq, Ng, C, k, 0, rl.data_ptr(), ql.data_ptr(), m,
                                                      s8f.data_ptr(), i8f.data_ptr(), w8f.data_ptr(), flags, st), "cor_similarity_topk_i8_filtered")

    def bf16_filtered():
        nat.check(lib.cor_similarity_topk_filtered(Q.data_ptr(), Gb.data_ptr(), nat.BF16, Bq, Ng, C, k, 0, rl.data_ptr(), ql.data_ptr(), m,
                                                   sbf.data_ptr(), ibf.data_ptr(), wbf.data_ptr(), 0, st), "cor_similarity_topk_filtered")

    def i8_plain():
        nat.check(lib.cor_similarity_topk_i8(Q.data_ptr(), q.data_ptr(), sc.data_ptr(), Bq, Ng, C, k, 0, s8.data_ptr(), i8.data_ptr(), w8.data_ptr(),
                                             0, st), "cor_similarity_topk_i8")

    return i8_filtered, bf16_filtered, i8_plain, (s8f, i8f)


def filtered_main(a):
    med = statistics.median
    if a.one:
        Bq, Ng = (int(v) for v in a.one[0].split("x"))
        Q, G = data(Bq, Ng)
        q, sc = ops.quantize_rows_i8(G)
        rl, ql, mode = labels(a.layout, Bq, Ng)
        f = direct_calls(Q, None, q, sc, rl, ql, mode, int(a.one[1]))[0]
        for _ in range(20):
            f()
        torch.cuda.synchronize()
        return
    rows, cache = [], {}
    for Bq, Ng, k in CASES:
        if (Bq, Ng) not in cache:
            cache.clear()
            Q, G = data(Bq, Ng)
            cache[(Bq, Ng)] = (Q, G, G.to(torch.bfloat16)) + ops.quantize_rows_i8(G)
        Q, G, Gb, q, sc = cache[(Bq, Ng)]
        n = max(5, min(200, int(2e9 / (Bq * Ng))))                                         # windows of a few ms
        for layout in ("ne", "eq"):
            rl, ql, mode = labels(layout, Bq, Ng)
            f8, fb, fp, (s8f, i8f) = direct_calls(Q, Gb, q, sc, rl, ql, mode, k)
            f8(nat.TOPK_NO_FALLBACK)
            overflowed = int((i8f == -2).any(dim=1).sum())
            f8()
            ok = (rl[i8f.clamp(min=0)] == ql[:, None]) == (mode == "eq")                   # every returned row is an allowed one
            clock = ClockSampler(dev).start()
            t8, tb, tp = rotate((f8, fb, fp), n, a.warmup, a.reps)
            clock = clock.stop()
            rows.append(dict(bench="topk_i8_filtered", layout=layout, mode=mode, Bq=Bq, Ng=Ng, C=C, k=k, i8_filtered_us=med(t8),
                             i8_filtered_us_min_max=[min(t8), max(t8)], bf16_filtered_us=med(tb), bf16_filtered_us_min_max=[min(tb), max(tb)],
                             i8_unfiltered_us=med(tp), i8_unfiltered_us_min_max=[min(tp), max(tp)], bf16_filtered_over_i8_filtered=med(tb) / med(t8),
                             i8_filtered_over_i8_unfiltered=med(t8) / med(tp), calls_per_window=n, reps=a.reps, queries_overflowed=overflowed,
                             rows_allowed=bool((ok | (i8f < 0)).all()), sclk_mhz_mean=clock.get("sclk_mhz_mean")))
            print(json.dumps(rows[-1]), flush=True)
            if k != 10:
                continue
            fine, c8, cb = GalleryShard(G), QuantizedShard(q, sc, labels=rl), GalleryShard(Gb, labels=rl)
            kw = dict(query_labels=ql, mode=mode)
            clock = ClockSampler(dev).start()
            t8, tb = alternate(lambda: two_stage_search(Q, c8, fine, 10, 100, **kw), lambda: two_stage_search(Q, cb, fine, 10, 100, **kw), n,
                               a.warmup, a.reps)
            clock = clock.stop()
            rows.append(dict(bench="two_stage_filtered", layout=layout, mode=mode, Bq=Bq, Ng=Ng, C=C, k=10, k_coarse=100, i8_coarse_us=med(t8),
                             i8_coarse_us_min_max=[min(t8), max(t8)], bf16_coarse_us=med(tb), bf16_coarse_us_min_max=[min(tb), max(tb)],
                             bf16_over_i8=med(tb) / med(t8), calls_per_window=n, reps=a.reps, sclk_mhz_mean=clock.get("sclk_mhz_mean")))
            print(json.dumps(rows[-1]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


DISTINCT_CASES = tuple((Bq, Ng, k) for Bq, Ng in ((512, 1_000_000), (512, 125_000), (32, 100_000)) for k in (10, 100))


def distinct_calls(Q, Gb, q, sc, rg, ql, k):
    """the three sides as closures over preallocated buffers: (int8 distinct, bf16 distinct, int8 plain), and the int8 distinct outputs.
    ql None: unfiltered; else "ne" with the group tensor as the row labels"""
    lib, st = nat.load(), torch.cuda.current_stream().cuda_stream
    Bq, Ng = Q.shape[0], q.shape[0]
    rl, qlp, m = (rg.data_ptr(), ql.data_ptr(), nat.FILTER_NE) if ql is not None else (None, None, nat.FILTER_EQ)
    w8d, s8d, i8d = ops._topk_buffers("cor_topk_i8_distinct_workspace_bytes", Q, Bq, Ng, k)
    wbd, sbd, ibd = ops._topk_buffers("cor_topk_distinct_workspace_bytes", Q, Bq, Ng, k)
    w8, s8, i8 = ops._topk_buffers("cor_topk_i8_workspace_bytes", Q, Bq, Ng, k)

    def i8_distinct(flags=0):
        nat.check(lib.cor_similarity_topk_i8_distinct(Q.data_ptr(), q.data_ptr(), sc.data_ptr(), Bq, Ng, C, k, 0, rg.data_ptr(), rl, qlp, m,
                                                      s8d.data_ptr(), i8d.data_ptr(), w8d.data_ptr(), flags, st), "cor_similarity_topk_i8_distinct")

    def bf16_distinct():
        nat.check(lib.cor_similarity_topk_distinct(Q.data_ptr(), Gb.data_ptr(), nat.BF16, Bq, Ng, C, k, 0, rg.data_ptr(), rl, qlp, m,
                                                   sbd.data_ptr(), ibd.data_ptr(), wbd.data_ptr(), 0, st), "cor_similarity_topk_distinct")

    def i8_plain():
        nat.check(lib.cor_similarity_topk_i8(Q.data_ptr(), q.data_ptr(), sc.data_ptr(), Bq, Ng, C, k, 0, s8.data_ptr(), i8.data_ptr(), w8.data_ptr(),
                                             0, st), "cor_similarity_topk_i8")

    return i8_distinct, bf16_distinct, i8_plain, (s8d, i8d)


def distinct_main(a):
    med = statistics.median
    if a.one:
        Bq, Ng = (int(v) for v in a.one[0].split("x"))
        Q, G = data(Bq, Ng)
        q, sc = ops.quantize_rows_i8(G)
        rg, ql, _ = labels("ne", Bq, Ng)
        f = distinct_calls(Q, None, q, sc, rg, ql if a.layout == "ne" else None, int(a.one[1]))[0]
        for _ in range(20):
            f()
        torch.cuda.synchronize()
        return
    rows, cache = [], {}
    for Bq, Ng, k in DISTINCT_CASES:
        if (Bq, Ng) not in cache:
            cache.clear()
            Q, G = data(Bq, Ng)
            cache[(Bq, Ng)] = (Q, G, G.to(torch.bfloat16)) + ops.quantize_rows_i8(G)
        Q, G, Gb, q, sc = cache[(Bq, Ng)]
        n = max(5, min(200, int(2e9 / (Bq * Ng))))                                         # windows of a few ms
        rg, own, _ = labels("ne", Bq, Ng)                                                  # image ids in runs of 1-8 rows; the queries' own images
        for layout, ql in (("none", None), ("ne", own)):
            f8, fb, fp, (s8d, i8d) = distinct_calls(Q, Gb, q, sc, rg, ql, k)
            f8(nat.TOPK_NO_FALLBACK)
            overflowed = int((i8d == -2).any(dim=1).sum())
            f8()
            img = rg[i8d.clamp(min=0)].sort(dim=1).values
            distinct = bool((img[:, 1:] != img[:, :-1]).all()) and bool((i8d >= 0).all())  # k different images per query
            allowed = ql is None or bool((rg[i8d.clamp(min=0)] != ql[:, None]).all())
            clock = ClockSampler(dev).start()
            t8, tb, tp = rotate((f8, fb, fp), n, a.warmup, a.reps)
            clock = clock.stop()
            rows.append(dict(bench="topk_i8_distinct", layout=layout, groups="runs", Bq=Bq, Ng=Ng, C=C, k=k, i8_distinct_us=med(t8),
                             i8_distinct_us_min_max=[min(t8), max(t8)], bf16_distinct_us=med(tb), bf16_distinct_us_min_max=[min(tb), max(tb)],
                             i8_plain_us=med(tp), i8_plain_us_min_max=[min(tp), max(tp)], bf16_distinct_over_i8_distinct=med(tb) / med(t8),
                             i8_distinct_over_i8_plain=med(t8) / med(tp), calls_per_window=n, reps=a.reps, queries_overflowed=overflowed,
                             groups_distinct=distinct, rows_allowed=allowed, sclk_mhz_mean=clock.get("sclk_mhz_mean")))
            print(json.dumps(rows[-1]), flush=True)
            if k != 10:
                continue
            fine, c8, cb = GalleryShard(G, groups=rg), QuantizedShard(q, sc, labels=rg, groups=rg), GalleryShard(Gb, labels=rg, groups=rg)
            kw = dict(distinct=True) if ql is None else dict(query_labels=ql, mode="ne", distinct=True)
            clock = ClockSampler(dev).start()
            t8, tb = alternate(lambda: two_stage_search(Q, c8, fine, 10, 100, **kw), lambda: two_stage_search(Q, cb, fine, 10, 100, **kw), n,
                               a.warmup, a.reps)
            clock = clock.stop()
            rows.append(dict(bench="two_stage_distinct", layout=layout, groups="runs", Bq=Bq, Ng=Ng, C=C, k=10, k_coarse=100, i8_coarse_us=med(t8),
                             i8_coarse_us_min_max=[min(t8), max(t8)], bf16_coarse_us=med(tb), bf16_coarse_us_min_max=[min(tb), max(tb)],
                             bf16_over_i8=med(tb) / med(t8), calls_per_window=n, reps=a.reps, sclk_mhz_mean=clock.get("sclk_mhz_mean")))
            print(json.dumps(rows[-1]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


def data(Bq, Ng):
    g = torch.Generator(device=dev).manual_seed(Bq + Ng)
    Q = torch.nn.functional.normalize(torch.randn((Bq, C), device=dev, generator=g), dim=-1)
    G = torch.nn.functional.normalize(torch.randn((Ng, C), device=dev, generator=g), dim=-1)
    return Q, G


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out")
    ap.add_argument("--one", nargs=2, metavar=("BQxNG", "K"))
    ap.add_argument("--filtered", action="store_true")
    ap.add_argument("--distinct", action="store_true")
    ap.add_argument("--layout", choices=("ne", "eq", "none"), default="ne")
    a = ap.parse_args()
    name = "topk_i8_distinct_bench.jsonl" if a.distinct else "topk_i8_filtered_bench.jsonl" if a.filtered else "topk_i8_bench.jsonl"
    a.out = a.out or os.path.join(ROOT, "profiles", name)
    if not torch.cuda.is_available():
        raise RuntimeError("topk_i8_bench.py measures on the GPU (no CPU path)")
    if a.distinct:
        return distinct_main(a)
    if a.filtered:
        return filtered_main(a)
    if a.one:
        Bq, Ng = (int(v) for v in a.one[0].split("x"))
        Q, G = data(Bq, Ng)
        q, sc = ops.quantize_rows_i8(G)
        for _ in range(20):
            ops.similarity_topk_i8(Q, q, sc, int(a.one[1]))
        torch.cuda.synchronize()
        return
    med = statistics.median
    rows, cache = [], {}
    for Bq, Ng, k in CASES:
        if (Bq, Ng) not in cache:
            cache.clear()
            Q, G = data(Bq, Ng)
            q, sc = ops.quantize_rows_i8(G)
            if Ng == 1_000_000:
                for _ in range(2):
                    ops.quantize_rows_i8(G)
                rows.append(dict(bench="quantize_rows_i8", rows=Ng, C=C, src="torch.float32", us=window_us(lambda: ops.quantize_rows_i8(G), 5)))
                print(json.dumps(rows[-1]), flush=True)
            cache[(Bq, Ng)] = (Q, G, G.to(torch.bfloat16), q, sc)
        Q, G, Gb, q, sc = cache[(Bq, Ng)]
        _, raw = ops.similarity_topk_i8(Q, q, sc, k, flags=nat.TOPK_NO_FALLBACK)
        _, fi = ops.similarity_topk(Q, G, k)
        _, ii = ops.similarity_topk_i8(Q, q, sc, k)
        overlap = float((ii[:, :, None] == fi[:, None, :]).any(-1).float().mean())       # share of the fp32 top-k the int8 top-k holds
        n = max(5, min(200, int(2e9 / (Bq * Ng))))                                         # windows of a few ms
        clock = ClockSampler(dev).start()
        t8, tb = alternate(lambda: ops.similarity_topk_i8(Q, q, sc, k), lambda: ops.similarity_topk(Q, Gb, k), n, a.warmup, a.reps)
        clock = clock.stop()
        rows.append(dict(bench="topk_i8", Bq=Bq, Ng=Ng, C=C, k=k, i8_us=med(t8), i8_us_min_max=[min(t8), max(t8)], bf16_us=med(tb),
                         bf16_us_min_max=[min(tb), max(tb)], bf16_over_i8=med(tb) / med(t8), calls_per_window=n, reps=a.reps,
                         queries_overflowed=int((raw == -2).any(dim=1).sum()), overlap_with_fp32_topk=overlap,
                         sclk_mhz_mean=clock.get("sclk_mhz_mean")))
        print(json.dumps(rows[-1]), flush=True)
        fine, c8, cb = GalleryShard(G), QuantizedShard(q, sc), GalleryShard(Gb)
        kc = max(k, 100)
        want = fine.search(Q, 10)[1]
        hit8 = float((two_stage_search(Q, c8, fine, 10, kc)[1] == want).all(1).float().mean())
        hitb = float((two_stage_search(Q, cb, fine, 10, kc)[1] == want).all(1).float().mean())
        clock = ClockSampler(dev).start()
        t8, tb = alternate(lambda: two_stage_search(Q, c8, fine, 10, kc), lambda: two_stage_search(Q, cb, fine, 10, kc), n, a.warmup, a.reps)
        clock = clock.stop()
        rows.append(dict(bench="two_stage", Bq=Bq, Ng=Ng, C=C, k=10, k_coarse=kc, i8_coarse_us=med(t8), i8_coarse_us_min_max=[min(t8), max(t8)],
                         bf16_coarse_us=med(tb), bf16_coarse_us_min_max=[min(tb), max(tb)], bf16_over_i8=med(tb) / med(t8),
                         queries_equal_to_fp32_top10=dict(i8=hit8, bf16=hitb), calls_per_window=n, reps=a.reps,
                         sclk_mhz_mean=clock.get("sclk_mhz_mean")))
        print(json.dumps(rows[-1]), flush=True)
    with open(a.out, "a") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

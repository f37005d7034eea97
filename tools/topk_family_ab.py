#!/usr/bin/env python3
"""Same-process A/B between ANOTHER build of the library (the parent commit's libcor_amd.so) and this one, for changes that must leave
results and speed as they are. Three case tables: `topk`, the wide top-k family (similarity_topk at k > 32, _filtered `ne`, _distinct, and the
same three over an int8 gallery, quantised once and shared by both builds), `lists`, the list kernels (cor_merge_topk, cor_rescore_topk,
cor_rescore_topk_i8, cor_rerank_reciprocal, cor_knn_reciprocal, cor_expand_queries) at the shapes of their own bench tools, and `rows`, the
calls that read gallery rows through a segment table (cor_diversify_mmr, cor_rerank_diffusion, cor_kmeans_seed, cor_kmeans_update,
cor_expand_queries_sq, cor_ivf_build) at their bench tools' shapes scaled to seconds, each over a table of one storage dtype (bf16) and over
an fp32 + bf16 + int8 table (cor_ivf_build, which copies rows and takes one dtype only: int8 instead), and the lane-loader calls also over
fp32, fp32 + bf16 (cor_expand_queries) and int8 tables, so that every instantiation of their kernels is launched.
    python tools/topk_family_ab.py PARENT_LIB.so [ROUNDS=5] [OUT=profiles/topk_family_ab.jsonl] [TABLE=topk]
"This one" is the library cor_amd loads (COR_AMD_LIB selects another build of it).
Both sides are called through ctypes with preallocated outputs and workspace, so they carry the same host work. Per case: the results of
the two builds must be bitwise equal (every output), then ROUNDS rounds alternate parent / new; a round is one window of >= 50 ms
(at least 20 calls, HIP events on the launch stream) after warm-up. The yardstick is the parent's own round-to-round spread: the run
fails if a case's new median exceeds the parent median by more than the parent's (max - min). One JSON line per case; OUT is written
afresh by every run, so it holds one run."""
import ctypes as C
import json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from cor_amd import _native as nat
dev = "cuda:0"
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "topk_family_ab.jsonl")
TABLE = sys.argv[4] if len(sys.argv) > 4 else "topk"
DT = {torch.float32: nat.F32, torch.bfloat16: nat.BF16, torch.float16: nat.F16}

new = nat.load()
parent = C.CDLL(os.path.abspath(sys.argv[1]))
for name, sig in nat.SIGNATURES.items():
    if hasattr(parent, name):
        getattr(parent, name).argtypes = sig
        getattr(parent, name).restype = C.c_long if name.endswith("_bytes") else C.c_int


def quantized(G):
    """(Gq int8 [Ng,C], gscale f32 [Ng]) of G by this build's cor_quantize_rows_i8: one copy, searched by both builds"""
    Gq, gs = torch.empty(G.shape, dtype=torch.int8, device=dev), torch.empty((G.shape[0],), device=dev)
    rc = new.cor_quantize_rows_i8(G.data_ptr(), DT[G.dtype], G.shape[0], G.shape[1], Gq.data_ptr(), gs.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    return Gq, gs


def caller(lib, route, Q, G, k, groups, own, G8=None):
    """(fn, scores, idx): fn() enqueues one search of `route` on the current stream; the i8_ routes search G8 = quantized(G)"""
    Bq, Ng, Cc = Q.shape[0], G.shape[0], Q.shape[1]
    i8, kind = route.startswith("i8"), route.removeprefix("i8_").replace("i8", "wide")
    infix = ("i8_" if i8 else "") + {"wide": "", "filtered_ne": "filtered_", "distinct": "distinct_"}[kind]
    ws = torch.empty((getattr(lib, f"cor_topk_{infix}workspace_bytes")(Bq, Ng, k),), dtype=torch.uint8, device=dev)
    s, i = torch.empty((Bq, k), device=dev), torch.empty((Bq, k), dtype=torch.int64, device=dev)
    rows = (G8[0].data_ptr(), G8[1].data_ptr()) if i8 else (G.data_ptr(), DT[G.dtype])
    head = (Q.data_ptr(), *rows, Bq, Ng, Cc, k, 0)
    tail = (s.data_ptr(), i.data_ptr(), ws.data_ptr(), 0)
    if kind == "wide":
        args = head + tail
    elif kind == "filtered_ne":
        args = head + (groups.data_ptr(), own.data_ptr(), nat.FILTER_NE) + tail
    else:
        args = head + (groups.data_ptr(), None, None, nat.FILTER_EQ) + tail
    f = getattr(lib, "cor_similarity_topk" + ("_" + infix[:-1] if infix else ""))

    def fn():
        rc = f(*args, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
        return ws                                            # keeps the buffers alive with the closure
    return fn, s, i


def window(fn, m):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(m):
        fn()
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) / m * 1e3


def gallery(Bq, Ng, Cc, dt):
    g = torch.Generator(device=dev).manual_seed(Bq + Ng)
    Q = torch.nn.functional.normalize(torch.randn((Bq, Cc), device=dev, generator=g), dim=-1)
    G = torch.nn.functional.normalize(torch.randn((Ng, Cc), device=dev, generator=g), dim=-1).to(dt)
    groups = torch.repeat_interleave(torch.arange(Ng, device=dev), torch.randint(1, 9, (Ng,), device=dev, generator=g))[:Ng].to(torch.int32)
    own = groups[torch.randint(0, Ng, (Bq,), device=dev, generator=g)].contiguous()
    return Q, G, groups, own


def _enqueue(f, args, keep):
    def fn():
        rc = f(*args, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
        return keep                                          # keeps the buffers alive with the closure
    return fn


def _outputs(Bq, k, third):
    outs = [torch.empty((Bq, k), device=dev), torch.empty((Bq, k), dtype=torch.int64, device=dev)]
    return outs + ([torch.empty((Bq, k), dtype=torch.int32, device=dev)] if third else [])


def _rand(shape, seed, **kw):
    return torch.rand(shape, device=dev, generator=torch.Generator(device=dev).manual_seed(seed), **kw)


def _ids(Bq, kin, N, seed):
    """i64 [Bq,kin], pairwise different within a row: an arithmetic walk with an odd step through N = 2^j ids"""
    g = torch.Generator(device=dev).manual_seed(seed)
    base, step = torch.randint(0, N, (Bq, 1), device=dev, generator=g), 2 * torch.randint(0, N // 2, (Bq, 1), device=dev, generator=g) + 1
    return ((base + step * torch.arange(kin, device=dev)) % N).contiguous()


def list_data(kernel, Bq, kin, dt, N=131072, Cc=256, KG=20):
    """the inputs of one list-kernel case, shared by both builds (the shapes of tools/{merge,rescore,rerank,expand}_bench.py)"""
    d = dict(scores=torch.sort(_rand((Bq, kin), kin), dim=1, descending=True).values.contiguous(), idx=_ids(Bq, kin, N, kin + 1))
    if kernel == "merge":                                    # P = 8 sorted lists with distinct ids; an image's regions meet across lists
        P = 8
        d["scores"] = torch.sort(_rand((P, Bq, kin), kin), dim=2, descending=True).values.contiguous()
        local = torch.argsort(_rand((P, Bq, 4 * kin), kin + 1), dim=2)[..., :kin]
        d["idx"] = (local + torch.arange(P, device=dev).view(P, 1, 1) * 4 * kin).contiguous()
        d["groups"] = (local // 2).to(torch.int32).contiguous()
    elif kernel in ("rescore", "expand"):
        d["Q"] = torch.nn.functional.normalize(_rand((Bq, Cc), 3) - 0.5, dim=-1)
        d["G"] = torch.nn.functional.normalize(_rand((N, Cc), 4) - 0.5, dim=-1).to(dt)
    else:                                                    # rerank, knn: a graph of width KG, about a third of the slots empty
        g = torch.Generator(device=dev).manual_seed(5)
        d["rnbr"] = torch.randint(0, N, (N, KG), device=dev, generator=g)
        d["rnbr"][_rand((N, KG), 6) < 0.3] = -1
        d["kth"] = (_rand((N,), 7) >= 0.5).float()           # half of the rows count any query among their nearest
    return d


def list_caller(lib, kernel, d, Bq, kin, k, variant):
    """(fn, outputs): fn() enqueues one call of the list kernel on the current stream"""
    c = C
    if kernel == "merge":
        grp = d["groups"] if variant == "distinct" else None
        outs = _outputs(Bq, k, grp is not None)
        args = (d["scores"].data_ptr(), d["idx"].data_ptr(), grp.data_ptr() if grp is not None else None, 8, Bq, kin, k, outs[0].data_ptr(), outs[1].data_ptr(),
                outs[2].data_ptr() if grp is not None else None, None)
        return _enqueue(lib.cor_merge_topk, args, outs), outs
    if kernel == "rescore":
        outs = _outputs(Bq, k, True)
        G = d["G"]
        if variant == "i8":                                  # the int8 call over the same rows, quantised once for both builds
            if "G8" not in d:
                d["G8"] = quantized(G)
            rows, f = (d["G8"][0].data_ptr(), d["G8"][1].data_ptr()), lib.cor_rescore_topk_i8
        else:
            rows, f = (G.data_ptr(), DT[G.dtype]), lib.cor_rescore_topk
        args = (d["Q"].data_ptr(), *rows, Bq, G.shape[0], G.shape[1], 0, d["idx"].data_ptr(), kin, k, outs[0].data_ptr(), outs[1].data_ptr(),
                outs[2].data_ptr(), None)
        return _enqueue(f, args, outs), outs
    one_i, one_ll = (c.c_int * 1), (c.c_longlong * 1)
    if kernel == "expand":                                   # k is m here
        G = d["G"]
        outs = [torch.empty((Bq, G.shape[1]), device=dev)]
        tabs = ((c.c_void_p * 1)(G.data_ptr()), one_ll(0), one_i(G.shape[0]), one_i(DT[G.dtype]))
        args = (d["Q"].data_ptr(), 1.0, *tabs, 1, d["scores"].data_ptr(), d["idx"].data_ptr(), Bq, kin, k, G.shape[1], 3, 1, outs[0].data_ptr(), nat.F32)
        return _enqueue(lib.cor_expand_queries, args, (outs, tabs)), outs
    N, KG = d["rnbr"].shape
    if kernel == "knn":                                      # the graph's own lists as the neighbour lists of one segment
        outs = [torch.empty((N, KG), dtype=torch.int64, device=dev)]
        tabs = ((c.c_void_p * 1)(d["rnbr"].data_ptr()), one_ll(0), one_i(N))
        return _enqueue(lib.cor_knn_reciprocal, (*tabs, 1, KG, 0, outs[0].data_ptr()), (outs, tabs)), outs
    outs = _outputs(Bq, k, True)
    tabs = ((c.c_void_p * 1)(d["rnbr"].data_ptr()), (c.c_void_p * 1)(d["kth"].data_ptr()), one_ll(0), one_i(N))
    args = (d["scores"].data_ptr(), d["idx"].data_ptr(), *tabs, 1, Bq, kin, KG, 20, 0.3, k, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr())
    return _enqueue(lib.cor_rerank_reciprocal, args, (outs, tabs)), outs


ROWS_N, ROWS_C = 3 * 32768, 256                              # three segments of 32768 rows


def rows_data(table):
    """the inputs of the `rows` cases, shared by both builds: the gallery as three segments (`bf16`: all bf16; `f32`: all fp32; `i8`: all int8
    with their scales; `f32bf16`: fp32, bf16, fp32; `mixed`: fp32, bf16, int8), lists whose ids walk 2^17 ids (a quarter of the entries names
    no row), a cell id and a score per row"""
    n = ROWS_N // 3
    G = torch.nn.functional.normalize(_rand((ROWS_N, ROWS_C), 11) - 0.5, dim=-1)
    kinds = dict(bf16=("bf16",) * 3, f32=("f32",) * 3, i8=("i8",) * 3, f32bf16=("f32", "bf16", "f32"), mixed=("f32", "bf16", "i8"))[table]
    segs = []                                                # (rows, scales or None, dtype code)
    for s, kind in enumerate(kinds):
        part = G[s * n:(s + 1) * n]
        if kind == "i8":
            segs.append((*quantized(part.contiguous()), nat.I8))
        else:
            segs.append((part.to(torch.bfloat16 if kind == "bf16" else torch.float32).contiguous(), None, nat.BF16 if kind == "bf16" else nat.F32))
    g = torch.Generator(device=dev).manual_seed(12)
    return dict(segs=segs, Q=torch.nn.functional.normalize(_rand((512, ROWS_C), 3) - 0.5, dim=-1),
                scores=torch.sort(_rand((512, 256), 256), dim=1, descending=True).values.contiguous(), idx=_ids(512, 256, 131072, 257),
                assign=torch.randint(0, 256, (ROWS_N,), device=dev, generator=g).to(torch.int32), score=_rand((ROWS_N,), 13))


def rows_caller(lib, call, d):
    """(fn, outputs): fn() enqueues one call over the segment table on the current stream"""
    segs, n, nseg, Cc = d["segs"], ROWS_N // 3, 3, ROWS_C
    arr = lambda ptrs: (C.c_void_p * nseg)(*ptrs)
    tabs = (arr([r.data_ptr() for r, _, _ in segs]), arr([s.data_ptr() if s is not None else None for _, s, _ in segs]),
            (C.c_longlong * nseg)(*[i * n for i in range(nseg)]), (C.c_int * nseg)(*[n] * nseg), (C.c_int * nseg)(*[dt for _, _, dt in segs]))
    Bq, kin = d["scores"].shape
    lists = (d["scores"].data_ptr(), d["idx"].data_ptr(), Bq, kin)
    if call == "diversify":                                  # tools/diversify_bench.py: kin = 256, k = 50
        outs = _outputs(Bq, 50, True) + [torch.empty((Bq, 50), device=dev)]
        args = (*tabs, nseg, *lists, Cc, 0.5, 0.95, 50, *[o.data_ptr() for o in outs])
        return _enqueue(lib.cor_diversify_mmr, args, (outs, tabs)), outs
    if call == "diffusion":                                  # tools/diffuse_bench.py: kin = 256, kd = 8, kq = k = kin
        outs = _outputs(Bq, kin, True)
        args = (*tabs, nseg, *lists, Cc, 8, kin, 3, 0.9, 20, kin, *[o.data_ptr() for o in outs])
        return _enqueue(lib.cor_rerank_diffusion, args, (outs, tabs)), outs
    if call == "expand_sq":                                  # tools/expand_bench.py: m = 100
        outs = [torch.empty((Bq, Cc), device=dev)]
        args = (d["Q"].data_ptr(), 1.0, *tabs, nseg, d["scores"].data_ptr(), d["idx"].data_ptr(), Bq, kin, 100, Cc, 3, 1, outs[0].data_ptr(), nat.F32)
        return _enqueue(lib.cor_expand_queries_sq, args, (outs, tabs)), outs
    if call == "expand":                                     # the call without scales: fp32 / 16-bit tables only
        outs = [torch.empty((Bq, Cc), device=dev)]
        args = (d["Q"].data_ptr(), 1.0, tabs[0], *tabs[2:], nseg, d["scores"].data_ptr(), d["idx"].data_ptr(), Bq, kin, 100, Cc, 3, 1, outs[0].data_ptr(), nat.F32)
        return _enqueue(lib.cor_expand_queries, args, (outs, tabs)), outs
    K = 8 if call == "kmeans_seed" else 256                  # the seeding is 2 K launches
    assign = arr([d["assign"][i * n:(i + 1) * n].data_ptr() for i in range(nseg)])
    if call == "ivf_build":
        dt = segs[0][2]
        ws = torch.empty((lib.cor_ivf_build_workspace_bytes(ROWS_N, K, Cc),), dtype=torch.uint8, device=dev)
        outs = [torch.empty((ROWS_N, Cc * (1 if dt == nat.I8 else 2)), dtype=torch.uint8, device=dev), torch.zeros((ROWS_N,), device=dev),
                torch.empty((ROWS_N,), dtype=torch.int64, device=dev), torch.empty((K + 1,), dtype=torch.int32, device=dev)]
        args = (*tabs, nseg, assign, Cc, K, dt, *[o.data_ptr() for o in outs], ws.data_ptr())
        return _enqueue(lib.cor_ivf_build, args, (outs, tabs, assign, ws)), outs
    ws = torch.empty((lib.cor_kmeans_workspace_bytes(ROWS_N, K, Cc),), dtype=torch.uint8, device=dev)
    if call == "kmeans_seed":
        outs = [torch.empty((K,), dtype=torch.int64, device=dev), torch.empty((K, Cc), device=dev)]
        return _enqueue(lib.cor_kmeans_seed, (*tabs, nseg, Cc, K, 5, outs[0].data_ptr(), outs[1].data_ptr(), ws.data_ptr()), (outs, tabs, ws)), outs
    score = arr([d["score"][i * n:(i + 1) * n].data_ptr() for i in range(nseg)])
    outs = [torch.empty((K, Cc), device=dev), torch.empty((K,), dtype=torch.int32, device=dev), torch.empty((K,), device=dev)]
    args = (*tabs, nseg, assign, score, Cc, K, None, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), ws.data_ptr())
    return _enqueue(lib.cor_kmeans_update, args, (outs, tabs, assign, score, ws)), outs


def ab(desc, fp, outs_p, fn, outs_n):
    """one case: bitwise-equal outputs, then the alternating rounds and the yardstick"""
    for f in (fp, fn, fp, fn, fp, fn):                       # warm-up, and the results to compare
        f()
    torch.cuda.synchronize()
    for a, b in zip(outs_p, outs_n):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), f"{desc}: parent and new differ"
    m = max(20, min(1000, int(50e3 / max(window(fp, 5), 1.0))))
    us_p, us_n = [], []
    for _ in range(ROUNDS):
        us_p.append(window(fp, m)); us_n.append(window(fn, m))
    mp, mn, spread = statistics.median(us_p), statistics.median(us_n), max(us_p) - min(us_p)
    r = dict(desc, calls_per_round=m, us_parent=us_p, us_new=us_n, median_parent=mp, median_new=mn, parent_spread=spread, bitwise_equal=True,
             within_margin=mn <= mp + spread)
    print(json.dumps(r), flush=True)
    return r


CASES = [("wide", 512, 1000000, 100, 256, torch.bfloat16), ("wide", 512, 125000, 100, 256, torch.bfloat16), ("wide", 64, 20000, 50, 128, torch.float32),
         ("filtered_ne", 512, 1000000, 100, 256, torch.bfloat16), ("distinct", 512, 1000000, 100, 256, torch.bfloat16),
         ("distinct", 512, 1000000, 10, 256, torch.bfloat16),
         ("i8", 512, 1000000, 100, 256, torch.bfloat16), ("i8_filtered_ne", 512, 1000000, 100, 256, torch.bfloat16),
         ("i8_distinct", 512, 1000000, 100, 256, torch.bfloat16), ("i8_distinct", 512, 1000000, 10, 256, torch.bfloat16),
         ("filtered_ne", 64, 20000, 50, 128, torch.float32), ("distinct", 64, 20000, 50, 128, torch.float32)]
# (kernel, Bq, kin, k (expand: m), gallery dtype, variant)
LIST_CASES = ([("merge", 512, kin, kin, None, v) for kin in (100, 256) for v in ("plain", "distinct")]
              + [("rescore", 512, kin, 10, dt, v) for kin in (256, 4096) for dt in (torch.float32, torch.bfloat16) for v in (("", "i8") if dt == torch.float32 else ("",))]
              + [("rerank", 512, kin, 10, None, "") for kin in (256, 1024)] + [("knn", 0, 20, 20, None, "")]
              + [("expand", 512, 256, m, torch.bfloat16, "") for m in (10, 256)])
# (call, table); the tables beyond bf16 and mixed reach the other instantiations of the lane-loader kernels: fp32 alone (ESZ = 4), fp32 and
# 16-bit (ESZ = 0), int8 alone (ESZ = 1)
ROWS_CASES = ([(call, table) for call in ("diversify", "diffusion", "kmeans_seed", "kmeans_update", "expand_sq") for table in ("bf16", "mixed")]
              + [("ivf_build", "bf16"), ("ivf_build", "i8"), ("expand", "f32"), ("expand", "f32bf16"), ("expand_sq", "i8"), ("kmeans_update", "i8")])
ROWS_SHAPE = dict(diversify=dict(Bq=512, kin=256, k=50), diffusion=dict(Bq=512, kin=256, k=256), expand=dict(Bq=512, kin=256, m=100),
                  expand_sq=dict(Bq=512, kin=256, m=100), kmeans_seed=dict(K=8), kmeans_update=dict(K=256), ivf_build=dict(K=256))
rows, data = [], None
for call, table in sorted(ROWS_CASES, key=lambda c: c[1]) if TABLE == "rows" else []:
    if data is None or data[0] != table:
        data = (table, rows_data(table))
    fp, outs_p = rows_caller(parent, call, data[1])
    fn, outs_n = rows_caller(new, call, data[1])
    rows.append(ab(dict(route=call, table=table, rows=ROWS_N, C=ROWS_C, **ROWS_SHAPE[call]), fp, outs_p, fn, outs_n))
for route, Bq, Ng, k, Cc, dt in CASES if TABLE == "topk" else []:
    if data is None or data[0] != (Bq, Ng, Cc, dt):
        data, G8 = ((Bq, Ng, Cc, dt), gallery(Bq, Ng, Cc, dt)), None
    Q, G, groups, own = data[1]
    if route.startswith("i8") and G8 is None:
        G8 = quantized(G)
    fp, sp, ip = caller(parent, route, Q, G, k, groups, own, G8)
    fn, sn, inn = caller(new, route, Q, G, k, groups, own, G8)
    rows.append(ab(dict(route=route, Bq=Bq, Ng=Ng, k=k, C=Cc, dtype=str(dt)), fp, (sp, ip), fn, (sn, inn)))
for kernel, Bq, kin, k, dt, variant in LIST_CASES if TABLE == "lists" else []:
    key = (kernel if kernel in ("merge", "rescore", "expand") else "graph", Bq, kin, dt)
    if data is None or data[0] != key:
        data = (key, list_data(kernel, Bq, kin, dt))
    fp, outs_p = list_caller(parent, kernel, data[1], Bq, kin, k, variant)
    fn, outs_n = list_caller(new, kernel, data[1], Bq, kin, k, variant)
    rows.append(ab(dict(route=kernel, variant=variant, Bq=Bq, kin=kin, k=k, dtype=str(dt)), fp, outs_p, fn, outs_n))
assert rows, f"unknown case table {TABLE!r}"
with open(OUT, "w") as f:
    for r in rows:
        f.write(json.dumps(r) + "\n")
bad = [r for r in rows if not r["within_margin"]]
assert not bad, f"slower than the parent beyond its own spread: {[(r['route'], r.get('table', r.get('Bq')), r.get('Ng', r.get('kin', r.get('K'))), r.get('k')) for r in bad]}"

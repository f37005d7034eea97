#!/usr/bin/env python3
"""Cell-probing search (cor_ivf_build, cor_ivf_search) against the exact search of the PARENT build over the same gallery. GPU only, called
by no test.
Workloads: 1 048 576 x 256 bf16 rows at K = 1024; 8 388 608 x 256 bf16 rows at K = 4096 and the int8 copy of them. The rows are unit
vectors around K planted directions and the queries are drawn the same way. The centres are a strided sample of the rows plus 3 k-means
passes (the exact search as assignment, cor_kmeans_update as centre step); the max-min seeding is too slow to run here.
Per case (Bq in 1, 32, 512; nprobe in 1, 8, 32, 128; k = 10), all through ctypes with every buffer allocated once:
  coarse_us      cor_similarity_topk of the queries over the K fp32 centres, k = nprobe (this build);
  scan_us        cor_ivf_search (scan and finish) over those probes;
  total_us       both, back to back: the whole IVF call;
  exact_us       the yardstick: cor_similarity_topk / cor_similarity_topk_i8 of --parent-lib (the parent commit's libcor_amd.so, loaded beside
                 this build) over the whole gallery at the same Bq; ratio = total_us / exact_us, ranges_overlap says whether the min-max
                 ranges of the two touch;
  recall_at_10   against the yardstick's lists; scanned_share: the mean share of the rows scored;
  floor_us       the scan's read floor: the candidate rows' bytes (every query reads its own cells) over the measured copy bandwidth
                 (6.29 TB/s).
Per workload: build_us (cor_ivf_build, 5 launches) against its copy floor (every row read and written once, with its assign entry, id and
scale). Device events around windows of --calls back-to-back calls; the four sides alternate over --reps windows after --warmup windows in
ONE process. Medians with min-max and the mean shader clock. One JSON line per case, printed and appended to --out.
    python tools/ivf_bench.py --parent-lib FILE [--reps 7] [--warmup 2] [--calls 5] [--small | --large] [--bq 1 32 512] [--split 0] [--out FILE]"""
import argparse, ctypes, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from cor_amd import _native as nat, ops
from cor_amd.retrieval import GalleryShard
from cor_amd.utils import ClockSampler

C, TOPK = 256, 10
COPY_TBS = 6.29            # measured copy bandwidth, SURVEY.md
dev = "cuda:0"
med = statistics.median


def window_us(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def planted(n, K, gen, modes):
    out = torch.empty((n, C), dtype=torch.bfloat16, device=dev)
    for lo in range(0, n, 1 << 20):
        m = min(1 << 20, n - lo)
        x = modes[torch.randint(0, K, (m,), device=dev, generator=gen)] + 0.6 * torch.randn((m, C), device=dev, generator=gen) / C ** 0.5
        out[lo:lo + m] = torch.nn.functional.normalize(x, dim=-1)
    return out


def centres_of(rows, K, passes=3, batch=4096):
    """a strided sample of the rows, then `passes` k-means passes -> (centres f32 [K,C], assign i32 [n])"""
    n = rows.shape[0]
    cent = torch.nn.functional.normalize(rows[:: n // K][:K].float(), dim=-1).contiguous()
    assign = torch.empty((n,), dtype=torch.int32, device=dev)
    for it in range(passes + 1):
        g = GalleryShard(cent)
        for lo in range(0, n, batch):
            assign[lo:lo + batch] = g.search(rows[lo:lo + batch].float(), 1)[1][:, 0]
        if it < passes:
            cent = ops.kmeans_update([(rows, 0)], [assign], K, prev=cent)[0]
    return cent, assign


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True, help="the parent commit's libcor_amd.so: the yardstick is never the code under test")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="only the 1M-row workload")
    ap.add_argument("--large", action="store_true", help="only the 8M-row workloads")
    ap.add_argument("--split", type=int, default=0, help="partial lists per query (0: the library's automatic choice)")
    ap.add_argument("--bq", type=int, nargs="*", default=[1, 32, 512])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ivf_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("ivf_bench.py measures on the GPU (no CPU path)")
    lib = nat.load()
    parent = ctypes.CDLL(os.path.abspath(a.parent_lib))
    assert not hasattr(parent, "cor_ivf_search"), "--parent-lib must be the PARENT build"
    for name in ("cor_similarity_topk", "cor_similarity_topk_i8"):
        getattr(parent, name).argtypes = nat.SIGNATURES[name]
        getattr(parent, name).restype = ctypes.c_int
    for name in ("cor_topk_workspace_bytes", "cor_topk_i8_workspace_bytes"):
        getattr(parent, name).argtypes = nat.SIGNATURES[name]
        getattr(parent, name).restype = ctypes.c_long
    st = torch.cuda.current_stream().cuda_stream
    out = []
    for n, K in ([(1 << 20, 1024)] if a.small else [(1 << 23, 4096)] if a.large else [(1 << 20, 1024), (1 << 23, 4096)]):
        gen = torch.Generator(device=dev).manual_seed(n + K)
        modes = torch.nn.functional.normalize(torch.randn((K, C), device=dev, generator=gen), dim=-1)
        G = planted(n, K, gen, modes)
        Qall = planted(512, K, gen, modes).float().contiguous()
        cent, assign = centres_of(G, K)
        kinds = ["bf16"] if n == 1 << 20 else ["bf16", "int8"]
        for kind in kinds:
            if kind == "int8":
                rows, scales = ops.quantize_rows_i8(G)
                dt, esize = nat.I8, 1
            else:
                rows, scales, dt, esize = G, None, nat.BF16, 2
            # the build, timed, then kept
            seg = ((ctypes.c_void_p * 1)(rows.data_ptr()), (ctypes.c_void_p * 1)(scales.data_ptr() if scales is not None else None),
                   (ctypes.c_longlong * 1)(0), (ctypes.c_int * 1)(n), (ctypes.c_int * 1)(dt))
            seg_a = (ctypes.c_void_p * 1)(assign.data_ptr())
            irows = torch.empty_like(rows)
            iscale = torch.empty((n,), device=dev) if scales is not None else None
            iids = torch.empty((n,), dtype=torch.int64, device=dev)
            cs = torch.empty((K + 1,), dtype=torch.int32, device=dev)
            bws = torch.empty((lib.cor_ivf_build_workspace_bytes(n, K, C),), dtype=torch.uint8, device=dev)

            def build():
                rc = lib.cor_ivf_build(*seg, 1, seg_a, C, K, dt, irows.data_ptr(), iscale.data_ptr() if iscale is not None else None, iids.data_ptr(),
                                       cs.data_ptr(), bws.data_ptr(), st)
                assert rc == 0, rc

            tb = [window_us(build, 1) for _ in range(1 + a.reps)][1:]
            build_floor = n * (2 * C * esize + 4 + 8 + (8 if kind == "int8" else 0)) / (COPY_TBS * 1e12) * 1e6
            counts = (cs[1:] - cs[:-1])
            max_cell = int(counts.max().item())
            del bws
            for Bq in a.bq:
                Q = Qall[:Bq].contiguous()
                ex_s = torch.empty((Bq, TOPK), device=dev)
                ex_i = torch.empty((Bq, TOPK), dtype=torch.int64, device=dev)
                if kind == "int8":
                    ews = torch.empty((parent.cor_topk_i8_workspace_bytes(Bq, n, TOPK),), dtype=torch.uint8, device=dev)

                    def exact():
                        rc = parent.cor_similarity_topk_i8(Q.data_ptr(), rows.data_ptr(), scales.data_ptr(), Bq, n, C, TOPK, 0, ex_s.data_ptr(),
                                                           ex_i.data_ptr(), ews.data_ptr(), 0, st)
                        assert rc == 0, rc
                else:
                    ews = torch.empty((parent.cor_topk_workspace_bytes(Bq, n, TOPK),), dtype=torch.uint8, device=dev)

                    def exact():
                        rc = parent.cor_similarity_topk(Q.data_ptr(), rows.data_ptr(), dt, Bq, n, C, TOPK, 0, ex_s.data_ptr(), ex_i.data_ptr(),
                                                        ews.data_ptr(), 0, st)
                        assert rc == 0, rc
                for nprobe in (1, 8, 32, 128):
                    probes = torch.empty((Bq, nprobe), dtype=torch.int64, device=dev)
                    pscore = torch.empty((Bq, nprobe), device=dev)
                    cws = torch.empty((lib.cor_topk_workspace_bytes(Bq, K, nprobe),), dtype=torch.uint8, device=dev)
                    sws = torch.empty((lib.cor_ivf_search_workspace_bytes(Bq, K, C, nprobe, TOPK, a.split),), dtype=torch.uint8, device=dev)
                    got_s = torch.empty((Bq, TOPK), device=dev)
                    got_i = torch.empty((Bq, TOPK), dtype=torch.int64, device=dev)
                    scanned = torch.empty((Bq,), dtype=torch.int32, device=dev)

                    def coarse():
                        rc = lib.cor_similarity_topk(Q.data_ptr(), cent.data_ptr(), nat.F32, Bq, K, C, nprobe, 0, pscore.data_ptr(), probes.data_ptr(),
                                                     cws.data_ptr(), 0, st)
                        assert rc == 0, rc

                    def scan():
                        rc = lib.cor_ivf_search(Q.data_ptr(), irows.data_ptr(), iscale.data_ptr() if iscale is not None else None, dt, iids.data_ptr(),
                                                cs.data_ptr(), K, C, Bq, probes.data_ptr(), nprobe, TOPK, max_cell, a.split, got_s.data_ptr(),
                                                got_i.data_ptr(), scanned.data_ptr(), sws.data_ptr(), st)
                        assert rc == 0, rc

                    def total():
                        coarse(); scan()

                    sides = (total, coarse, scan, exact)
                    for _ in range(a.warmup):
                        for fn in sides:
                            window_us(fn, a.calls)
                    clock = ClockSampler(dev).start()
                    t = [[] for _ in sides]
                    for _ in range(a.reps):
                        for m, fn in enumerate(sides):
                            t[m].append(window_us(fn, a.calls))
                    clock = clock.stop()
                    torch.cuda.synchronize()
                    hit = (got_i[:, :, None] == ex_i[:, None, :]).any(dim=2).float().mean().item()
                    share = scanned.float().mean().item() / n
                    floor = scanned.double().sum().item() * (C * esize + (4 if kind == "int8" else 0)) / (COPY_TBS * 1e12) * 1e6
                    tt, tc, tsc, te = t
                    r = dict(bench="ivf", rows=n, K=K, C=C, gallery=kind, Bq=Bq, nprobe=nprobe, k=TOPK, max_cell=max_cell, split=a.split,
                             total_us=med(tt), total_us_min_max=[min(tt), max(tt)], coarse_us=med(tc), coarse_us_min_max=[min(tc), max(tc)],
                             scan_us=med(tsc), scan_us_min_max=[min(tsc), max(tsc)], exact_us=med(te), exact_us_min_max=[min(te), max(te)],
                             ratio=med(tt) / med(te), ranges_overlap=not (max(tt) < min(te) or max(te) < min(tt)), recall_at_10=hit,
                             scanned_share=share, floor_us=floor, scan_over_floor=med(tsc) / floor if floor else None,
                             build_us=med(tb), build_us_min_max=[min(tb), max(tb)], build_floor_us=build_floor, build_over_floor=med(tb) / build_floor,
                             yardstick="parent library, exact search of the whole gallery", reps=a.reps, calls_per_window=a.calls,
                             sclk_mhz_mean=clock.get("sclk_mhz_mean"))
                    print(json.dumps(r), flush=True)
                    out.append(r)
                del ews
            del irows, iscale, iids
            torch.cuda.empty_cache()
        del G
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for r in out:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

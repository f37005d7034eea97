#!/usr/bin/env python3
"""Host merge against device merge of P per-shard top-k lists, as the merging rank of distributed_search meets them: P lists of k entries
for each of B query slots, already on the GPU (the gathered packed lists).
  (a) host:   ONE device-to-host copy of the packed lists ([P,B,k,3] int32, distinct: [P,B,k,4]) + retrieval.merge_topk[_distinct]_host on
              the CPU with 16 threads: what merge="host" does on `dst`.
  (b) device: ops.merge_topk on the GPU + ONE device-to-host copy of [B,k] indices and scores: what merge="device" does.
Both are host wall time from the first enqueue to the merged lists being on the host (they end there), medians over --reps calls after
--warmup calls, the two sides alternating; (a) is split into its copy and its sort, and the kernel of (b) is also timed alone with device
events over a window of back-to-back launches. The two results are compared bitwise before anything is timed.
One JSON line per shape and mode, printed and appended to --out (default profiles/merge_device.jsonl).
    python tools/merge_bench.py [--reps 15] [--warmup 3] [--out FILE]"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from cor_amd import ops, retrieval

SHAPES = [(8, 256, 10), (8, 512, 10), (8, 512, 100), (8, 256, 256)]
dev = "cuda:0"


def lists(P, B, k):
    """P sorted lists per query with distinct global ids; an image's regions (group = id // 2 within a list's id range) meet across lists."""
    g = torch.Generator(device=dev).manual_seed(P * B + k)
    s = torch.sort(torch.randn((P, B, k), device=dev, generator=g), dim=2, descending=True).values
    local = torch.argsort(torch.rand((P, B, 4 * k), device=dev, generator=g), dim=2)[..., :k]
    i = local + torch.arange(P, device=dev).view(P, 1, 1) * 4 * k
    return s.contiguous(), i.contiguous(), (local // 2).to(torch.int32).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge_device.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("merge_bench.py measures on the GPU (no CPU path)")
    torch.set_num_threads(16)
    rows = []
    for P, B, k in SHAPES:
        s, i, grp = lists(P, B, k)
        for distinct in (False, True):
            packed = retrieval._pack_lists(s, i)
            if distinct:
                packed = torch.cat([packed, grp.unsqueeze(-1)], dim=-1).contiguous()
            pinned_a = torch.empty(packed.shape, dtype=torch.int32, pin_memory=True)
            pinned_b = torch.empty((3 * B * k,), dtype=torch.int32, pin_memory=True)

            def host():
                t0 = time.perf_counter()
                pinned_a.copy_(packed, non_blocking=True)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                ps, pi = retrieval._unpack_lists(pinned_a[..., :3])
                if distinct:
                    out = retrieval.merge_topk_distinct_host(list(ps), list(pi), list(pinned_a[..., 3]), k)
                else:
                    out = retrieval.merge_topk_host(list(ps), list(pi), k)
                t2 = time.perf_counter()
                return out, (t1 - t0) * 1e3, (t2 - t1) * 1e3

            def device():
                t0 = time.perf_counter()
                ps, pi = retrieval._unpack_lists(packed[..., :3])             # the gathered lists arrive packed: unpacking is part of the path
                out = ops.merge_topk(ps, pi, k, packed[..., 3].contiguous() if distinct else None)
                flat = torch.cat([out[1].view(torch.int32).reshape(-1), out[0].view(torch.int32).reshape(-1)])
                pinned_b.copy_(flat, non_blocking=True)
                torch.cuda.synchronize()
                n = B * k
                res = pinned_b[2 * n:].view(torch.float32).view(B, k), pinned_b[:2 * n].view(torch.int64).view(B, k)
                return res, (time.perf_counter() - t0) * 1e3

            (hs, hi), _, _ = host()
            (ds, di), _ = device()
            assert torch.equal(hi, di) and torch.equal(hs.view(torch.int32), ds.view(torch.int32)), (P, B, k, distinct)
            for _ in range(a.warmup):
                host(); device()
            t_copy, t_sort, t_dev = [], [], []
            for _ in range(a.reps):
                _, c, m = host()
                t_copy.append(c); t_sort.append(m)
                t_dev.append(device()[1])
            ps, pi = retrieval._unpack_lists(packed[..., :3])
            pg = packed[..., 3].contiguous() if distinct else None
            n_launch = 200
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n_launch):
                ops.merge_topk(ps, pi, k, pg)
            e1.record(); e1.synchronize()
            med = statistics.median
            host_ms = med([c + m for c, m in zip(t_copy, t_sort)])
            r = dict(P=P, B=B, k=k, mode="distinct" if distinct else "plain", entries_per_query=P * k,
                     host_copy_bytes=packed.numel() * 4, device_copy_bytes=3 * B * k * 4,
                     host_total_ms=host_ms, host_copy_ms=med(t_copy), host_sort_ms=med(t_sort), host_total_ms_min_max=[min(c + m for c, m in zip(t_copy, t_sort)), max(c + m for c, m in zip(t_copy, t_sort))],
                     device_total_ms=med(t_dev), device_total_ms_min_max=[min(t_dev), max(t_dev)],
                     merge_kernel_call_us=e0.elapsed_time(e1) / n_launch * 1e3, ratio_device_over_host=med(t_dev) / host_ms,
                     cpu_threads=torch.get_num_threads(), reps=a.reps)
            print(json.dumps(r), flush=True)
            rows.append(r)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

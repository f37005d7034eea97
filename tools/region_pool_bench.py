#!/usr/bin/env python3
"""GPU timing of the multi-region gallery path; JSON lines appended to profiles/region_pool.jsonl.
    python tools/region_pool_bench.py op        # ops.region_pool against the former way of pooling the same rows
    python tools/region_pool_bench.py builder   # build_gallery_regions against build_gallery, regions per second (SAM-B encoder, full depth)
    python tools/region_pool_bench.py op 20     # 20 region_pool calls only (for rocprofv3 --kernel-trace --stats, in a run of its own)
op: B = 32 images x 16 regions, P = 4096, D = 256 (512 rows). The former way is ops.masked_pool with B = 512 over tokens replicated per
region (cor_masked_pool and its kernel are the same code in the commit before this entry point existed); the replication copy
(index_select of 512 x 4 MB) is timed separately. Each side: warm-up, then rounds alternating between the sides; a round enqueues
`calls` launches back to back between two HIP events on the launch stream; the figure is the median over the rounds of time per call.
The 128 MB of tokens fit the 256 MB Infinity Cache, their 2 GB replica does not: region_pool's tokens can stay cached between calls,
which is also the builder's situation (the encoder has just written them); masked_pool's replica always comes from HBM.
builder: one synthetic set of 32 images x 8 regions at 1024^2 (device tensors, no files), batches of 8 images; both builders in one
process, alternating, host wall time around a device synchronise; the old builder gets the same data as 256 (image, mask) pairs."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from cor_amd import ops, utils  # noqa: E402

dev = "cuda:0"
OUT = os.path.join(ROOT, "profiles", "region_pool.jsonl")


def emit(rec):
    print(json.dumps(rec), flush=True)
    with open(OUT, "a") as f:
        f.write(json.dumps(rec) + "\n")


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls            # us per call


def bench_op(only_new_calls=0):
    B, per, P, D = 32, 16, 4096, 256
    R = B * per
    g = torch.Generator().manual_seed(5)
    tokens = torch.randn(B, P, D, generator=g).to(dev)
    masks = torch.rand(R, P, generator=g).to(dev)
    off = torch.arange(0, R + 1, per, dtype=torch.int32, device=dev)
    img_of = torch.repeat_interleave(torch.arange(B, device=dev), per)
    new = lambda: ops.region_pool(tokens, masks, off, B, P, D, clamp01=True, l2norm=True)   # noqa: E731
    if only_new_calls:
        for _ in range(only_new_calls):
            new()
        torch.cuda.synchronize()
        return
    rep = tokens.index_select(0, img_of)                                                    # [512, P, D]: 2 GB
    old = lambda: ops.masked_pool(rep, masks, R, P, D, feat_nchw=False, clamp01=True, l2norm=True)   # noqa: E731
    copy = lambda: tokens.index_select(0, img_of)                                           # noqa: E731
    same = bool(torch.equal(new().view(torch.int32), old().view(torch.int32)))
    for fn in (new, old, copy):
        timed(fn, 3)
    clock = utils.ClockSampler(dev).start()
    t = {"region_pool": [], "masked_pool_replicated": [], "replication_copy": []}
    for _ in range(7):
        t["region_pool"].append(timed(new, 20))
        t["masked_pool_replicated"].append(timed(old, 5))
        t["replication_copy"].append(timed(copy, 5))
    clk = clock.stop()
    med = {k: statistics.median(v) for k, v in t.items()}
    emit(dict(kind="op", B=B, regions_per_image=per, P=P, D=D, rows=R, bit_identical=same,
              us_per_call_median=med, us_per_call_min={k: min(v) for k, v in t.items()}, us_per_call_max={k: max(v) for k, v in t.items()},
              speedup_vs_masked_pool_alone=med["masked_pool_replicated"] / med["region_pool"],
              token_bytes=B * P * D * 4, region_pool_token_GBps=B * P * D * 4 * (per // 8) / med["region_pool"] / 1e3, clock=clk,
              note="region_pool_token_GBps counts the tokens once per tile of 8 regions (what the kernel requests, cached or not)"))


def bench_builder():
    from cor_amd import retrieval
    from cor_amd.lib.build_model import build_model_with_query_support_feat
    n_img, per, bs = 32, 8, 8
    model = build_model_with_query_support_feat("sam_base", "ViT-B-16-SigLIP-384", None, None, "MaskedPooling").to(dev).eval()
    g = torch.Generator().manual_seed(6)
    imgs = torch.randn(n_img, 3, 1024, 1024, generator=g).to(dev)
    masks = (torch.rand(n_img * per, 1, 64, 64, generator=g) > 0.7).float().to(dev)          # already at the token grid on both sides

    def region_batches():
        for i in range(0, n_img, bs):
            yield dict(query_img=imgs[i:i + bs], region_masks=masks[i * per:(i + bs) * per],
                       region_offsets=torch.arange(0, bs * per + 1, per, dtype=torch.int32))

    def pair_batches():
        for r in range(0, n_img * per, bs):
            idx = torch.arange(r, r + bs, device=dev) // per
            yield dict(query_img=imgs.index_select(0, idx), query_mask=masks[r:r + bs])

    def run(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    with torch.autocast("cuda", dtype=torch.bfloat16):
        new = lambda: retrieval.build_gallery_regions(model, region_batches(), dtype=torch.float16)[0]   # noqa: E731
        old = lambda: retrieval.build_gallery(model, pair_batches(), dtype=torch.float16)               # noqa: E731
        _, a = run(new)
        _, b = run(old)
        err = float((a.float() - b.float()).abs().max())
        clock = utils.ClockSampler(dev).start()
        tn, to = [], []
        for _ in range(3):
            tn.append(run(new)[0])
            to.append(run(old)[0])
        clk = clock.stop()
    n = n_img * per
    emit(dict(kind="builder", images=n_img, regions_per_image=per, rows=n, batch_images=bs, encoder="SAM-B depth 12, default (bf16) mode",
              seconds_median=dict(build_gallery_regions=statistics.median(tn), build_gallery=statistics.median(to)),
              seconds_all=dict(build_gallery_regions=tn, build_gallery=to),
              regions_per_second=dict(build_gallery_regions=n / statistics.median(tn), build_gallery=n / statistics.median(to)),
              ratio=statistics.median(to) / statistics.median(tn), max_abs_row_difference=err, clock=clk,
              note="the old builder's input includes the gather of each pair's image on the device (index_select), no file decoding on either side"))


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "op"
    if mode == "op":
        bench_op(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
    elif mode == "builder":
        bench_builder()
    else:
        raise SystemExit(__doc__)

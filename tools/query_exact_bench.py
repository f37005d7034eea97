"""Same-box speed of the exact-query mode against the default line.

The headline workload of bench.py (SAM-B + SigLIP-B/16-384 + MaskAdapterPooling, B = 32 structured synthetic triplets, a 100k-row bf16
gallery, top-10, two forwards in flight through model.capture_pipeline, every step's lists on the host inside the timed region), run
with compute_dtype bf16 and query_dtype None ("default") and query_dtype float32 ("exact_query"), in alternating rounds on ONE model
and ONE gallery. Then a stand-alone timing of flash_fwd_f32 (cor_attention_f32) against the fp32 row-per-lane kernel (cor_attention)
on the SigLIP-B tower shape. One JSON line per measurement on stdout (and appended to --out).

    python tools/query_exact_bench.py --steps 20 --warmup 3 --rounds 3 --out profiles/query_exact_bench.jsonl
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def time_mode(model, pipe, search, steps, warmup):
    import torch
    for _ in range(warmup):
        pipe.submit(None, then=search)[1].result()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pend = []
    for _ in range(steps):
        pend.append(pipe.submit(None, then=search)[1])
        while len(pend) > 1:
            pend.pop(0).result()
    while pend:
        pend.pop(0).result()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def attention_timing(reps, out):
    import torch
    from cor_amd import ops
    N, H, T, hd = 32, 12, 576, 64                      # SigLIP-B/16-384 tower at batch 32
    D = H * hd
    qkv = torch.randn((N * T, 3 * D), device="cuda")
    q, k, v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
    flops = 4.0 * N * H * T * T * hd
    for name, fn in (("flash_fwd_f32", lambda: ops.attention_f32(q, k, v, N, H, T, T, hd, hd ** -0.5)),
                     ("flash_fwd_f32_x3_out", lambda: ops.attention_f32(q, k, v, N, H, T, T, hd, hd ** -0.5, out_dtype=ops.X3)),
                     ("attn_rowlane_fp32", lambda: ops.attention(q, k, v, N, H, T, T, hd, hd ** -0.5, out_dtype=torch.float32))):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / reps
        emit(dict(kind="attention", kernel=name, shape=dict(N=N, H=H, T=T, hd=hd), ms=round(ms, 4), tflops=round(flops / ms / 1e9, 2)), out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3, help="alternating (default, exact_query) rounds")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--gallery", type=int, default=100000)
    ap.add_argument("--attn-reps", type=int, default=20)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "4")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("query_exact_bench.py needs a GPU")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    from cor_amd import retrieval, utils
    from cor_amd.lib.build_model import build_model_with_query_support_feat

    model = build_model_with_query_support_feat("sam_base", "ViT-B-16-SigLIP-384", None, None, "MaskAdapterPooling")
    utils.randomize_parameters(model, seed=0)
    utils.zero_support_head_biases(model)
    model = model.to(dev).eval()
    model.compute_dtype = torch.bfloat16
    B = args.batch
    batch = utils.synthetic_batch(B, dev, seed=0, structured=True)
    gen = torch.Generator(device="cpu").manual_seed(1234)
    rows = torch.nn.functional.normalize(torch.randn((args.gallery, 256), generator=gen), dim=-1)
    shard = retrieval.GalleryShard(rows.to(dev), offset=0, dtype=torch.bfloat16)

    def search(out):
        return retrieval.distributed_search(out[2][:, 0], shard, 10, max_local=B, defer=True)

    pipes = {}
    for mode, qd in (("default", None), ("exact_query", torch.float32)):
        model.query_dtype = qd
        pipes[mode] = model.capture_pipeline(**batch, multimask_output=True, depth=2)
    res = {m: [] for m in pipes}
    for r in range(args.rounds):
        for mode in pipes:
            dt = time_mode(model, pipes[mode], search, args.steps, args.warmup)
            tps = B * args.steps / dt
            res[mode].append(tps)
            emit(dict(kind="step", mode=mode, round=r, steps=args.steps, batch=B, triplets_per_s=round(tps, 2),
                      ms_per_step=round(dt / args.steps * 1e3, 3)), out=args.out)
    d, e = max(res["default"]), max(res["exact_query"])
    emit(dict(kind="summary", workload="sam_base+ViT-B-16-SigLIP-384+MaskAdapterPooling, B=32, 100k-row bf16 gallery, top-10, "
                                       "capture_pipeline depth 2", default_best=round(d, 2), exact_query_best=round(e, 2),
              ratio=round(e / d, 4), rounds=args.rounds, steps=args.steps), out=args.out)
    del pipes
    torch.cuda.synchronize()
    attention_timing(args.attn_reps, args.out)


if __name__ == "__main__":
    main()

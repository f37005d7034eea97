"""GPU side of the multi-region gallery builder: ops.region_pool bit for bit against per-region ops.masked_pool, its independence of
the other regions of the tile, parity with the oracle's region embedding, and the builder end to end from a CSV (one encoder pass
per distinct image, rows in CSV order, group ids, save -> load -> distinct search)."""
import csv

import numpy as np
import pytest
import torch

from oracle import config as ocfg, retrieval as oret, sam as osam
from tests.golden_util import make_inputs
from tests.test_gpu_parity import DEV, _build, report

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

_BITS = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(_BITS[a.dtype]), b.contiguous().view(_BITS[b.dtype]))


def _problem(seed, counts, P, D):
    """tokens [B,P,D], masks [R,P] with values outside [0,1]; region 0 is all zero and the last one a single pixel."""
    g = torch.Generator().manual_seed(seed)
    B, R = len(counts), sum(counts)
    tokens = torch.randn(B, P, D, generator=g)
    masks = torch.randn(R, P, generator=g) * 0.8 + 0.4
    masks[0] = 0.0
    if R > 1:
        masks[R - 1] = 0.0
        masks[R - 1, (7 * P) // 11] = 1.0
    off = torch.tensor([0] + np.cumsum(counts).tolist(), dtype=torch.int32)
    return tokens.to(DEV), masks.to(DEV), off.to(DEV)


def _per_region(ops, tokens, masks, off, clamp01, l2norm):
    B, P, D = tokens.shape
    o = off.cpu().tolist()
    rows = [ops.masked_pool(tokens[b], masks[r], 1, P, D, feat_nchw=False, clamp01=clamp01, l2norm=l2norm)
            for b in range(B) for r in range(o[b], o[b + 1])]
    return torch.cat(rows, dim=0)


@pytest.mark.parametrize("counts,P,D", [
    ([1], 64, 32),               # one image, one region
    ([3, 0, 2], 100, 48),        # an image without regions between two that have some; P below one chunk and ragged
    ([9], 300, 256),             # one region more than a tile; two chunks of p, the second partial
    ([19, 5], 4096, 256),        # the real shape; three tiles, the last with 3 of 8 regions
    ([3], 576, 768),             # more channels than threads
])
def test_region_pool_bitwise_vs_masked_pool(counts, P, D):
    from cor_amd import ops
    tokens, masks, off = _problem(101 + P + D, counts, P, D)
    for clamp01 in (False, True):
        for l2norm in (False, True):
            ref = _per_region(ops, tokens, masks, off, clamp01, l2norm)
            got = ops.region_pool(tokens, masks, off, len(counts), P, D, clamp01=clamp01, l2norm=l2norm)
            assert _same_bits(got, ref), (counts, P, D, clamp01, l2norm, float((got - ref).abs().max()))
            assert torch.equal(got, ref) or not bool(torch.isfinite(ref).all())
            for dt in (torch.float16, torch.bfloat16):
                got16 = ops.region_pool(tokens, masks, off, len(counts), P, D, out_dtype=dt, clamp01=clamp01, l2norm=l2norm)
                assert _same_bits(got16, ref.to(dt)), (counts, P, D, clamp01, l2norm, dt)
                assert torch.equal(got16, ref.to(dt)) or not bool(torch.isfinite(ref.to(dt).float()).all())


def test_region_pool_row_is_independent_of_its_neighbours():
    from cor_amd import ops
    P, D = 4096, 256
    tokens, masks, off = _problem(7, [37], P, D)
    masks[36] = torch.rand(P, device=DEV)
    one = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    alone = ops.region_pool(tokens, masks[36:37].contiguous(), one, 1, P, D, clamp01=True, l2norm=True)
    last = ops.region_pool(tokens, masks, off, 1, P, D, clamp01=True, l2norm=True)
    flipped = ops.region_pool(tokens, masks.flip(0).contiguous(), off, 1, P, D, clamp01=True, l2norm=True)
    assert _same_bits(alone[0], last[36]) and _same_bits(alone[0], flipped[0])
    assert _same_bits(flipped.flip(0), last)
    # two images, the region lists swapped between them in memory order: rows follow their masks
    tokens2, masks2, off2 = _problem(8, [5, 11], P, D)
    a = ops.region_pool(tokens2, masks2, off2, 2, P, D, clamp01=True, l2norm=True)
    for b, (lo, hi) in enumerate([(0, 5), (5, 16)]):
        solo = ops.region_pool(tokens2[b:b + 1].contiguous(), masks2[lo:hi].contiguous(),
                               torch.tensor([0, hi - lo], dtype=torch.int32, device=DEV), 1, P, D, clamp01=True, l2norm=True)
        assert _same_bits(solo, a[lo:hi])


def test_region_pool_edge_arguments():
    from cor_amd import ops, _native
    tokens, masks, off = _problem(9, [2, 1], 64, 32)
    out = ops.region_pool(tokens, masks[:0].contiguous(), torch.zeros(3, dtype=torch.int32, device=DEV), 2, 64, 32)
    assert out.shape == (0, 32)
    big = torch.zeros(1, 4, 1025, device=DEV)
    with pytest.raises(_native.NativeError):                                           # D above the documented bound: no kernel
        ops.region_pool(big, torch.ones(1, 4, device=DEV), torch.tensor([0, 1], dtype=torch.int32, device=DEV), 1, 4, 1025)
    # offsets the host cannot see: whatever they hold, the kernel stays inside its arrays (rows it does not cover are not written)
    wild = torch.tensor([-5, 99, 1], dtype=torch.int32, device=DEV)
    ops.region_pool(tokens, masks, wild, 2, 64, 32)
    torch.cuda.synchronize()
    ref = _per_region(ops, tokens, masks, off, False, False)
    assert _same_bits(ops.region_pool(tokens, masks, off, 2, 64, 32), ref)


def test_region_pool_vs_oracle_region_embedding():
    from cor_amd import ops
    counts = [3, 1, 2]
    inp = make_inputs(211, emb=(3, 256, 64, 64), mask=("mask", 6, 256))
    img_of = torch.repeat_interleave(torch.arange(3), torch.tensor(counts))
    ref = oret.region_embedding(inp["emb"][img_of], inp["mask"])[:, 0]
    tok = ops.nchw_to_tokens(inp["emb"].to(DEV), torch.float32)
    m = ops.bilinear(inp["mask"].to(DEV), 64, 64).reshape(6, 4096)
    off = torch.tensor([0, 3, 4, 6], dtype=torch.int32, device=DEV)
    got = ops.region_pool(tok, m, off, 3, 4096, 256, clamp01=True, l2norm=True)
    report("region_pool_vs_oracle_region_embedding", got, ref, 1e-4, 1e-5)


def test_gallery_regions_builder_end_to_end(tmp_path, monkeypatch):
    """3 images x {3, 1, 2} regions, an image's rows not adjacent in the CSV, two Dataset folders that share a file name, one
    Compose == 1 row. Reduced model, random state (as test_gallery_builder_and_checkpoint_loader)."""
    from PIL import Image
    from cor_amd import config, dataloader, engine, retrieval
    from oracle import preprocess as OP
    gcfg = dict(config.siglip_cfg("ViT-B-16-SigLIP-384"), depth=1, t_depth=1, vocab=64)
    model = _build(2, (1,), gcfg, "MaskedPooling")
    sd = ocfg.random_state({k: tuple(v.shape) for k, v in model.state_dict().items()}, 61)
    model.load_state_dict(sd, strict=True)
    model = model.to(DEV).eval()
    rng = np.random.default_rng(64)
    root = tmp_path / "data"
    images = {("dsA", "q0.png"): (300, 220), ("dsB", "q0.png"): (180, 240), ("dsA", "q1.png"): (256, 256)}
    for (ds, name), (w, h) in images.items():
        (root / ds / "image").mkdir(parents=True, exist_ok=True)
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(root / ds / "image" / name)
    # (Dataset, Query_img, Target, Query_mask, Compose): image A0 has rows 0, 3, 5 of the kept rows, A1 rows 2, 4, B0 row 1
    order = [("dsA", "q0.png", "dog", "a0.png", 0), ("dsB", "q0.png", "dog", "b0.png", 0), ("dsA", "q1.png", "cat", "c0.png", 0),
             ("dsA", "q0.png", "cat", "a1.png", 0), ("dsB", "q0.png", "cat", "skipped.png", 1), ("dsA", "q1.png", "dog", "c1.png", 0),
             ("dsA", "q0.png", "dog", "a2.png", 0)]
    recs = []
    for i, (ds, name, tgt, mname, compose) in enumerate(order):
        w, h = images[(ds, name)]
        (root / ds / "mask" / tgt).mkdir(parents=True, exist_ok=True)
        mk = np.zeros((h, w), np.uint8)
        y0, x0 = (i * 23) % (h // 2), (i * 37) % (w // 2)
        mk[y0: y0 + h // 3, x0: x0 + w // 4] = 255
        Image.fromarray(mk).save(root / ds / "mask" / tgt / mname)
        recs.append(dict(Id=i, Query_img=name, Query_mask=mname, Support_img="x.png", Support_mask="x.png", Text="t", Compose=compose,
                         Dataset=ds, Target=tgt, query_cat=0))
    path = str(tmp_path / "gal.csv")
    with open(path, "w", newline="") as f:
        wr = csv.DictWriter(f, fieldnames=dataloader.CSV_COLUMNS); wr.writeheader(); wr.writerows(recs)
    kept = [r for r in recs if r["Compose"] == 0]

    encoded = []
    real_encoder = engine.sam_encoder

    def counting_encoder(W, img, cfg, T):
        encoded.append(int(img.shape[0]))
        return real_encoder(W, img, cfg, T)

    monkeypatch.setattr(engine, "sam_encoder", counting_encoder)
    rows, groups = retrieval.build_gallery_regions(model, dataloader.gallery_region_batches(path, str(root), batch_size=2, device=DEV),
                                                   dtype=torch.float32)
    n_regions_builder = sum(encoded)
    encoded.clear()
    rows_old = retrieval.build_gallery(model, dataloader.gallery_batches(path, str(root), batch_size=2, device=DEV), dtype=torch.float32)
    n_old_builder = sum(encoded)
    monkeypatch.setattr(engine, "sam_encoder", real_encoder)
    assert (n_regions_builder, n_old_builder) == (3, 6)                                # (a) one encoder pass per distinct image
    assert rows.shape == (6, 256) and rows_old.shape == (6, 256)
    report("gallery_region_rows_vs_build_gallery", rows, rows_old, 1e-3, 1e-4)          # (b) CSV order, the old builder's rows
    keys = list(images)
    emb = {}
    for ds, name in keys:
        qi = torch.from_numpy(OP.to_tensor_normalize(OP.resize_bilinear_u8(np.asarray(Image.open(root / ds / "image" / name).convert("RGB")), 1024, 1024),
                                                     OP.IMAGENET_MEAN, OP.IMAGENET_STD))[None]
        emb[(ds, name)] = osam.image_encoder(sd, qi, dict(model.image_encoder.cfg))
    mi = torch.stack([torch.from_numpy(OP.to_tensor_normalize(OP.resize_bilinear_u8(
        np.asarray(Image.open(root / r["Dataset"] / "mask" / r["Target"] / r["Query_mask"]).convert("L")), 1024, 1024), None, None)) for r in kept])
    ref = oret.region_embedding(torch.cat([emb[(r["Dataset"], r["Query_img"])] for r in kept]), mi)[:, 0]
    report("gallery_region_rows_from_csv_vs_oracle", rows, ref, 1e-3, 1e-4)
    want_groups, gkeys = dataloader.gallery_groups(path)                               # (c)
    assert groups.dtype == torch.int32 and torch.equal(groups.cpu(), want_groups) and want_groups.tolist() == [0, 1, 2, 0, 2, 0]
    assert gkeys == keys
    # 16-bit rows are the rounded fp32 rows of the same call
    rows16, _ = retrieval.build_gallery_regions(model, dataloader.gallery_region_batches(path, str(root), batch_size=2, device=DEV, max_regions=2))
    assert rows16.dtype == torch.float16
    # bound: the encoder's batch-size dependence as above (1e-3 / 1e-4) + half an fp16 ulp of a component below 1 (2^-12 = 2.5e-4)
    report("gallery_region_rows_fp16_split_batches", rows16, rows, 1e-3, 1e-4 + 2.5e-4)
    # (d) disk round trip with group ids, then a distinct search: three different images, the query's own region first
    retrieval.save_gallery(str(tmp_path / "gal"), rows, world=2, groups=groups)
    shards = [retrieval.load_gallery_shard(str(tmp_path / "gal"), r, DEV) for r in range(2)]
    assert [s.offset for s in shards] == [0, 3] and torch.equal(shards[1].groups.cpu(), want_groups[3:])
    for j in (0, 2):
        s0, i0 = shards[0].search(rows[j:j + 1], k=3, distinct=True)
        assert int(i0[0, 0]) == j and sorted(want_groups[i0[0].cpu()].tolist()) == [0, 1, 2]
        parts = [sh.search(rows[j:j + 1], k=3, distinct=True) for sh in shards]
        ms, mi_ = retrieval.merge_topk_distinct_host([p[0].cpu() for p in parts], [p[1].cpu() for p in parts],
                                                     [retrieval.groups_of(p[1], want_groups).to(torch.int32) for p in parts], 3)
        assert int(mi_[0, 0]) == j and sorted(want_groups[mi_[0]].tolist()) == [0, 1, 2]

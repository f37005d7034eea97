"""CPU side of the multi-region gallery builder: the cor_region_pool entry point in header / library / ctypes table, the front end's
refusal of CPU tensors, the group ids and batch plans of the loader, and build_gallery_regions' host logic with the device parts
replaced by CPU stand-ins."""
import csv
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _write_csv(path, recs):
    from cor_amd import dataloader
    with open(path, "w", newline="") as f:
        wr = csv.DictWriter(f, fieldnames=dataloader.CSV_COLUMNS)
        wr.writeheader()
        wr.writerows(recs)


def _rec(i, ds, img, target, mask, compose=0):
    return dict(Id=i, Query_img=img, Query_mask=mask, Support_img="x.png", Support_mask="x.png", Text="t", Compose=compose, Dataset=ds,
                Target=target, query_cat=0)


def test_region_pool_is_declared_exported_and_bound():
    if not os.path.exists(os.path.join(ROOT, "cor_amd", "csrc", "libcor_amd.so")):
        import __graft_entry__ as g
        g.build()
    from cor_amd import _native
    lib = _native.load()
    hdr = open(os.path.join(ROOT, "include", "cor_amd.h")).read()
    proto = re.search(r"^int\s+cor_region_pool\s*\(([^)]*)\)\s*;", hdr, flags=re.M | re.S)
    assert proto, "cor_region_pool is not declared in include/cor_amd.h"
    assert hasattr(lib, "cor_region_pool")
    assert len(proto.group(1).split(",")) == 12 and len(_native.SIGNATURES["cor_region_pool"]) == 12


def test_region_pool_refuses_cpu_tensors():
    from cor_amd import ops
    with pytest.raises(RuntimeError):
        ops.region_pool(torch.zeros(1, 16, 8), torch.zeros(2, 16), torch.tensor([0, 2], dtype=torch.int32), 1, 16, 8)


def test_gallery_groups_key_on_dataset_and_image(tmp_path):
    from cor_amd import dataloader
    recs = [_rec(0, "dsA", "0001.jpg", "dog", "m0.png"), _rec(1, "dsB", "0001.jpg", "cat", "m1.png"),
            _rec(2, "dsA", "0002.jpg", "dog", "m2.png", compose=1), _rec(3, "dsA", "0001.jpg", "cat", "m3.png"),
            _rec(4, "dsA", "0003.jpg", "dog", "m4.png"), _rec(5, "dsB", "0001.jpg", "dog", "m5.png")]
    _write_csv(tmp_path / "g.csv", recs)
    groups, keys = dataloader.gallery_groups(str(tmp_path / "g.csv"))
    assert groups.dtype == torch.int32 and groups.tolist() == [0, 1, 0, 2, 1]          # the Compose == 1 row is absent
    assert keys == [("dsA", "0001.jpg"), ("dsB", "0001.jpg"), ("dsA", "0003.jpg")]
    labels, names = dataloader.gallery_labels(str(tmp_path / "g.csv"), column="Query_img")
    assert labels.shape == groups.shape
    assert labels.tolist() == [0, 0, 0, 1, 0]                                          # the file name alone merges the two datasets
    df = dataloader.read_pairs_csv(str(tmp_path / "g.csv"))
    assert [keys[g] for g in groups.tolist()] == list(zip(df["Dataset"], df["Query_img"]))


def _check_plan(plan, groups, images_per_batch, max_regions):
    rows = [r for batch in plan for _, rs in batch for r in rs]
    assert sorted(rows) == list(range(len(groups)))                                    # every row exactly once: a permutation
    counts = {}
    for g in groups:
        counts[g] = counts.get(g, 0) + 1
    pieces = {}
    for batch in plan:
        assert 1 <= len(batch) <= images_per_batch
        if max_regions is not None:
            assert sum(len(rs) for _, rs in batch) <= max_regions
        for g, rs in batch:
            assert all(groups[r] == g for r in rs) and rs == sorted(rs)
            pieces.setdefault(g, []).append(rs)
    first_seen = list(dict.fromkeys(groups))
    assert list(pieces) == first_seen                                                  # images in order of first appearance
    for g, ps in pieces.items():
        assert [r for p in ps for r in p] == [i for i, x in enumerate(groups) if x == g]   # CSV order inside an image
        if max_regions is None or counts[g] <= max_regions:
            assert len(ps) == 1, f"image {g} was split without need"
        else:
            assert len(ps) == -(-counts[g] // max_regions)
    return rows


def test_plan_region_batches():
    from cor_amd import dataloader
    groups = [0, 1, 0, 2, 2, 2, 2, 2, 3, 1, 4, 0]                                      # image 0: rows 0, 2, 11 (A, B, A interleaving)
    plan = dataloader.plan_region_batches(groups, images_per_batch=2)
    _check_plan(plan, groups, 2, None)
    assert plan[0] == [(0, [0, 2, 11]), (1, [1, 9])]
    plan = dataloader.plan_region_batches(torch.tensor(groups, dtype=torch.int32), images_per_batch=3, max_regions=4)
    _check_plan(plan, groups, 3, 4)
    assert [p for b in plan for p in b if p[0] == 2] == [(2, [3, 4, 5, 6]), (2, [7])]  # 5 rows > 4: split, consecutive batches
    plan = dataloader.plan_region_batches(groups, images_per_batch=8, max_regions=3)
    _check_plan(plan, groups, 8, 3)
    plan = dataloader.plan_region_batches(groups, images_per_batch=1, max_regions=100)
    _check_plan(plan, groups, 1, 100)
    assert len(plan) == 5
    assert dataloader.plan_region_batches([], 4) == []
    with pytest.raises(ValueError):
        dataloader.plan_region_batches(groups, 0)


class _StubModel:
    device = torch.device("cpu")

    class image_encoder:
        cfg = dict(img=64, patch=16, out=8)

    def _resolve_dtype(self):
        return torch.float32

    def packed(self, T):
        return {}


def _stub_device_parts(monkeypatch, calls):
    """CPU stand-ins: the "encoder" gives image b the constant tokens b + 1 (as the image's first pixel says), pooling follows the
    definition in plain torch."""
    from cor_amd import engine, ops

    def sam_encoder(W, img, cfg, T):
        calls.append(img.shape[0])
        g = cfg["img"] // cfg["patch"]
        return img[:, 0, 0, 0].reshape(-1, 1, 1).expand(-1, g * g, cfg["out"]).reshape(-1, cfg["out"]).contiguous()

    def bilinear(x, OH, OW, clamp01=False):
        return torch.nn.functional.interpolate(x, size=(OH, OW), mode="bilinear", align_corners=False)

    def region_pool(tokens, masks, off, B, P, D, out_dtype=torch.float32, clamp01=False, l2norm=False):
        tok = tokens.reshape(B, P, D)
        m = masks.clamp(0, 1) if clamp01 else masks
        img_of = torch.repeat_interleave(torch.arange(B), (off[1:] - off[:-1]).long())
        out = torch.einsum("rp,rpd->rd", m, tok[img_of]) / (m.sum(1, keepdim=True) + 1e-8)
        # (no normalisation: the stub keeps the image's constant visible in the row)
        return out.to(out_dtype)

    monkeypatch.setattr(engine, "sam_encoder", sam_encoder)
    monkeypatch.setattr(ops, "bilinear", bilinear)
    monkeypatch.setattr(ops, "region_pool", region_pool)


def _batch(image_values, counts, **extra):
    B, R = len(image_values), sum(counts)
    img = torch.zeros(B, 3, 64, 64)
    for b, v in enumerate(image_values):
        img[b] = v
    off = torch.tensor([0] + list(torch.tensor(counts).cumsum(0).tolist()), dtype=torch.int32)
    return dict(query_img=img, region_masks=torch.ones(R, 1, 8, 8), region_offsets=off, **extra)


def test_build_gallery_regions_host_logic(monkeypatch):
    from cor_amd import retrieval
    calls = []
    _stub_device_parts(monkeypatch, calls)
    model = _StubModel()
    # two batches: images valued 1, 2, 3 with 2, 0, 1 regions, then images 4, 5 with 1, 3 regions
    rows, groups = retrieval.build_gallery_regions(model, [_batch([1., 2., 3.], [2, 0, 1]), _batch([4., 5.], [1, 3])], dtype=torch.float32)
    assert calls == [3, 2]                                                             # one encoder call per batch
    assert rows.shape == (7, 8) and groups.dtype == torch.int32
    assert groups.tolist() == [0, 0, 2, 3, 4, 4, 4]                                    # a running count of the images seen
    assert torch.allclose(rows[:, 0], torch.tensor([1., 1., 3., 4., 5., 5., 5.]))
    # image ids and row positions given: rows and groups come back permuted by row_index
    calls.clear()
    b1 = _batch([1., 2., 3.], [2, 0, 1], image_ids=torch.tensor([10, 11, 12]), row_index=torch.tensor([6, 0, 3]))
    b2 = _batch([4., 5.], [1, 3], image_ids=[13, 14], row_index=[1, 5, 2, 4])
    rows, groups = retrieval.build_gallery_regions(model, iter([b1, b2]), dtype=torch.float16)
    assert calls == [3, 2] and rows.dtype == torch.float16
    assert groups.tolist() == [10, 13, 14, 12, 14, 14, 10]
    assert rows[:, 0].float().tolist() == [1., 4., 5., 3., 5., 5., 1.]
    # not a permutation: a repeated position, a position out of range, a missing index in one batch
    for bad in ([1, 5, 2, 2], [1, 5, 2, 7]):
        with pytest.raises(ValueError):
            retrieval.build_gallery_regions(model, [b1, dict(b2, row_index=bad)])
    with pytest.raises(ValueError):
        retrieval.build_gallery_regions(model, [b1, _batch([4., 5.], [1, 3])])
    with pytest.raises(ValueError):                                                    # offsets that do not end at R
        retrieval.build_gallery_regions(model, [dict(_batch([1.], [2]), region_offsets=torch.tensor([0, 1], dtype=torch.int32))])
    rows, groups = retrieval.build_gallery_regions(model, [])
    assert rows.shape == (0, 8) and groups.shape == (0,)

"""Distinct-group gallery top-k (cor_similarity_topk_distinct / ops.similarity_topk_distinct): every row has a group id (the source
image of a region), a group's representative is its best allowed row by (chain score desc, index asc), the result is the k best
representatives. Every result is held BITWISE (scores and indices, ties and the (-inf, -1) tail included) to the definition computed with
the CPU fmaf-chain oracle (oracle.retrieval.similarity_topk_chain): chain-rank the allowed rows, keep the first row of each group, keep
the first k. With at most R rows per group the k best representatives lie within the first k * R rows of the chain ranking."""
import json
import socket

import numpy as np
import pytest
import torch

from oracle import retrieval as oret

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
NINF = float("-inf")


def _ops():
    from cor_amd import ops, _native as nat
    return ops, nat


def _unit(rng, n, C):
    return torch.nn.functional.normalize(torch.from_numpy(rng.standard_normal((n, C), dtype=np.float32)), dim=-1)


def _data(Bq, Ng, gdt, C=256, seed=0):
    """random unit rows with planted exact duplicates: rows 3 = 5 and 17 = Ng - 200 = Ng - 1; queries 0 and 1 point at them"""
    rng = np.random.default_rng(Bq + Ng + C + seed)
    Q = _unit(rng, Bq, C)
    G = _unit(rng, Ng, C).to(gdt)
    G[5] = G[3]
    if Ng > 300:
        G[Ng - 1] = G[17]; G[Ng - 200] = G[17]
    Q[0] = torch.nn.functional.normalize(G[3].float(), dim=-1)
    if Bq > 1:
        Q[1] = torch.nn.functional.normalize(G[17].float(), dim=-1)
    return Q, G, rng


def _groups(layout, Ng, rng):
    """(group ids int32[Ng], R = the most rows any group holds)"""
    runs = np.repeat(np.arange(Ng), rng.integers(1, 9, Ng))[:Ng]        # image ids: runs of 1-8 consecutive rows
    if layout == "runs":
        g = runs
    elif layout == "perm":                                              # the same ids, regions of one image far apart
        g = runs[rng.permutation(Ng)]
    elif layout == "dup_in":                                            # every planted duplicate set inside ONE group
        g = runs.copy(); g[5] = g[3]
        if Ng > 300:
            g[Ng - 1] = g[17]; g[Ng - 200] = g[17]
    elif layout == "dup_across":                                        # ... and spread over different groups
        g = runs + 10; g[3], g[5], g[17] = 0, 1, 2
        if Ng > 300:
            g[Ng - 200], g[Ng - 1] = 3, 4
    elif layout == "own":
        g = np.arange(Ng)
    elif layout == "negative":
        g = -1 - rng.integers(0, 5, Ng)                                 # all negative (values repeat): every row its own group
    else:
        raise ValueError(layout)
    R = 1 if layout == "negative" else int(np.bincount(g - g.min()).max())
    return torch.from_numpy(g.astype(np.int32)), R


def _chain(Q, G, k, margin=2e-4):
    Qr = Q if G.dtype == F32 else Q.to(G.dtype).float()
    return oret.similarity_topk_chain(Qr, G.float(), k, margin=margin)


def _dedupe(s, i, groups, k):
    """ranked rows (s, i) of one query -> first row of each group (negative id: its own), first k, (-inf, -1) tail"""
    rs = torch.full((k,), NINF); ri = torch.full((k,), -1, dtype=torch.int64)
    seen, n = set(), 0
    for sj, ij in zip(s.tolist(), i.tolist()):
        if ij < 0:
            continue
        g = int(groups[ij])
        key = g if g >= 0 else ("row", ij)
        if key in seen:
            continue
        seen.add(key)
        rs[n] = sj; ri[n] = ij; n += 1
        if n == k:
            break
    return rs, ri


def _oracle(Q, G, k, groups, R, rl=None, ql=None, mode="eq"):
    """the definition: chain-rank each query's allowed rows (the first k * R of them suffice), first row of each group, first k"""
    Bq, Ng = Q.shape[0], G.shape[0]
    rs = torch.full((Bq, k), NINF); ri = torch.full((Bq, k), -1, dtype=torch.int64)
    classes = [(torch.ones(Bq, dtype=torch.bool), torch.arange(Ng))] if ql is None else []
    if ql is not None and mode == "ne" and rl is groups:
        # the filter excludes ONE group (<= R rows): rank the whole shard R rows deeper and drop them
        s, i = _chain(Q, G, min(k * R + R, Ng))
        for b in range(Bq):
            keep = torch.ones_like(i[b], dtype=torch.bool) if ql[b] < 0 else rl[i[b]] != ql[b]
            rs[b], ri[b] = _dedupe(s[b][keep], i[b][keep], groups, k)
        return rs, ri
    if ql is not None:
        if (ql < 0).any():
            classes.append((ql < 0, torch.arange(Ng)))
        for lab in torch.unique(ql[ql >= 0]).tolist():
            rows = ((rl == lab) if mode == "eq" else (rl != lab)).nonzero().flatten()
            classes.append((ql == lab, rows))
    for qsel, rows in classes:
        if rows.numel() == 0 or not qsel.any():
            continue
        s, i = _chain(Q[qsel], G[rows], min(k * R, rows.numel()))
        for j, b in enumerate(qsel.nonzero().flatten().tolist()):
            rs[b], ri[b] = _dedupe(s[j], rows[i[j]], groups, k)
    return rs, ri


def _assert_bitwise(s, i, rs, ri, g_offset):
    s, i = s.cpu(), i.cpu()
    exp = torch.where(ri >= 0, ri + g_offset, ri)
    mism = int((i != exp).sum())
    bits = int((s.view(torch.int32) != rs.view(torch.int32)).sum())
    assert mism == 0, f"{mism} of {ri.numel()} indices differ from the definition on the chain oracle"
    assert bits == 0, f"{bits} of {ri.numel()} scores are not bit-identical to the chain oracle"


def _run(Q, G, k, groups, rl=None, ql=None, mode="eq", g_offset=0, flags=0):
    ops, _ = _ops()
    d = lambda t: None if t is None else t.to(DEV)
    return ops.similarity_topk_distinct(Q.to(DEV), G.to(DEV), k, groups.to(DEV), d(rl), d(ql), mode=mode, g_offset=g_offset, flags=flags)


def _check(Q, G, k, groups, R, rl=None, ql=None, mode="eq", g_offset=1000):
    """on-plan: no query may overflow (COR_TOPK_NO_FALLBACK exposes -2), and the result is the definition, bitwise"""
    _, nat = _ops()
    s, i = _run(Q, G, k, groups, rl, ql, mode, g_offset, flags=nat.TOPK_NO_FALLBACK)
    over = int((i == -2).any(dim=1).sum())
    assert over == 0, f"{over} of {Q.shape[0]} queries overflowed their candidate lists"
    _assert_bitwise(s, i, *_oracle(Q, G, k, groups, R, rl, ql, mode), g_offset)
    return s, i


SHAPES = [(32, 100000, 10), (512, 125000, 10), (512, 12500, 16), (64, 4097, 1), (300, 70001, 100), (7, 200, 256)]
LAYOUTS = ["runs", "perm", "dup_in", "dup_across"]
GRID = []
for _si, _sh in enumerate(SHAPES):
    for _di, _gdt in enumerate((F32, BF16, F16)):
        GRID.append(_sh + (_gdt, 256, LAYOUTS[(_si + _di) % 4]))
        GRID.append(_sh + (_gdt, 256, LAYOUTS[(_si + _di + 2) % 4]))
GRID += [(64, 20000, 50, BF16, 128, "runs"), (64, 20000, 50, F16, 128, "dup_in"), (33, 3001, 10, BF16, 128, "dup_across"),
         (40, 9000, 20, F32, 64, "perm"), (40, 9000, 20, F16, 64, "dup_in"),
         # k = 256 on shards beyond the tiny-shard plan: the narrowest sample stride (1024 / k = 4), the most distinct sampled groups asked for
         (64, 50000, 256, BF16, 256, "runs"), (40, 30000, 256, F32, 256, "perm"), (48, 40000, 256, F16, 128, "dup_in")]


@pytest.mark.parametrize("Bq,Ng,k,gdt,C,layout", GRID)
def test_distinct_topk_matches_the_definition(Bq, Ng, k, gdt, C, layout):
    Q, G, rng = _data(Bq, Ng, gdt, C=C)
    groups, R = _groups(layout, Ng, rng)
    s, i = _check(Q, G, k, groups, R)
    i = i.cpu()
    if layout == "dup_in":                       # rows 3 = 5 share a group: the lower index represents it, once
        assert i[0, 0] == 1003 and 1005 not in i[0].tolist()
    if layout == "dup_across" and k >= 2:        # ... in two groups: both, in index order
        assert i[0, :2].tolist() == [1003, 1005]


@pytest.mark.parametrize("layout", ["own", "negative"])
@pytest.mark.parametrize("Bq,Ng,k,gdt,C", [(32, 100000, 10, BF16, 256), (300, 70001, 100, F32, 256), (512, 12500, 16, F16, 256), (64, 20000, 50, BF16, 128)])
def test_one_group_per_row_equals_similarity_topk(Bq, Ng, k, gdt, C, layout):
    ops, nat = _ops()
    Q, G, rng = _data(Bq, Ng, gdt, C=C, seed=2)
    groups, _ = _groups(layout, Ng, rng)
    s, i = _run(Q, G, k, groups, g_offset=5, flags=nat.TOPK_NO_FALLBACK)          # on plan: no query may overflow
    over = int((i == -2).any(dim=1).sum())
    assert over == 0, f"{over} of {Bq} queries overflowed their candidate lists"
    s0, i0 = ops.similarity_topk(Q.to(DEV), G.to(DEV), k, g_offset=5)
    assert torch.equal(i, i0) and torch.equal(s.view(torch.int32), s0.view(torch.int32))


def _oracle_per_group(Q, G, k, groups):
    """few, large groups: chain top-1 of each group's rows, then rank by (score desc, index asc)"""
    Bq = Q.shape[0]
    reps_s, reps_i = [], []
    for g in torch.unique(groups).tolist():
        rows = (groups == g).nonzero().flatten()
        s, i = _chain(Q, G[rows], 1)
        reps_s.append(s[:, 0]); reps_i.append(rows[i[:, 0]])
    S, I = torch.stack(reps_s, 1), torch.stack(reps_i, 1)
    rs = torch.full((Bq, k), NINF); ri = torch.full((Bq, k), -1, dtype=torch.int64)
    for b in range(Bq):
        order = np.lexsort((I[b].numpy(), -S[b].double().numpy()))[:k]
        rs[b, :len(order)] = S[b][order]; ri[b, :len(order)] = I[b][order]
    return rs, ri


@pytest.mark.parametrize("Bq,Ng,k,gdt,ngroups,on_plan", [(7, 200, 256, F32, 5, True), (16, 2000, 50, BF16, 12, True), (8, 100000, 10, BF16, 5, False),
                                                         (8, 30000, 20, F32, 7, False)])
def test_fewer_groups_than_k_ends_in_the_tail(Bq, Ng, k, gdt, ngroups, on_plan):
    """Fewer than k groups: all of them, then (-inf, -1). A shard of up to SLW = 2048 rows ranks all its rows on plan; a large shard with
    fewer than k groups has no finite threshold (the best row of EVERY group is wanted, wherever it scores), so it is the paging fallback's
    case by construction and is compared through it. That path pages the whole shard (Ng^2 / 410 row scores per query; measured 545 ms per
    call for 8 x 100 000 rows in 5 groups), so these shards stay small."""
    _, nat = _ops()
    Q, G, rng = _data(Bq, Ng, gdt, seed=5)
    groups = torch.from_numpy(rng.integers(0, ngroups, Ng).astype(np.int32))
    s, i = _run(Q, G, k, groups, g_offset=9, flags=nat.TOPK_NO_FALLBACK if on_plan else 0)
    _assert_bitwise(s, i, *_oracle_per_group(Q, G, k, groups), 9)
    assert (i.cpu()[:, ngroups:] == -1).all() and (i.cpu()[:, :ngroups] >= 9).all()


@pytest.mark.parametrize("Bq,Ng,k,gdt", [(32, 100000, 10, BF16), (512, 125000, 10, F16), (300, 70001, 100, F32), (512, 12500, 16, BF16), (64, 20000, 50, F16)])
def test_distinct_with_the_own_image_excluded(Bq, Ng, k, gdt):
    """the evaluation protocol: one hit per image and not the query's own image: the SAME tensor filters (ne) and groups; every 7th query unrestricted"""
    Q, G, rng = _data(Bq, Ng, gdt, seed=6)
    groups, R = _groups("runs", Ng, rng)
    ql = groups[torch.from_numpy(rng.integers(0, Ng, Bq))].clone()
    ql[0] = groups[3]; ql[::7] = -1
    _check(Q, G, k, groups, R, rl=groups, ql=ql, mode="ne")


@pytest.mark.parametrize("Bq,Ng,k,gdt", [(32, 100000, 10, F16), (512, 125000, 10, BF16), (300, 70001, 100, BF16), (64, 20000, 50, F32)])
def test_distinct_inside_a_class_filter(Bq, Ng, k, gdt):
    """different tensors: eq on 16 classes, grouped by image (an image's regions carry different classes)"""
    Q, G, rng = _data(Bq, Ng, gdt, seed=7)
    groups, R = _groups("perm", Ng, rng)
    rl = torch.from_numpy(rng.integers(0, 16, Ng).astype(np.int32))
    ql = torch.from_numpy(rng.integers(0, 16, Bq).astype(np.int32)); ql[::7] = -1
    _check(Q, G, k, groups, R, rl=rl, ql=ql, mode="eq")


@pytest.mark.parametrize("gdt", [BF16, F16])
@pytest.mark.parametrize("k", [10, 100])
def test_distinct_topk_1m_rows(gdt, k):
    Q, G, rng = _data(512, 1000000, gdt, seed=3)
    groups, R = _groups("runs", 1000000, rng)
    _check(Q, G, k, groups, R, g_offset=7)


@pytest.mark.parametrize("case,k", [("one_group", 10), ("one_group", 100), ("many_groups", 10), ("many_groups", 256), ("single", 50)])
@pytest.mark.parametrize("gdt", [BF16, F32])
def test_overflow_fallback_is_exact(case, k, gdt):
    """Ordinary inputs that overflow the candidate lists by construction: 5 000 identical rows in one group / in 5 000 groups among 20 000
    rows, and 3 000 rows of one single group. The paging fallback ranks them on the device, bitwise the definition."""
    _, nat = _ops()
    Ng = 3000 if case == "single" else 20000
    Q, G, rng = _data(16, Ng, gdt, seed=8)
    if case == "single":
        groups = torch.full((Ng,), 4, dtype=torch.int32)
        rs, ri = _oracle_per_group(Q, G, k, groups)
    else:
        groups, R = _groups("runs", Ng, rng)
        groups = groups + 6000
        dup = torch.from_numpy(rng.permutation(Ng)[:5000]).sort().values
        G[dup] = G[dup[0]].clone()
        Q[2] = torch.nn.functional.normalize(G[dup[0]].float(), dim=-1)
        groups[dup] = 77 if case == "one_group" else torch.arange(5000, dtype=torch.int32)
        s_all, i_all = _chain(Q, G, min(Ng, 5000 + 9 * k))
        rs = torch.full((16, k), NINF); ri = torch.full((16, k), -1, dtype=torch.int64)
        for b in range(16):
            rs[b], ri[b] = _dedupe(s_all[b], i_all[b], groups, k)
    s, i = _run(Q, G, k, groups, g_offset=11)
    _assert_bitwise(s, i, rs, ri, 11)
    _, raw = _run(Q, G, k, groups, g_offset=11, flags=nat.TOPK_NO_FALLBACK)
    raw = raw.cpu()
    over = (raw == -2).any(dim=1)
    assert bool(over.any()) and bool((raw[over] == -2).all())          # the fallback did run, and the marker fills every slot


def test_distinct_topk_argument_checks():
    ops, nat = _ops()
    lib = nat.load()
    Q, G, rng = _data(8, 5000, BF16, seed=3)
    Qd, Gd = Q.to(DEV), G.to(DEV)
    rg = torch.arange(5000, dtype=torch.int32, device=DEV) // 3
    rl = torch.zeros(5000, dtype=torch.int32, device=DEV); ql = torch.zeros(8, dtype=torch.int32, device=DEV)
    for bad in (0, 257):
        with pytest.raises(ValueError):
            ops.similarity_topk_distinct(Qd, Gd, bad, rg)
    with pytest.raises(ValueError):
        ops.similarity_topk_distinct(Qd, Gd, 10, rg, rl, ql, mode="lt")
    with pytest.raises(ValueError):
        ops.similarity_topk_distinct(Qd, Gd, 10, rg[:4999])
    with pytest.raises(ValueError, match="similarity_topk_distinct: row_groups"):
        ops.similarity_topk_distinct(Qd, Gd, 10, rg.float())
    with pytest.raises(ValueError):
        ops.similarity_topk_distinct(Qd, Gd, 10, rg, rl, None)
    with pytest.raises(ValueError):
        ops.similarity_topk_distinct(Qd, Gd, 10, rg, rl, ql[:7])
    assert lib.cor_topk_distinct_workspace_bytes(8, 5000, 257) == nat.EINVAL
    ws = torch.empty((lib.cor_topk_distinct_workspace_bytes(8, 5000, 10),), dtype=torch.uint8, device=DEV)
    out_s = torch.empty((8, 10), dtype=torch.float32, device=DEV); out_i = torch.empty((8, 10), dtype=torch.int64, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def call(rgp, rlp, qlp, mode, flags):
        return lib.cor_similarity_topk_distinct(Qd.data_ptr(), Gd.data_ptr(), nat.BF16, 8, 5000, 256, 10, 0, rgp, rlp, qlp, mode, out_s.data_ptr(),
                                                out_i.data_ptr(), ws.data_ptr(), flags, stream)
    assert call(0, None, None, nat.FILTER_EQ, 0) == nat.EINVAL
    assert call(rg.data_ptr(), rl.data_ptr(), None, nat.FILTER_EQ, 0) == nat.EINVAL
    assert call(rg.data_ptr(), None, ql.data_ptr(), nat.FILTER_EQ, 0) == nat.EINVAL
    assert call(rg.data_ptr(), rl.data_ptr(), ql.data_ptr(), 2, 0) == nat.EINVAL
    assert call(rg.data_ptr(), None, None, nat.FILTER_EQ, nat.TOPK_FORCE_LISTS) == nat.ENOSUPPORT
    assert call(rg.data_ptr(), None, None, nat.FILTER_EQ, nat.TOPK_WAVE_FINAL) == nat.ENOSUPPORT
    assert call(rg.data_ptr() + 4, None, None, nat.FILTER_EQ, 0) == nat.EINVAL                       # 16-byte alignment of the row vectors
    assert call(rg.data_ptr(), rl.data_ptr() + 8, ql.data_ptr(), nat.FILTER_EQ, 0) == nat.EINVAL
    assert call(rg.data_ptr(), None, None, nat.FILTER_EQ, 0) == 0
    assert call(rg.data_ptr(), rl.data_ptr(), ql.data_ptr(), nat.FILTER_NE, 0) == 0
    torch.cuda.synchronize()
    assert (out_i == -1).all()                                         # every row carries the excluded label


def test_distinct_topk_replays_under_graph_capture():
    ops, _ = _ops()
    Q, G, rng = _data(64, 30000, BF16, seed=6)
    groups, _ = _groups("runs", 30000, rng)
    Qd, Gd, gd = Q.to(DEV), G.to(DEV), groups.to(DEV)
    s0, i0 = ops.similarity_topk_distinct(Qd, Gd, 50, gd)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.similarity_topk_distinct(Qd, Gd, 50, gd)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        s1, i1 = ops.similarity_topk_distinct(Qd, Gd, 50, gd)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(i1, i0) and torch.equal(s1.view(torch.int32), s0.view(torch.int32))


def test_distinct_shard_search_and_persistence(tmp_path):
    from cor_amd import ops, retrieval
    Q, G, rng = _data(24, 30000, BF16, seed=8)
    groups, R = _groups("runs", 30000, rng)
    Qd, Gd = Q.to(DEV), G.to(DEV)
    shard = retrieval.GalleryShard(Gd, offset=100, labels=groups, groups=groups)
    s0, i0 = shard.search(Qd, 50, distinct=True)
    _assert_bitwise(s0, i0, *_oracle(Q, G, 50, groups, R), 100)
    ql = groups[torch.from_numpy(rng.integers(0, 30000, 24))]
    s1, i1 = shard.search(Qd, 50, query_labels=ql.to(DEV), mode="ne", distinct=True)
    _assert_bitwise(s1, i1, *_oracle(Q, G, 50, groups, R, groups, ql, "ne"), 100)
    g_of = retrieval.groups_of(i1.cpu() - 100, groups)
    assert all(len(set(r)) == 50 for r in g_of.tolist()) and not (g_of == ql.unsqueeze(1)).any()
    sd, id_ = retrieval.distributed_search(Qd, shard, 50, distinct=True)
    assert torch.equal(id_, i0.cpu()) and torch.equal(sd.view(torch.int32), s0.cpu().view(torch.int32))
    with pytest.raises(ValueError):
        retrieval.GalleryShard(Gd).search(Qd, 10, distinct=True)
    e_s, e_i = retrieval.GalleryShard(Gd[:0], groups=groups[:0]).search(Qd, 10, distinct=True)
    assert (e_i == -1).all() and torch.isneginf(e_s).all()
    path = str(tmp_path / "gal")
    retrieval.save_gallery(path, G[:1001], world=2, groups=groups[:1001])
    man = json.load(open(path + ".manifest.json"))
    assert man["groups"] is True and man["labels"] is False
    for r in range(2):
        lo, hi = retrieval.shard_bounds(1001, 2, r)
        sh = retrieval.load_gallery_shard(path, r, DEV)
        assert sh.offset == lo and sh.labels is None and torch.equal(sh.groups.cpu(), groups[lo:hi])
        s_r, i_r = sh.search(Qd, 10, distinct=True)
        _assert_bitwise(s_r, i_r, *_oracle(Q, G[lo:hi], 10, groups[lo:hi], R), lo)
    retrieval.save_gallery(path + "2", G[:100], world=2)
    assert retrieval.load_gallery_shard(path + "2", 1, DEV).groups is None


def test_distinct_distributed_search_on_a_one_rank_rccl_group():
    import torch.distributed as dist
    from cor_amd import retrieval
    assert not dist.is_initialized()
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]
    dev = torch.device(DEV)
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=dev)
    try:
        Q, G, rng = _data(5, 12500, BF16, seed=9)
        groups, R = _groups("runs", 12500, rng)
        shard = retrieval.GalleryShard(G.to(dev), offset=100, labels=groups, groups=groups)
        Qd = Q.to(dev)
        ql = groups[torch.from_numpy(rng.integers(0, 12500, 5))].to(dev)
        for kw in (dict(), dict(query_labels=ql, filter_mode="ne")):
            s0, i0 = shard.search(Qd, 10, query_labels=kw.get("query_labels"), mode=kw.get("filter_mode", "eq"), distinct=True)
            s1, i1 = retrieval.distributed_search(Qd, shard, 10, max_local=8, always_collective=True, distinct=True, **kw)
            s2, i2 = retrieval.distributed_search(Qd, shard, 10, max_local=8, dst=None, always_collective=True, distinct=True, **kw)
            s3, i3 = retrieval.distributed_search(Qd, shard, 10, max_local=8, always_collective=True, defer=True, distinct=True, **kw).result()
            for s_, i_ in ((s1, i1), (s2, i2), (s3, i3)):
                assert torch.equal(i_, i0.cpu()) and torch.equal(s_.view(torch.int32), s0.cpu().view(torch.int32))
        sp, ip = retrieval.distributed_search(Qd, shard, 10, max_local=8, always_collective=True)     # the plain call beside it
        s0, i0 = shard.search(Qd, 10)
        assert torch.equal(ip, i0.cpu()) and torch.equal(sp.view(torch.int32), s0.cpu().view(torch.int32))
    finally:
        dist.destroy_process_group()

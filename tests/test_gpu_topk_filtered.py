"""Filtered gallery top-k (cor_similarity_topk_filtered / ops.similarity_topk_filtered): per-query label filters (eq: restrict to a
class or subset, ne: exclude a source such as the query's own image) inside the wide route's scans. Every result is held BITWISE (scores
and indices, ties and the (-inf, -1) tail included) to the CPU fmaf-chain oracle (oracle.retrieval.similarity_topk_chain) run on the
allowed rows, for fp32, bf16 and fp16 galleries; random and class-sorted galleries stay off the overflow path."""
import json

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
    rng = np.random.default_rng(Bq + Ng + C + seed)
    Q = _unit(rng, Bq, C)
    G = _unit(rng, Ng, C).to(gdt)
    G[5] = G[3]
    if Ng > 300:
        G[Ng - 1] = G[17]; G[Ng - 200] = G[17]
    return Q, G, rng


def _labels(layout, Ng, Bq, rng):
    """(row labels int32[Ng], query labels int32[Bq], longest run of one row label for 'runs'); every 7th query is unrestricted"""
    run = 0
    if layout.startswith("uniform"):
        n = int(layout[7:]); rl = rng.integers(0, n, Ng); ql = rng.integers(0, n, Bq)
    elif layout == "blocks16":                                         # a class-sorted gallery: 16 contiguous blocks
        rl = (np.arange(Ng) * 16) // Ng; ql = rng.integers(0, 16, Bq)
    elif layout == "skew":                                             # class 0 holds 90 % of the rows
        rl = np.where(rng.random(Ng) < 0.9, 0, rng.integers(1, 9, Ng)); ql = rng.integers(0, 9, Bq)
    else:                                                              # "runs": image ids, runs of 1-8 rows
        rl = np.repeat(np.arange(Ng), rng.integers(1, 9, Ng))[:Ng]; ql = rl[rng.integers(0, Ng, Bq)]; run = 8
    ql = ql.copy(); ql[::7] = -1
    return torch.from_numpy(rl.astype(np.int32)), torch.from_numpy(ql.astype(np.int32)), run


def _chain(Q, G, k, margin=2e-4):
    Qr = Q if G.dtype == F32 else Q.to(G.dtype).float()
    return oret.similarity_topk_chain(Qr, G.float(), k, margin=margin)


def _oracle(Q, G, k, rl, ql, mode, run=0, margin=2e-4):
    """chain top-k of each query's allowed rows: shard-local indices, (-inf, -1) tail"""
    Bq, Ng = Q.shape[0], G.shape[0]
    rs = torch.full((Bq, k), NINF); ri = torch.full((Bq, k), -1, dtype=torch.int64)
    free = ql < 0
    if free.any():
        s, i = _chain(Q[free], G, min(k, Ng), margin)
        rs[free, :s.shape[1]] = s; ri[free, :s.shape[1]] = i
    if mode == "ne" and run:                       # short label runs: top k + run, drop the query's own label, keep k
        lab = (~free).nonzero().flatten()
        if lab.numel():
            s, i = _chain(Q[lab], G, min(k + run, Ng), margin)
            own = rl[i] == ql[lab].unsqueeze(1)
            for j, b in enumerate(lab.tolist()):
                sj, ij = s[j][~own[j]][:k], i[j][~own[j]][:k]
                rs[b, :sj.shape[0]] = sj; ri[b, :ij.shape[0]] = ij
        return rs, ri
    for lab in torch.unique(ql[~free]).tolist():
        qsel = ql == lab
        rows = ((rl == lab) if mode == "eq" else (rl != lab)).nonzero().flatten()
        if rows.numel() == 0:
            continue
        s, i = _chain(Q[qsel], G[rows], min(k, rows.numel()), margin)
        rs[qsel, :s.shape[1]] = s; ri[qsel, :s.shape[1]] = rows[i]
    return rs, ri


def _assert_bitwise(s, i, rs, ri, g_offset):
    s, i = s.cpu(), i.cpu()
    exp = torch.where(ri >= 0, ri + g_offset, ri)
    mism = int((i != exp).sum())
    bits = int((s.view(torch.int32) != rs.view(torch.int32)).sum())
    assert mism == 0, f"{mism} of {ri.numel()} indices differ from the chain oracle on the allowed rows"
    assert bits == 0, f"{bits} of {ri.numel()} scores are not bit-identical to the chain oracle"


def _run(Q, G, k, rl, ql, mode, g_offset=0, flags=0):
    ops, _ = _ops()
    return ops.similarity_topk_filtered(Q.to(DEV), G.to(DEV), k, rl.to(DEV), ql.to(DEV), mode=mode, g_offset=g_offset, flags=flags)


SHAPES = [(32, 100000, 10), (512, 125000, 10), (512, 12500, 16), (64, 4097, 1), (300, 70001, 100), (7, 200, 256)]
EQ_LAYOUTS = ["uniform4", "uniform16", "uniform64", "blocks16", "skew"]
NE_LAYOUTS = ["runs", "uniform4"]
GRID = []
for _si, _sh in enumerate(SHAPES):
    for _di, _gdt in enumerate((F32, BF16, F16)):
        GRID.append(_sh + (_gdt, 256, "eq", EQ_LAYOUTS[(_si + _di) % len(EQ_LAYOUTS)]))
        GRID.append(_sh + (_gdt, 256, "ne", NE_LAYOUTS[(_si + _di) % len(NE_LAYOUTS)]))
GRID += [(64, 20000, 50, BF16, 128, "eq", "blocks16"), (64, 20000, 50, F16, 128, "ne", "runs"), (33, 3001, 10, BF16, 128, "eq", "uniform16")]


@pytest.mark.parametrize("Bq,Ng,k,gdt,C,mode,layout", GRID)
def test_filtered_topk_bitwise_vs_chain_oracle(Bq, Ng, k, gdt, C, mode, layout):
    _, nat = _ops()
    Q, G, rng = _data(Bq, Ng, gdt, C=C)
    rl, ql, run = _labels(layout, Ng, Bq, rng)
    s, i = _run(Q, G, k, rl, ql, mode, g_offset=1000)
    rs, ri = _oracle(Q, G, k, rl, ql, mode, run)
    _assert_bitwise(s, i, rs, ri, 1000)
    _, raw = _run(Q, G, k, rl, ql, mode, g_offset=1000, flags=nat.TOPK_NO_FALLBACK)     # random and clustered labels: no overflow
    assert int((raw == -2).any(dim=1).sum()) == 0


@pytest.mark.parametrize("gdt", [BF16, F16])
@pytest.mark.parametrize("layout", ["uniform16", "blocks16"])
@pytest.mark.parametrize("k", [10, 100])
def test_filtered_topk_1m_rows(gdt, layout, k):
    """512 x 1M, eq over 16 classes, uniform and class-sorted (contiguous blocks: the case an unsplit sample and per-slice streams
    would send to the brute force)."""
    _, nat = _ops()
    Q, G, rng = _data(512, 1000000, gdt, seed=3)
    rl, ql, _ = _labels(layout, 1000000, 512, rng)
    s, i = _run(Q, G, k, rl, ql, "eq", g_offset=7)
    _assert_bitwise(s, i, *_oracle(Q, G, k, rl, ql, "eq"), 7)
    _, raw = _run(Q, G, k, rl, ql, "eq", g_offset=7, flags=nat.TOPK_NO_FALLBACK)
    assert int((raw == -2).any(dim=1).sum()) == 0


@pytest.mark.parametrize("gdt", [F32, BF16, F16])
@pytest.mark.parametrize("mode", ["eq", "ne"])
def test_filtered_topk_planted_excluded_copies(gdt, mode):
    """Every query has 8 exact copies of itself in the gallery that its filter excludes (ne: they carry the query's own label; eq: they
    are in another class). An unmasked sample pass would put tau_q at ~1 above every allowed row."""
    _, nat = _ops()
    Bq, Ng, k = 64, 50000, 5
    Q, G, rng = _data(Bq, Ng, gdt, seed=11)
    pos = torch.from_numpy(rng.choice(Ng, Bq * 8, replace=False)).view(Bq, 8)
    for b in range(Bq):
        G[pos[b]] = Q[b].to(gdt)
    if mode == "ne":
        rl = torch.arange(Ng, dtype=torch.int32) + 1000                 # every other row its own image
        ql = torch.arange(Bq, dtype=torch.int32) + 100000
        for b in range(Bq):
            rl[pos[b]] = int(ql[b])
        run = 8
    else:
        rl = torch.from_numpy(rng.integers(0, 8, Ng).astype(np.int32))
        ql = torch.arange(Bq, dtype=torch.int32) % 8
        for b in range(Bq):
            rl[pos[b]] = (int(ql[b]) + 1) % 8
        run = 0
    s, i = _run(Q, G, k, rl, ql, mode)
    _assert_bitwise(s, i, *_oracle(Q, G, k, rl, ql, mode, run), 0)
    ic = i.cpu()
    assert not any(bool(torch.isin(ic[b], pos[b]).any()) for b in range(Bq))      # no query finds its own excluded copies
    _, raw = _run(Q, G, k, rl, ql, mode, flags=nat.TOPK_NO_FALLBACK)
    assert int((raw == -2).any(dim=1).sum()) == 0


# (gdt, C, queries, rows): the record (scan-form) selection kernel, then the entry-list (tile-form) one for fp32 and for C != 256
OVERFLOW_CASES = [(BF16, 256, 40, 60000), (F32, 256, 16, 20000), (F16, 128, 16, 20000)]


@pytest.mark.parametrize("gdt,C,nq,Ng", OVERFLOW_CASES, ids=["bf16-256", "f32-256", "f16-128"])
def test_filtered_topk_overflow_falls_back_over_the_allowed_rows(gdt, C, nq, Ng):
    """6000 identical rows close to query 0, alternating classes 0 / 1; query 0 keeps class 0: 3000 tied allowed rows overflow the short
    list at k = 100, the in-kernel brute force ranks the ALLOWED rows only (the first 100 class-0 copies in index order)."""
    _, nat = _ops()
    k = 100
    rng = np.random.default_rng(5)
    Q = _unit(rng, nq, C)
    row = _unit(rng, 1, C)
    G = _unit(rng, Ng, C)
    G[10000:16000] = torch.nn.functional.normalize(Q[0:1] + 0.05 * row, dim=-1)
    G = G.to(gdt)
    rl = torch.from_numpy(rng.integers(0, 4, Ng).astype(np.int32))
    rl[10000:16000] = torch.arange(6000, dtype=torch.int32) % 2
    ql = torch.from_numpy(rng.integers(0, 4, nq).astype(np.int32)); ql[0] = 0; ql[1::5] = -1
    s, i = _run(Q, G, k, rl, ql, "eq")
    _, raw = _run(Q, G, k, rl, ql, "eq", flags=nat.TOPK_NO_FALLBACK)
    flagged = (raw == -2).all(dim=1).cpu()
    assert bool(flagged[0]) and int(flagged.sum()) < nq
    assert torch.equal(i[0].cpu(), torch.arange(10000, 16000, 2)[:k])
    keep = ~flagged.to(DEV)
    assert torch.equal(raw[keep], i[keep])
    _assert_bitwise(s, i, *_oracle(Q, G, k, rl, ql, "eq", margin=1e-3), 0)


@pytest.mark.parametrize("gdt,C", [(BF16, 256), (F32, 64)])
@pytest.mark.parametrize("k", [10, 100])
def test_filtered_topk_edge_cases(gdt, C, k):
    """An absent class (only the tail), a class with fewer than k rows, a class with exactly one row, unrestricted and labelled queries
    mixed in one call."""
    Q, G, rng = _data(24, 20000, gdt, C=C, seed=2)
    rl = torch.from_numpy(rng.integers(0, 4, 20000).astype(np.int32))
    rl[[11, 500, 9000, 15000, 19999]] = 5
    rl[777] = 6
    ql = torch.from_numpy(rng.integers(0, 4, 24).astype(np.int32))
    ql[0], ql[1], ql[2], ql[3] = 9, 5, 6, -1
    s, i = _run(Q, G, k, rl, ql, "eq", g_offset=3)
    _assert_bitwise(s, i, *_oracle(Q, G, k, rl, ql, "eq"), 3)
    i = i.cpu()
    assert (i[0] == -1).all() and torch.isneginf(s[0]).all()
    assert sorted(i[1, :5].tolist()) == [14, 503, 9003, 15003, 20002] and (i[1, 5:] == -1).all()
    assert i[2, 0] == 780 and (i[2, 1:] == -1).all()


@pytest.mark.parametrize("gdt,C,k", [(BF16, 256, 10), (F32, 256, 10), (BF16, 256, 100), (F16, 128, 64), (F32, 64, 32)])
def test_unrestricted_queries_equal_similarity_topk(gdt, C, k):
    ops, _ = _ops()
    Q, G, rng = _data(100, 30000, gdt, C=C, seed=4)
    rl = torch.from_numpy(rng.integers(0, 16, 30000).astype(np.int32))
    ql = torch.full((100,), -1, dtype=torch.int32)
    s, i = _run(Q, G, k, rl, ql, "ne", g_offset=5)
    s0, i0 = ops.similarity_topk(Q.to(DEV), G.to(DEV), k, g_offset=5)
    assert torch.equal(i, i0) and torch.equal(s.view(torch.int32), s0.view(torch.int32))


def test_filtered_topk_argument_checks():
    ops, nat = _ops()
    lib = nat.load()
    Q, G, rng = _data(8, 5000, BF16, seed=3)
    Qd, Gd = Q.to(DEV), G.to(DEV)
    rl = torch.zeros(5000, dtype=torch.int32, device=DEV); ql = torch.zeros(8, dtype=torch.int32, device=DEV)
    for bad in (0, 257):
        with pytest.raises(ValueError):
            ops.similarity_topk_filtered(Qd, Gd, bad, rl, ql)
    with pytest.raises(ValueError):
        ops.similarity_topk_filtered(Qd, Gd, 10, rl, ql, mode="lt")
    with pytest.raises(ValueError):
        ops.similarity_topk_filtered(Qd, Gd, 10, rl[:4999], ql)
    with pytest.raises(ValueError):
        ops.similarity_topk_filtered(Qd, Gd, 10, rl, ql[:7])
    assert lib.cor_topk_filtered_workspace_bytes(8, 5000, 257) == nat.EINVAL
    ws = torch.empty((lib.cor_topk_filtered_workspace_bytes(8, 5000, 10),), dtype=torch.uint8, device=DEV)
    out_s = torch.empty((8, 10), dtype=torch.float32, device=DEV); out_i = torch.empty((8, 10), dtype=torch.int64, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def call(rlp, qlp, mode, flags):
        return lib.cor_similarity_topk_filtered(Qd.data_ptr(), Gd.data_ptr(), nat.BF16, 8, 5000, 256, 10, 0, rlp, qlp, mode, out_s.data_ptr(),
                                                out_i.data_ptr(), ws.data_ptr(), flags, stream)
    assert call(0, ql.data_ptr(), nat.FILTER_EQ, 0) == nat.EINVAL
    assert call(rl.data_ptr(), 0, nat.FILTER_EQ, 0) == nat.EINVAL
    assert call(rl.data_ptr(), ql.data_ptr(), 2, 0) == nat.EINVAL
    assert call(rl.data_ptr(), ql.data_ptr(), nat.FILTER_EQ, nat.TOPK_FORCE_LISTS) == nat.ENOSUPPORT
    assert call(rl.data_ptr(), ql.data_ptr(), nat.FILTER_EQ, nat.TOPK_WAVE_FINAL) == nat.ENOSUPPORT
    assert call(rl.data_ptr(), ql.data_ptr(), nat.FILTER_NE, 0) == 0
    torch.cuda.synchronize()
    s, i = ops.similarity_topk_filtered(Qd, Gd, 10, rl, ql, mode="ne")
    s2, i2 = ops.similarity_topk_filtered(Qd, Gd, 10, rl, ql, mode="ne", flags=nat.TOPK_FORCE_GLOBAL_THRESHOLD)
    assert (i == -1).all() and torch.equal(i, i2) and torch.equal(s.view(torch.int32), s2.view(torch.int32))


def test_filtered_topk_replays_under_graph_capture():
    """No host synchronisation: a filtered search captured in a graph replays to the eager result."""
    ops, _ = _ops()
    Q, G, rng = _data(64, 30000, BF16, seed=6)
    rl, ql, _ = _labels("uniform16", 30000, 64, rng)
    Qd, Gd, rld, qld = Q.to(DEV), G.to(DEV), rl.to(DEV), ql.to(DEV)
    s0, i0 = ops.similarity_topk_filtered(Qd, Gd, 50, rld, qld)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.similarity_topk_filtered(Qd, Gd, 50, rld, qld)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        s1, i1 = ops.similarity_topk_filtered(Qd, Gd, 50, rld, qld)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(i1, i0) and torch.equal(s1.view(torch.int32), s0.view(torch.int32))


def test_filtered_shard_search_distributed_search_and_persistence(tmp_path):
    import torch.distributed as dist
    from cor_amd import ops, retrieval
    Q, G, rng = _data(24, 30000, BF16, seed=8)
    rl, ql, _ = _labels("uniform16", 30000, 24, rng)
    Qd, Gd = Q.to(DEV), G.to(DEV)
    shard = retrieval.GalleryShard(Gd, offset=100, labels=rl)
    s0, i0 = shard.search(Qd, 50, query_labels=ql.to(DEV), mode="eq")
    sd, id_ = ops.similarity_topk_filtered(Qd, Gd, 50, rl.to(DEV), ql.to(DEV), g_offset=100)
    assert torch.equal(i0, id_) and torch.equal(s0.view(torch.int32), sd.view(torch.int32))
    _assert_bitwise(s0, i0, *_oracle(Q, G, 50, rl, ql, "eq"), 100)
    assert not dist.is_initialized()
    s1, i1 = retrieval.distributed_search(Qd, shard, 50, query_labels=ql.to(DEV), filter_mode="eq")
    s2, i2 = retrieval.distributed_search(Qd, shard, 50, query_labels=ql.to(DEV), filter_mode="eq", defer=True).result()
    for s_, i_ in ((s1, i1), (s2, i2)):
        assert torch.equal(i_, i0.cpu()) and torch.equal(s_.view(torch.int32), s0.cpu().view(torch.int32))
    with pytest.raises(ValueError):
        retrieval.GalleryShard(Gd).search(Qd, 10, query_labels=ql)
    e_s, e_i = retrieval.GalleryShard(Gd[:0], labels=rl[:0]).search(Qd, 10, query_labels=ql)
    assert (e_i == -1).all() and torch.isneginf(e_s).all()
    # two shards on disk with their labels
    path = str(tmp_path / "gal")
    retrieval.save_gallery(path, G[:1001], world=2, labels=rl[:1001])
    assert json.load(open(path + ".manifest.json"))["labels"] is True
    for r in range(2):
        lo, hi = retrieval.shard_bounds(1001, 2, r)
        sh = retrieval.load_gallery_shard(path, r, DEV)
        assert sh.offset == lo and torch.equal(sh.labels.cpu(), rl[lo:hi])
        s_r, i_r = sh.search(Qd, 10, query_labels=ql.to(DEV), mode="ne")
        _assert_bitwise(s_r, i_r, *_oracle(Q, G[lo:hi], 10, rl[lo:hi], ql, "ne"), lo)
    retrieval.save_gallery(path + "2", G[:100], world=2)
    assert retrieval.load_gallery_shard(path + "2", 1, DEV).labels is None

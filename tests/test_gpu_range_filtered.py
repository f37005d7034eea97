"""Filtered threshold search on the GPU: ops.similarity_range_filtered / cor_similarity_range_filtered, GalleryShard.range_search and
GallerySet.range_search with query_labels, distributed_search(min_score=...).

Everything is held BITWISE (score bits, indices, counts) to the restatement tests/range_filtered_refs.py: the chain score matrix of the
operands the GPU multiplies, the allow mask, `>= floor`, a stable sort. Every case uses a g_offset past 2^32 and unit rows with
G[5] = G[3] plus one far-apart duplicate pair, and mixes the floors per query within one call: -inf (the count must be the number of
allowed rows), +inf, NaN, 0.0, the chain score of the query's rank-r row AMONG ITS ALLOWED ROWS for r in {1, k, k + 1, 5k} (rows exactly
on the floor count, ties included) and the floats next above and next below that score. Label layouts as in test_gpu_topk_filtered.py
(uniform over 16 classes, the class-sorted `blocks16`, `skew`), every 7th query unrestricted."""
import functools
import socket

import numpy as np
import pytest
import torch

from tests import range_filtered_refs as RF
from tests import range_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
F = np.float32
OFF = 2 ** 32 + 12345
LAYOUTS = ("uniform16", "blocks16", "skew")


def _ops():
    from cor_amd import ops, _native as nat
    return ops, nat


def _unit(rng, n, C):
    return torch.nn.functional.normalize(torch.from_numpy(rng.standard_normal((n, C), dtype=np.float32)), dim=-1)


@functools.lru_cache(maxsize=None)
def _case(Bq, Ng, C, gdt):
    """(Q, G, S) of one shape and gallery dtype, computed once and left unchanged: unit queries and rows with the planted duplicates and
    the chain score matrix S."""
    rng = np.random.default_rng(1000 * Bq + Ng + C)
    Q = _unit(rng, Bq, C)
    G = _unit(rng, Ng, C).to(gdt)
    if Ng > 5:
        G[5] = G[3]
    if Ng > 40:
        G[Ng - 1] = G[Ng // 3]
    return Q, G, R.chain_scores(Q, G)


@functools.lru_cache(maxsize=None)
def _labels(layout, Ng, Bq):
    """(row labels int32[Ng], query labels int32[Bq]) of test_gpu_topk_filtered.py's layouts; every 7th query is unrestricted."""
    rng = np.random.default_rng(Ng + 7 * Bq + len(layout))
    if layout == "uniform16":
        rl, ql = rng.integers(0, 16, Ng), rng.integers(0, 16, Bq)
    elif layout == "blocks16":                                         # a class-sorted gallery: 16 contiguous blocks
        rl, ql = (np.arange(Ng) * 16) // Ng, rng.integers(0, 16, Bq)
    else:                                                              # "skew": class 0 holds 90 % of the rows
        rl, ql = np.where(rng.random(Ng) < 0.9, 0, rng.integers(1, 9, Ng)), rng.integers(0, 9, Bq)
    ql = ql.copy(); ql[::7] = -1
    return torch.from_numpy(rl.astype(np.int32)), torch.from_numpy(ql.astype(np.int32))


def _mixed_floors(D, k, rot):
    """One floor per query, pattern (b + rot) % 16: the four special floors, then exact / next above / next below the rank-r score of
    D's row (the query's allowed scores, descending; fewer than r allowed rows: -inf and its neighbours)."""
    Bq, Ng = D.shape
    ranks = (1, k, k + 1, 5 * k)
    thr = np.empty((Bq,), dtype=F)
    for b in range(Bq):
        p = (b + rot) % 16
        if p < 4:
            thr[b] = (-np.inf, np.inf, np.nan, 0.0)[p]
        else:
            v = D[b, min(ranks[(p - 4) // 3], Ng) - 1]
            thr[b] = (v, np.nextafter(v, F(np.inf)), np.nextafter(v, F(-np.inf)))[(p - 4) % 3]
    return thr


def _assert_same(got, want, what=""):
    s, i, c = (t.cpu().numpy() for t in got)
    ws, wi, wc = want
    assert c.dtype == np.int32 and i.dtype == np.int64 and s.dtype == F
    bad_c = np.nonzero(c != wc)[0]
    assert bad_c.size == 0, f"{what}: {bad_c.size} counts differ, first query {bad_c[:1]}: {c[bad_c[:1]]} vs {wc[bad_c[:1]]}"
    assert int((i != wi).sum()) == 0, f"{what}: {int((i != wi).sum())} of {wi.size} indices differ from the restatement"
    assert int((s.view(np.int32) != ws.view(np.int32)).sum()) == 0, f"{what}: score bits differ from the restatement"


def _run(Q, G, thr, k, rl, ql, mode, flags=0):
    ops, _ = _ops()
    thr = torch.from_numpy(thr).to(DEV) if isinstance(thr, np.ndarray) else thr
    return ops.similarity_range_filtered(Q.to(DEV), G.to(DEV), thr, k, rl.to(DEV), ql.to(DEV), mode=mode, g_offset=OFF, flags=flags)


# (Bq, Ng, C) -> ks: the boundary set of test_gpu_range.py (one row; the 64-row tile and its neighbours; the tiny-shard / sample boundary;
# the scan form with a sample stride > 1; more than 256 queries = two query groups of the filtered range scan; three; small C; the tile
# form for 16-bit rows; the tile form with a sample stride > 1)
SHAPES = {
    (1, 1, 256): (1, 10, 256), (3, 63, 256): (1, 33, 256), (5, 64, 256): (10, 33, 256), (7, 65, 256): (1, 10, 33),
    (33, 4096, 256): (1, 10, 256), (33, 4097, 256): (10, 33, 256), (64, 20000, 256): (1, 10, 33, 256), (257, 5000, 256): (10, 33, 256),
    (513, 3000, 256): (1, 33, 256), (16, 1000, 16): (1, 10, 33), (12, 3000, 240): (10, 33, 256), (8, 40000, 64): (1, 10, 33, 256),
}
MAIN = []
for _n, ((_Bq, _Ng, _C), _ks) in enumerate(SHAPES.items()):
    for _j, _k in enumerate(_ks):
        for _d, _g in enumerate((F32, BF16, F16)):
            for _m, _mode in enumerate(("eq", "ne")):
                MAIN.append((_Bq, _Ng, _C, _k, _g, _mode, LAYOUTS[(_n + _j + _d + _m) % 3]))


@pytest.mark.parametrize("Bq,Ng,C,k,gdt,mode,layout", MAIN, ids=[f"{b}x{n}x{c}-k{k}-{str(g)[6:]}-{m}-{l}" for b, n, c, k, g, m, l in MAIN])
def test_filtered_range_bitwise_vs_restatement(Bq, Ng, C, k, gdt, mode, layout):
    Q, G, S = _case(Bq, Ng, C, gdt)
    rl, ql = _labels(layout, Ng, Bq)
    allow = RF.allow_mask(rl, ql, mode)
    thr = _mixed_floors(RF.allowed_sorted(S, allow), k, rot=k + Ng)
    got = _run(Q, G, thr, k, rl, ql, mode)
    _assert_same(got, RF.range_from_scores(S, allow, thr, k, OFF), "mixed floors")
    whole = np.isneginf(thr)
    assert (got[2].cpu().numpy()[whole] == allow.sum(1)[whole]).all()


@pytest.mark.parametrize("gdt,C", [(BF16, 256), (F32, 256), (F16, 64)], ids=["bf16-256", "f32-256", "f16-64"])
@pytest.mark.parametrize("k", [10, 100])
def test_filtered_range_edge_cases(gdt, C, k):
    """An absent class (count 0, only the tail), a class with fewer than k rows (all of them above a low floor, then the tail), a class
    of ONE row lying exactly on the floor (count 1; one ulp higher: 0), unrestricted and labelled queries mixed in one call."""
    Q, G, S = _case(24, 20000, C, gdt)
    rng = np.random.default_rng(2)
    rl = torch.from_numpy(rng.integers(0, 4, 20000).astype(np.int32))
    rl[[11, 500, 9000, 15000, 19999]] = 5
    rl[777] = 6
    ql = torch.from_numpy(rng.integers(0, 4, 24).astype(np.int32))
    ql[0], ql[1], ql[2], ql[3], ql[4] = 9, 5, 6, -1, 6
    allow = RF.allow_mask(rl, ql, "eq")
    thr = _mixed_floors(RF.allowed_sorted(S, allow), k, rot=1)
    thr[0], thr[1], thr[2], thr[4] = -np.inf, -1.0, S[2, 777], np.nextafter(S[4, 777], F(np.inf))
    got = _run(Q, G, thr, k, rl, ql, "eq")
    _assert_same(got, RF.range_from_scores(S, allow, thr, k, OFF), "edge cases")
    s, i, c = (t.cpu() for t in got)
    assert c[0] == 0 and (i[0] == -1).all() and torch.isneginf(s[0]).all()
    assert c[1] == 5 and sorted((i[1, :5] - OFF).tolist()) == [11, 500, 9000, 15000, 19999] and (i[1, 5:] == -1).all()
    assert c[2] == 1 and i[2, 0] == OFF + 777 and (i[2, 1:] == -1).all()
    assert c[4] == 0 and (i[4] == -1).all()


EQUIV = [(64, 20000, 256, 33, F32), (64, 20000, 256, 100, BF16), (64, 20000, 256, 256, F16), (12, 3000, 240, 33, BF16),
         (8, 40000, 64, 64, F16), (16, 1000, 16, 256, BF16), (64, 20000, 256, 10, BF16), (513, 3000, 256, 1, BF16), (7, 65, 256, 10, F32)]


@pytest.mark.parametrize("Bq,Ng,C,k,gdt", EQUIV, ids=[f"{b}x{n}x{c}-k{k}-{str(g)[6:]}" for b, n, c, k, g in EQUIV])
def test_unrestricted_queries_equal_similarity_range(Bq, Ng, C, k, gdt):
    """All query labels negative: the unfiltered range search, bit for bit, counts included, whatever the mode and the row labels."""
    ops, _ = _ops()
    Q, G, S = _case(Bq, Ng, C, gdt)
    rl, _ = _labels("uniform16", Ng, Bq)
    ql = torch.full((Bq,), -1, dtype=torch.int32)
    thr = _mixed_floors(-np.sort(-S, axis=1), k, rot=3)
    want = ops.similarity_range(Q.to(DEV), G.to(DEV), torch.from_numpy(thr).to(DEV), k, g_offset=OFF)
    for mode in ("eq", "ne"):
        got = _run(Q, G, thr, k, rl, ql, mode)
        assert torch.equal(got[1], want[1]) and torch.equal(got[2], want[2]) and torch.equal(got[0].view(torch.int32), want[0].view(torch.int32))
    _assert_same(want, R.range_from_scores(S, thr, k, OFF), "the unfiltered call")


@pytest.mark.parametrize("mode", ["eq", "ne"])
@pytest.mark.parametrize("Bq,Ng,C,k,gdt", EQUIV, ids=[f"{b}x{n}x{c}-k{k}-{str(g)[6:]}" for b, n, c, k, g in EQUIV])
def test_floor_minus_inf_equals_filtered_topk(Bq, Ng, C, k, gdt, mode):
    """With the floor at -inf the lists are ops.similarity_topk_filtered's, bit for bit (that call is bitwise the chain on the allowed
    rows for every dtype, C and k), and the count is the number of allowed rows. A scalar floor equals the tensor of that floor."""
    ops, _ = _ops()
    Q, G, S = _case(Bq, Ng, C, gdt)
    rl, ql = _labels(LAYOUTS[(Bq + k) % 3], Ng, Bq)
    allow = RF.allow_mask(rl, ql, mode)
    s, i, c = _run(Q, G, float("-inf"), k, rl, ql, mode)
    ts, ti = ops.similarity_topk_filtered(Q.to(DEV), G.to(DEV), k, rl.to(DEV), ql.to(DEV), mode=mode, g_offset=OFF)
    assert torch.equal(i, ti) and torch.equal(s.view(torch.int32), ts.view(torch.int32))
    assert (c.cpu().numpy() == allow.sum(1)).all()
    floor = float(RF.allowed_sorted(S, allow)[1 % Bq, min(3 * k, Ng) - 1])
    a = _run(Q, G, floor, k, rl, ql, mode)
    b = _run(Q, G, torch.full((Bq,), floor, dtype=F32, device=DEV), k, rl, ql, mode)
    assert torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[2], b[2])
    _assert_same(a, RF.range_from_scores(S, allow, F(floor), k, OFF), "scalar floor")


@pytest.mark.parametrize("gdt", [F32, BF16, F16])
@pytest.mark.parametrize("mode", ["eq", "ne"])
def test_planted_excluded_copies_never_count(gdt, mode):
    """Every query has 8 exact copies of itself in the gallery that its filter excludes (ne: they carry the query's own label, every
    other row its own; eq: they sit in another class), and the floor lies just below 1 (0.99; no allowed row of these random unit
    vectors comes near it). An unmasked scan would count 8 and list the copies: the count is 0 and no copy appears; with the floor at
    -inf the lists rank allowed rows only."""
    Bq, Ng, k = 64, 40000, 5
    rng = np.random.default_rng(11)
    Q = _unit(rng, Bq, 256)
    G = _unit(rng, Ng, 256).to(gdt)
    pos = torch.from_numpy(rng.choice(Ng, Bq * 8, replace=False)).view(Bq, 8)
    for b in range(Bq):
        G[pos[b]] = Q[b].to(gdt)
    if mode == "ne":
        rl = torch.arange(Ng, dtype=torch.int32) + 1000                 # every other row its own image
        ql = torch.arange(Bq, dtype=torch.int32) + 100000
        for b in range(Bq):
            rl[pos[b]] = int(ql[b])
    else:
        rl = torch.from_numpy(rng.integers(0, 8, Ng).astype(np.int32))
        ql = torch.arange(Bq, dtype=torch.int32) % 8
        for b in range(Bq):
            rl[pos[b]] = (int(ql[b]) + 1) % 8
    S = R.chain_scores(Q, G)
    allow = RF.allow_mask(rl, ql, mode)
    assert float(S[np.arange(Bq)[:, None], pos.numpy()].min()) > 0.99 and float(np.where(allow, S, -1).max()) < 0.5
    _, nat = _ops()
    for thr in (F(0.99), F(-np.inf)):
        got = _run(Q, G, float(thr), k, rl, ql, mode, flags=nat.TOPK_NO_FALLBACK)
        _assert_same(got, RF.range_from_scores(S, allow, thr, k, OFF), f"floor {thr}")
        ic = got[1].cpu() - OFF
        assert not any(bool(torch.isin(ic[b], pos[b]).any()) for b in range(Bq))      # no query finds its own excluded copies
    c = _run(Q, G, 0.99, k, rl, ql, mode)[2]
    assert not bool(c.any())


@pytest.mark.parametrize("layout", ["uniform16", "blocks16"])
@pytest.mark.parametrize("k", [10, 100])
@pytest.mark.parametrize("gdt", [F32, BF16, F16])
def test_rank_floors_and_floor_zero_stay_on_the_fast_path(gdt, k, layout):
    """(64, 20 000, 256), eq over uniform and class-sorted labels, floors at each query's rank-r allowed score and at 0.0: no query may
    need the fallback (COR_TOPK_NO_FALLBACK shows no -2 in any list or count). A condition, not a measurement. The two calls this one
    combines mark no query at these inputs either: similarity_topk_filtered and similarity_range with the same flag, whose kernels this
    change leaves instruction for instruction as they were, are asserted clean here first."""
    ops, nat = _ops()
    Q, G, S = _case(64, 20000, 256, gdt)
    rl, ql = _labels(layout, 20000, 64)
    allow = RF.allow_mask(rl, ql, "eq")
    D = RF.allowed_sorted(S, allow)
    Qd, Gd = Q.to(DEV), G.to(DEV)
    for thr in (_mixed_floors(D, k, rot=4), np.zeros(64, dtype=F)):
        td = torch.from_numpy(thr).to(DEV)
        _, ti = ops.similarity_topk_filtered(Qd, Gd, k, rl.to(DEV), ql.to(DEV), mode="eq", g_offset=OFF, flags=nat.TOPK_NO_FALLBACK)
        _, ri, rc = ops.similarity_range(Qd, Gd, td, k, g_offset=OFF, flags=nat.TOPK_NO_FALLBACK)
        assert not bool((ti == -2).any()) and not bool((ri == -2).any()) and not bool((rc == -2).any())
        got = _run(Q, G, thr, k, rl, ql, "eq", flags=nat.TOPK_NO_FALLBACK)
        assert not bool((got[1] == -2).any()) and not bool((got[2] == -2).any())
        _assert_same(got, RF.range_from_scores(S, allow, thr, k, OFF), "no fallback")


# (gdt, C): the record (scan-form) selection kernel, then the entry-list (tile-form) one for fp32 and for C != 256
@pytest.mark.parametrize("gdt,C", [(BF16, 256), (F32, 256), (F16, 128)], ids=["bf16-256", "f32-256", "f16-128"])
def test_overflow_falls_back_over_the_allowed_rows(gdt, C):
    """6 000 identical rows close to query 0, alternating classes 0 / 1 (the filtered top-k's fixture); query 0 keeps class 0: 3 000 tied
    allowed rows overflow the short list at k = 100. With the floor (a) equal to the identical rows' score (3 000 allowed rows exactly on
    the floor) and (b) far below everything, the fallback counts and ranks the ALLOWED copies only (the first 100 class-0 copies in index
    order); with COR_TOPK_NO_FALLBACK exactly the overflowed queries carry -2 in every slot and in the count."""
    _, nat = _ops()
    nq, Ng, k = 16, 20000, 100
    rng = np.random.default_rng(5 + C)
    Q = _unit(rng, nq, C)
    row = _unit(rng, 1, C)
    G = _unit(rng, Ng, C)
    G[10000:16000] = torch.nn.functional.normalize(Q[0:1] + 0.05 * row, dim=-1)
    G[5] = G[3]; G[Ng - 1] = G[Ng // 3]
    G = G.to(gdt)
    rl = torch.from_numpy(rng.integers(0, 4, Ng).astype(np.int32))
    rl[10000:16000] = torch.arange(6000, dtype=torch.int32) % 2
    ql = torch.from_numpy(rng.integers(0, 4, nq).astype(np.int32)); ql[0] = 0; ql[1::5] = -1
    S = R.chain_scores(Q, G)
    allow = RF.allow_mask(rl, ql, "eq")
    for thr in (S[:, 10000].copy(), np.full((nq,), -2.0, dtype=F)):
        want = RF.range_from_scores(S, allow, thr, k, OFF)
        assert 3000 <= int(want[2][0]) <= int(allow[0].sum())
        got = _run(Q, G, thr, k, rl, ql, "eq")
        _assert_same(got, want, "with the fallback")
        assert got[1][0].cpu().tolist() == list(range(OFF + 10000, OFF + 10000 + 2 * k, 2))
        rs, ri, rc = _run(Q, G, thr, k, rl, ql, "eq", flags=nat.TOPK_NO_FALLBACK)
        flagged = (ri == -2).all(dim=1)
        assert bool(flagged[0]) and int(flagged.sum()) < nq
        assert torch.equal((ri == -2).any(dim=1), flagged) and torch.equal(rc == -2, flagged)
        keep = ~flagged
        assert torch.equal(ri[keep], got[1][keep]) and torch.equal(rc[keep], got[2][keep])
        assert torch.equal(rs[keep].view(torch.int32), got[0][keep].view(torch.int32))


def test_label_validation_on_the_device():
    ops, nat = _ops()
    Q, G, S = _case(7, 65, 256, F32)
    Qd, Gd = Q.to(DEV), G.to(DEV)
    rl, ql = torch.zeros(65, dtype=torch.int32, device=DEV), torch.zeros(7, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="row_labels"):
        ops.similarity_range_filtered(Qd, Gd, 0.0, 3, rl[:64], ql)
    with pytest.raises(ValueError, match="query_labels"):
        ops.similarity_range_filtered(Qd, Gd, 0.0, 3, rl, ql[:6])
    with pytest.raises(ValueError, match="int32"):
        ops.similarity_range_filtered(Qd, Gd, 0.0, 3, rl.float(), ql)
    with pytest.raises(nat.NativeError):
        ops.similarity_range_filtered(Qd, Gd, 0.0, 3, rl, ql, flags=nat.TOPK_FORCE_LISTS)
    s, i, c = ops.similarity_range_filtered(Qd, Gd, 0.0, 3, rl.long(), ql.long(), mode="ne")     # int64 labels are converted; nobody is allowed
    assert (i == -1).all() and not bool(c.any())
    # a label view at an odd offset (not 16-byte aligned) is copied, not refused
    big = torch.zeros(66, dtype=torch.int32, device=DEV)
    s, i, c = ops.similarity_range_filtered(Qd, Gd, float("-inf"), 3, big[1:], ql)
    assert (c == 65).all()


def test_shard_and_set_range_search_with_labels():
    """GalleryShard.range_search with query_labels is the filtered call with the shard's labels and offset; three bf16 segments (and an
    empty one) equal one shard over the concatenated rows bitwise, lists and counts; mixed fp32 + fp16 segments equal the restatement per
    segment, merged; None keeps the unfiltered result."""
    from cor_amd import retrieval
    Q, G, S = _case(257, 5000, 256, BF16)
    rl, ql = _labels("uniform16", 5000, 257)
    Qd, Gd = Q.to(DEV), G.to(DEV)
    for mode in ("eq", "ne"):
        allow = RF.allow_mask(rl, ql, mode)
        thr = _mixed_floors(RF.allowed_sorted(S, allow), 33, rot=1)
        td = torch.from_numpy(thr).to(DEV)
        cuts = (0, 1500, 3100, 5000, 5000)                                         # the last segment is empty
        gs = retrieval.GallerySet([retrieval.GalleryShard(Gd[a:b], offset=OFF + a, labels=rl[a:b]) for a, b in zip(cuts, cuts[1:])])
        one = retrieval.GalleryShard(Gd, offset=OFF, labels=rl).range_search(Qd, td, 33, query_labels=ql, mode=mode)
        got = gs.range_search(Qd, td, 33, query_labels=ql.to(DEV), mode=mode)
        assert all(torch.equal(a, b) for a, b in zip(got[1:], one[1:])) and torch.equal(got[0].view(torch.int32), one[0].view(torch.int32))
        _assert_same(got, RF.range_from_scores(S, allow, thr, 33, OFF), f"three bf16 segments, {mode}")
        # mixed dtypes: a row's score depends on its segment's dtype
        G32 = G.float()
        parts = [(G32[:2000], 0), (G32[2000:].to(F16), 2000)]
        mixed = retrieval.GallerySet([retrieval.GalleryShard(g.to(DEV), offset=OFF + o, labels=rl[o:o + g.shape[0]]) for g, o in parts])
        want = R.merge_lists([RF.similarity_range_filtered(Q, g, 0.1, 20, rl[o:o + g.shape[0]], ql, mode, OFF + o) for g, o in parts], 20)
        _assert_same(mixed.range_search(Q, 0.1, 20, query_labels=ql, mode=mode), want, f"fp32 + fp16 segments, {mode}")
    plain = retrieval.GalleryShard(Gd, offset=OFF, labels=rl).range_search(Qd, 0.1, 20)
    _assert_same(plain, R.range_from_scores(S, F(0.1), 20, OFF), "no query labels: the unfiltered call")
    with pytest.raises(ValueError, match="no row labels"):
        retrieval.GalleryShard(Gd, offset=OFF).range_search(Qd, 0.1, 20, query_labels=ql)
    s, i, c = retrieval.GalleryShard(Gd[:0], offset=7, labels=rl[:0]).range_search(Qd, 0.0, 5, query_labels=ql)
    assert s.shape == (257, 5) and torch.isneginf(s).all() and (i == -1).all() and c.dtype == torch.int32 and not bool(c.any())
    i8 = retrieval.QuantizedShard.from_rows(Gd[:64], offset=10 ** 12, labels=rl[:64])
    assert not hasattr(i8, "range_search")
    with pytest.raises(ValueError, match="int8"):
        retrieval.GallerySet([retrieval.GalleryShard(Gd[:100], offset=0, labels=rl[:100]), i8]).range_search(Qd, 0.1, 4, query_labels=ql)


@pytest.mark.parametrize("Bq,Ng,C,gdt", [(64, 20000, 256, BF16), (8, 40000, 64, F32)], ids=["scan-form", "tile-form"])
def test_side_stream_and_graph_replay(Bq, Ng, C, gdt):
    """The call runs on the current stream, allocates nothing inside the library and never synchronises: a side stream, and a captured
    graph (one linear capture stream) replayed three times with new queries, floors and labels."""
    ops, _ = _ops()
    Q, G, S = _case(Bq, Ng, C, gdt)
    rl, ql_a = _labels("uniform16", Ng, Bq)
    k = 33
    perm = np.arange(Bq)[::-1].copy()
    Qb, Sb = Q[torch.from_numpy(perm)], S[perm]
    ql_b = torch.roll(ql_a, 3)
    allow_a, allow_b = RF.allow_mask(rl, ql_a, "ne"), RF.allow_mask(rl, ql_b, "ne")
    thr_a, thr_b = _mixed_floors(RF.allowed_sorted(S, allow_a), k, rot=0), _mixed_floors(RF.allowed_sorted(Sb, allow_b), k, rot=7)
    want_a, want_b = RF.range_from_scores(S, allow_a, thr_a, k, OFF), RF.range_from_scores(Sb, allow_b, thr_b, k, OFF)
    Gd, rld, qin, tin, lin = G.to(DEV), rl.to(DEV), Q.to(DEV), torch.from_numpy(thr_a).to(DEV), ql_a.to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = ops.similarity_range_filtered(qin, Gd, tin, k, rld, lin, mode="ne", g_offset=OFF)   # (also sets the kernels' one-time attributes)
    side.synchronize()
    _assert_same(got, want_a, "side stream")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.similarity_range_filtered(qin, Gd, tin, k, rld, lin, mode="ne", g_offset=OFF)
    for n, (q_, t_, l_, want) in enumerate(((Q, thr_a, ql_a, want_a), (Qb, thr_b, ql_b, want_b), (Q, thr_a, ql_a, want_a))):
        qin.copy_(q_.to(DEV)); tin.copy_(torch.from_numpy(t_).to(DEV)); lin.copy_(l_.to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        _assert_same(out, want, f"graph replay {n}")


def test_distributed_range_search_on_a_one_rank_rccl_group():
    """distributed_search(min_score=..., always_collective=True) on a one-rank nccl group moves floors, labels, lists and counts through
    both collectives: merge="host" and merge="device", gather, all-gather and deferred forms, a GallerySet as the shard, plain and with
    labels, all equal the set-level range_search bitwise, and the counts arrive as int64."""
    import torch.distributed as dist
    from cor_amd import retrieval
    assert not dist.is_initialized()
    Q, G, S = _case(33, 4097, 256, F16)
    rl, ql = _labels("uniform16", 4097, 33)
    Q, ql, S = Q[:5], ql[:5].clone(), S[:5]
    ql[1] = -1
    Qd, Gd = Q.to(DEV), G.to(DEV)
    gs = retrieval.GallerySet([retrieval.GalleryShard(Gd[:3000], offset=OFF, labels=rl[:3000]),
                               retrieval.GalleryShard(Gd[3000:].float(), offset=OFF + 3000, labels=rl[3000:])])
    k = 20
    thr = torch.tensor([-np.inf, 0.05, np.nan, float(S[3].max()), 0.0], dtype=F32, device=DEV)
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=torch.device(DEV))
    try:
        for kw in (dict(), dict(query_labels=ql.to(DEV), filter_mode="eq"), dict(query_labels=ql.to(DEV), filter_mode="ne")):
            s0, i0, c0 = gs.range_search(Qd, thr, k, query_labels=kw.get("query_labels"), mode=kw.get("filter_mode", "eq"))
            n_allowed = 4097 if not kw else int(RF.allow_mask(rl, ql, kw["filter_mode"])[0].sum())
            assert int(c0[0]) == n_allowed and int(c0[2]) == 0                         # a floor of -inf; a NaN floor
            common = dict(max_local=8, always_collective=True, min_score=thr, **kw)
            results = [retrieval.distributed_search(Qd, gs, k, merge=m, **common) for m in ("host", "device")]
            results.append(retrieval.distributed_search(Qd, gs, k, dst=None, **common))
            results.append(retrieval.distributed_search(Qd, gs, k, defer=True, merge="device", **common).result())
            results.append(retrieval.distributed_search(Qd, gs, k, defer=True, **common).result())
            for s_, i_, c_ in results:
                assert c_.dtype == torch.int64 and torch.equal(c_, c0.cpu().to(torch.int64))
                assert torch.equal(i_, i0.cpu()) and torch.equal(s_.view(torch.int32), s0.cpu().view(torch.int32))
        s0, i0, c0 = gs.range_search(Qd, 0.05, k)
        s1, i1, c1 = retrieval.distributed_search(Qd, gs, k, max_local=8, always_collective=True, min_score=0.05)   # a scalar floor
        assert torch.equal(c1, c0.cpu().to(torch.int64)) and torch.equal(i1, i0.cpu()) and torch.equal(s1.view(torch.int32), s0.cpu().view(torch.int32))
        two = retrieval.distributed_search(Qd, gs, k, max_local=8, always_collective=True)                          # without it: two tensors
        assert len(two) == 2
        with pytest.raises(ValueError, match="min_score"):
            retrieval.distributed_search(Qd, retrieval.GalleryShard(Gd, groups=rl), k, max_local=8, always_collective=True, min_score=0.5, distinct=True)
        with pytest.raises(ValueError, match="int8"):
            retrieval.distributed_search(Qd, retrieval.QuantizedShard.from_rows(Gd[:64]), k, max_local=8, always_collective=True, min_score=0.5)
    finally:
        dist.destroy_process_group()
    # no process group: the shortcut returns the same three tensors, deferred or not
    s0, i0, c0 = gs.range_search(Qd, thr, k, query_labels=ql.to(DEV), mode="ne")
    for res in (retrieval.distributed_search(Qd, gs, k, min_score=thr, query_labels=ql.to(DEV), filter_mode="ne"),
                retrieval.distributed_search(Qd, gs, k, min_score=thr, query_labels=ql.to(DEV), filter_mode="ne", defer=True).result()):
        assert res[2].dtype == torch.int64 and torch.equal(res[2], c0.cpu().to(torch.int64))
        assert torch.equal(res[1], i0.cpu()) and torch.equal(res[0].view(torch.int32), s0.cpu().view(torch.int32))

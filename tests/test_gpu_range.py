"""Threshold (range) search on the GPU: ops.similarity_range / cor_similarity_range, GalleryShard.range_search, GallerySet.range_search.

Everything is held BITWISE (score bits, indices, counts) to the restatement tests/range_refs.py: the chain score matrix of the
operands the GPU multiplies, `>= floor`, a stable sort. Every case uses a g_offset past 2^32 and unit rows with G[5] = G[3] plus one
far-apart duplicate pair, and mixes the floors per query within one call: -inf (the count must be Ng), +inf, NaN, 0.0, the chain score
of the query's rank-r row for r in {1, k, k + 1, 5k} (rows exactly on the floor count, ties included) and the floats next above and
next below that score, the smallest inputs that expose a wrong band."""
import functools

import numpy as np
import pytest
import torch

from tests import range_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
F = np.float32
OFF = 2 ** 32 + 12345


def _ops():
    from cor_amd import ops, _native as nat
    return ops, nat


def _unit(rng, n, C):
    return torch.nn.functional.normalize(torch.from_numpy(rng.standard_normal((n, C), dtype=np.float32)), dim=-1)


@functools.lru_cache(maxsize=None)
def _case(Bq, Ng, C, gdt):
    """(Q, G, S, D) of one shape and gallery dtype, computed once and left unchanged: unit queries and rows with the planted duplicates,
    the chain score matrix S and its rows sorted descending D."""
    rng = np.random.default_rng(1000 * Bq + Ng + C)
    Q = _unit(rng, Bq, C)
    G = _unit(rng, Ng, C).to(gdt)
    if Ng > 5:
        G[5] = G[3]
    if Ng > 40:
        G[Ng - 1] = G[Ng // 3]
    S = R.chain_scores(Q, G)
    return Q, G, S, -np.sort(-S, axis=1)


def _mixed_floors(D, k, rot):
    """One floor per query, pattern (b + rot) % 16: the four special floors, then exact / next above / next below the rank-r score."""
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


# (Bq, Ng, C): one row; the 64-row tile and its neighbours; the tiny-shard / sample boundary; the scan form with a sample stride > 1; two
# query blocks per wave; two query groups; small C; the tile form for 16-bit rows; the tile form with a sample stride > 1
SHAPES = {
    (1, 1, 256): (1, 10, 256), (3, 63, 256): (1, 33, 256), (5, 64, 256): (10, 33, 256), (7, 65, 256): (1, 10, 33),
    (33, 4096, 256): (1, 10, 256), (33, 4097, 256): (10, 33, 256), (64, 20000, 256): (1, 10, 33, 256), (257, 5000, 256): (10, 33, 256),
    (513, 3000, 256): (1, 33, 256), (16, 1000, 16): (1, 10, 33), (12, 3000, 240): (10, 33, 256), (8, 40000, 64): (1, 10, 33, 256),
}
MAIN = [(Bq, Ng, C, k, g) for (Bq, Ng, C), ks in SHAPES.items() for k in ks for g in (F32, BF16, F16)]


@pytest.mark.parametrize("Bq,Ng,C,k,gdt", MAIN, ids=[f"{b}x{n}x{c}-k{k}-{str(g)[6:]}" for b, n, c, k, g in MAIN])
def test_range_bitwise_vs_restatement(Bq, Ng, C, k, gdt):
    ops, _ = _ops()
    Q, G, S, D = _case(Bq, Ng, C, gdt)
    thr = _mixed_floors(D, k, rot=k + Ng)
    got = ops.similarity_range(Q.to(DEV), G.to(DEV), torch.from_numpy(thr).to(DEV), k, g_offset=OFF)
    want = R.range_from_scores(S, thr, k, OFF)
    _assert_same(got, want, "mixed floors")
    whole = np.isneginf(thr)
    assert (got[2].cpu().numpy()[whole] == Ng).all()


EQUIV = [(64, 20000, 256, 33, F32), (64, 20000, 256, 100, BF16), (64, 20000, 256, 256, F16), (12, 3000, 240, 33, BF16),
         (8, 40000, 64, 64, F16), (16, 1000, 16, 256, BF16), (64, 20000, 256, 10, BF16), (64, 20000, 256, 32, F16),
         (8, 40000, 64, 10, F32), (513, 3000, 256, 1, BF16), (7, 65, 256, 10, F32)]


@pytest.mark.parametrize("Bq,Ng,C,k,gdt", EQUIV, ids=[f"{b}x{n}x{c}-k{k}-{str(g)[6:]}" for b, n, c, k, g in EQUIV])
def test_floor_minus_inf_equals_topk_and_scalar_equals_tensor(Bq, Ng, C, k, gdt):
    """With the floor at -inf the lists are ops.similarity_topk's, bit for bit, wherever that call is itself bitwise the chain (every
    dtype and C at k >= 33; fp32, and 16-bit rows at C = 256, at k <= 32), and the count is Ng. A scalar floor and the tensor of that
    floor give the same result."""
    ops, _ = _ops()
    Q, G, S, D = _case(Bq, Ng, C, gdt)
    Qd, Gd = Q.to(DEV), G.to(DEV)
    s, i, c = ops.similarity_range(Qd, Gd, float("-inf"), k, g_offset=OFF)
    ts, ti = ops.similarity_topk(Qd, Gd, k, g_offset=OFF)
    assert torch.equal(i, ti) and torch.equal(s.view(torch.int32), ts.view(torch.int32))
    assert (c == Ng).all()
    floor = float(D[0, min(3 * k, Ng) - 1])
    a = ops.similarity_range(Qd, Gd, floor, k, g_offset=OFF)
    b = ops.similarity_range(Qd, Gd, torch.full((Bq,), floor, dtype=F32, device=DEV), k, g_offset=OFF)
    assert torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[2], b[2])
    _assert_same(a, R.range_from_scores(S, F(floor), k, OFF), "scalar floor")


@pytest.mark.parametrize("k", [10, 100])
@pytest.mark.parametrize("gdt", [F32, BF16, F16])
def test_rank_floors_stay_on_the_fast_path(gdt, k):
    """(64, 20 000, 256) with floors at each query's rank-r score: no query may need the fallback (COR_TOPK_NO_FALLBACK shows no -2)."""
    ops, nat = _ops()
    Q, G, S, D = _case(64, 20000, 256, gdt)
    thr = _mixed_floors(D, k, rot=4)
    got = ops.similarity_range(Q.to(DEV), G.to(DEV), torch.from_numpy(thr).to(DEV), k, g_offset=OFF, flags=nat.TOPK_NO_FALLBACK)
    assert not bool((got[1] == -2).any()) and not bool((got[2] == -2).any())
    _assert_same(got, R.range_from_scores(S, thr, k, OFF), "no fallback")


def test_floor_zero_counts_half_the_shard_on_the_fast_path():
    """(64, 20 000, 256) bf16 with the floor at 0.0: the counting path at full load. About half the rows are members (a count is
    Binomial(20 000, 1/2): within 10 000 +- 6 sigma = 425; on this data 9 859 .. 10 125) and the band [-delta, +delta) around the floor
    holds at most 30 rows per query (checked here with delta = 6.5e-5), so the band must fit the plan: no -2 marker with
    COR_TOPK_NO_FALLBACK."""
    ops, nat = _ops()
    Q, G, S, D = _case(64, 20000, 256, BF16)
    assert int((np.abs(S) < 6.5e-5).sum(1).max()) <= 30
    for k in (10, 100):
        got = ops.similarity_range(Q.to(DEV), G.to(DEV), 0.0, k, g_offset=OFF, flags=nat.TOPK_NO_FALLBACK)
        assert not bool((got[1] == -2).any()) and not bool((got[2] == -2).any())
        want = R.range_from_scores(S, F(0.0), k, OFF)
        _assert_same(got, want, "floor 0.0")
        assert 10000 - 425 <= int(want[2].min()) and int(want[2].max()) <= 10000 + 425


# (gdt, C): the record (scan-form) selection kernel, then the entry-list (tile-form) one for fp32 and for C != 256
@pytest.mark.parametrize("gdt,C", [(BF16, 256), (F32, 256), (F16, 128)], ids=["bf16-256", "f32-256", "f16-128"])
def test_overflow_falls_back_on_the_device(gdt, C):
    """3 000 identical rows close to query 0 tie far more rows than the short list holds: the query overflows. With the floor (a) equal
    to the identical rows' score (3 000 rows exactly on the floor, for every query) and (b) far below everything, counts and lists stay
    exact; with COR_TOPK_NO_FALLBACK the overflowed queries, and only they, carry -2 in every slot and in the count."""
    ops, nat = _ops()
    nq, Ng, k = 16, 20000, 100
    rng = np.random.default_rng(5 + C)
    Q = _unit(rng, nq, C)
    row = _unit(rng, 1, C)
    G = _unit(rng, Ng, C)
    G[10000:13000] = torch.nn.functional.normalize(Q[0:1] + 0.05 * row, dim=-1)
    G[5] = G[3]; G[Ng - 1] = G[Ng // 3]
    G = G.to(gdt)
    S = R.chain_scores(Q, G)
    Qd, Gd = Q.to(DEV), G.to(DEV)
    for thr in (S[:, 10000].copy(), np.full((nq,), -2.0, dtype=F)):
        want = R.range_from_scores(S, thr, k, OFF)
        assert int(want[2][0]) >= 3000
        td = torch.from_numpy(thr).to(DEV)
        got = ops.similarity_range(Qd, Gd, td, k, g_offset=OFF)
        _assert_same(got, want, "with the fallback")
        assert got[1][0].cpu().tolist() == list(range(OFF + 10000, OFF + 10000 + k))
        rs, ri, rc = ops.similarity_range(Qd, Gd, td, k, g_offset=OFF, flags=nat.TOPK_NO_FALLBACK)
        flagged = (ri == -2).all(dim=1)
        assert bool(flagged[0]) and int(flagged.sum()) < nq
        assert torch.equal((ri == -2).any(dim=1), flagged) and torch.equal(rc == -2, flagged)
        keep = ~flagged
        assert torch.equal(ri[keep], got[1][keep]) and torch.equal(rc[keep], got[2][keep])
        assert torch.equal(rs[keep].view(torch.int32), got[0][keep].view(torch.int32))


def test_gallery_shard_range_search():
    from cor_amd import retrieval
    Q, G, S, D = _case(33, 4097, 256, F16)
    shard = retrieval.GalleryShard(G.to(DEV), offset=OFF)
    thr = _mixed_floors(D, 10, rot=0)
    _assert_same(shard.range_search(Q.to(DEV), torch.from_numpy(thr), 10), R.range_from_scores(S, thr, 10, OFF), "tensor floors")
    _assert_same(shard.range_search(Q, 0.125, 33), R.range_from_scores(S, F(0.125), 33, OFF), "scalar floor, host queries")
    s, i, c = retrieval.GalleryShard(G[:0].to(DEV), offset=7).range_search(Q.to(DEV), 0.0, 5)
    assert s.shape == (33, 5) and torch.isneginf(s).all() and (i == -1).all() and c.dtype == torch.int32 and not bool(c.any())
    assert s.is_cuda and i.is_cuda and c.is_cuda


def test_gallery_set_range_search():
    """Three bf16 segments equal one shard over the concatenated rows bitwise, lists and counts; mixed fp32 + fp16 segments equal the
    restatement per segment, merged; an empty set and an empty segment are covered."""
    from cor_amd import retrieval
    Q, G, S, D = _case(257, 5000, 256, BF16)
    Qd, Gd = Q.to(DEV), G.to(DEV)
    thr = _mixed_floors(D, 33, rot=1)
    td = torch.from_numpy(thr).to(DEV)
    cuts = (0, 1500, 3100, 5000, 5000)                                             # the last segment is empty
    gs = retrieval.GallerySet([retrieval.GalleryShard(Gd[a:b], offset=OFF + a) for a, b in zip(cuts, cuts[1:])])
    assert len(gs.segments) == 4 and len(gs) == 5000
    one = retrieval.GalleryShard(Gd, offset=OFF).range_search(Qd, td, 33)
    got = gs.range_search(Qd, td, 33)
    assert all(torch.equal(a, b) for a, b in zip(got[1:], one[1:])) and torch.equal(got[0].view(torch.int32), one[0].view(torch.int32))
    _assert_same(got, R.range_from_scores(S, thr, 33, OFF), "three bf16 segments")
    # mixed dtypes: a row's score depends on its segment's dtype
    G32 = G.float()
    parts = [(G32[:2000], 0), (G32[2000:].to(F16), 2000)]
    mixed = retrieval.GallerySet([retrieval.GalleryShard(g.to(DEV), offset=OFF + o) for g, o in parts])
    want = R.merge_lists([R.similarity_range(Q, g, 0.1, 20, OFF + o) for g, o in parts], 20)
    _assert_same(mixed.range_search(Qd, 0.1, 20), want, "fp32 + fp16 segments")
    for empty in (retrieval.GallerySet(), retrieval.GallerySet([retrieval.GalleryShard(Gd[:0], offset=3)])):
        s, i, c = empty.range_search(Qd, 0.1, 4)
        assert s.shape == (257, 4) and torch.isneginf(s).all() and (i == -1).all() and c.dtype == torch.int32 and not bool(c.any())
    i8 = retrieval.QuantizedShard.from_rows(Gd[:64], offset=10 ** 12)
    with pytest.raises(ValueError, match="int8"):
        retrieval.GallerySet([retrieval.GalleryShard(Gd[:100], offset=0), i8]).range_search(Qd, 0.1, 4)


@pytest.mark.parametrize("Bq,Ng,C,gdt", [(64, 20000, 256, BF16), (8, 40000, 64, F32)], ids=["scan-form", "tile-form"])
def test_side_stream_and_graph_replay(Bq, Ng, C, gdt):
    """The call runs on the current stream, allocates nothing inside the library and never synchronises: a side stream, and a captured
    graph (one linear capture stream) replayed three times with new queries and floors."""
    ops, _ = _ops()
    Q, G, S, D = _case(Bq, Ng, C, gdt)
    k = 33
    thr_a = _mixed_floors(D, k, rot=0)
    perm = np.arange(Bq)[::-1].copy()
    Qb, Sb, thr_b = Q[torch.from_numpy(perm)], S[perm], _mixed_floors(D[perm], k, rot=7)
    want_a, want_b = R.range_from_scores(S, thr_a, k, OFF), R.range_from_scores(Sb, thr_b, k, OFF)
    Gd, qin, tin = G.to(DEV), Q.to(DEV), torch.from_numpy(thr_a).to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = ops.similarity_range(qin, Gd, tin, k, g_offset=OFF)                  # (also sets the kernels' one-time attributes before the capture)
    side.synchronize()
    _assert_same(got, want_a, "side stream")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.similarity_range(qin, Gd, tin, k, g_offset=OFF)
    for n, (q_, t_, want) in enumerate(((Q, thr_a, want_a), (Qb, thr_b, want_b), (Q, thr_a, want_a))):
        qin.copy_(q_.to(DEV)); tin.copy_(torch.from_numpy(t_).to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        _assert_same(out, want, f"graph replay {n}")

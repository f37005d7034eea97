"""GPU tests of the k-reciprocal re-ranking (cor_knn_reciprocal, cor_rerank_reciprocal, ops.knn_reciprocal / rerank_reciprocal,
GalleryShard / GallerySet .neighbour_graph and .rerank, reranked_search). Every comparison is bitwise on scores (.view(int32)), ids and
positions. The references are tests/test_cpu_rerank.ref_prune / ref_rerank, the NumPy restatements of the definitions in
include/cor_amd.h, fed the GPU searches' own lists so that only the new kernels are under test; they never call the code under test."""
import functools

import numpy as np
import pytest
import torch

from tests.test_cpu_rerank import ref_prune, ref_rerank

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
INT64_MIN, INT64_MAX = -2 ** 63, 2 ** 63 - 1
BIG = 2 ** 33 + 5


def _unit(n, C, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn((n, C), generator=g), dim=-1)


def _np(t):
    return t.detach().cpu().numpy()


def _same(got, want, what=""):
    """got: the (scores, idx[, pos]) device tensors of a re-ranking; want: ref_rerank's arrays. Bitwise."""
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.int64 and tuple(got[0].shape) == want[0].shape, what
    assert np.array_equal(_np(got[1]), want[1]), f"ids differ {what}"
    assert np.array_equal(_np(got[0]).view(np.int32), want[0].view(np.int32)), f"score bits differ {what}"
    if len(got) > 2:
        assert got[2].dtype == torch.int32 and np.array_equal(_np(got[2]), want[2]), f"positions differ {what}"


def _graph_np(graph):
    return [(_np(r), _np(t), o) for r, t, o in graph.segments]


def _lists(nb, rows, k1, batch):
    """The searches a graph build makes, batch by batch: (scores, idx) of `rows` in `nb`."""
    res = [nb.search(rows[lo:lo + batch], k1) for lo in range(0, rows.shape[0], batch)]
    return torch.cat([r[0] for r in res]), torch.cat([r[1] for r in res])


# ------------------------------------------------------------------------------------------------------------------ graph pruning

PRUNE = [(Ng, k1, n % 3, (0, BIG)[n // 3 % 2]) for n, (Ng, k1) in enumerate((Ng, k1) for Ng in (1, 7, 300, 2000) for k1 in (1, 5, 20, 64, 256))]


def test_prune_cases_cover_every_axis_value():
    assert len(PRUNE) == 20 and {c[2] for c in PRUNE} == {0, 1, 2} and {c[3] for c in PRUNE} == {0, BIG}
    assert {(c[2], c[3]) for c in PRUNE} == {(d, o) for d in range(3) for o in (0, BIG)}


@pytest.mark.parametrize("Ng,k1,dt,offset", PRUNE)
def test_neighbour_graph_of_a_shard(Ng, k1, dt, offset):
    from cor_amd.retrieval import GalleryShard
    sh = GalleryShard(_unit(Ng, 64, 30 + Ng).to(DTYPES[dt]).to(DEV), offset=offset)
    batch = (4096, 128, 7)[k1 % 3]                                     # above, not dividing, far below the row count
    graph = sh.neighbour_graph(k1, batch=batch)
    s, i = _lists(sh, sh.rows, k1, batch)
    assert graph.width == k1 and graph.offsets == (offset,) and graph.lengths == (Ng,) and len(graph.segments) == 1
    assert torch.equal(i[:, 0].cpu(), torch.arange(Ng) + offset)       # a row finds itself first
    want = ref_prune([(_np(i), offset)])[0]
    assert np.array_equal(_np(graph.rnbr[0]), want) and graph.rnbr[0].dtype == torch.int64
    assert np.array_equal(_np(graph.kth[0]).view(np.int32), _np(s[:, k1 - 1]).view(np.int32))
    assert (want[:, 0] == np.arange(Ng) + offset).all()                # and stays in its own reciprocal list
    if k1 > Ng:
        assert (want[:, Ng:] == -1).all() and np.isneginf(_np(graph.kth[0])).all()


def test_pruning_writes_a_buffer_of_its_own_and_tests_ids_first():
    from cor_amd import ops
    o = BIG
    nbr = torch.tensor([[o + 1, o + 2, -1, INT64_MIN], [o, o + 1, INT64_MAX, o + 3], [o + 3, o + 2 ** 32, o - 1, o + 1], [o + 4, o + 2, -2, o + 1]],
                       dtype=torch.int64)
    dev, before = nbr.to(DEV), nbr.clone()
    out = ops.knn_reciprocal([(dev, o)], 0)
    assert out.data_ptr() != dev.data_ptr() and torch.equal(dev.cpu(), before)
    assert np.array_equal(_np(out), ref_prune([(nbr.numpy(), o)])[0])
    assert _np(out).tolist() == [[o + 1, -1, -1, -1], [o, o + 1, -1, o + 3], [o + 3, -1, -1, -1], [-1, o + 2, -1, o + 1]]
    into = torch.zeros_like(dev)
    assert ops.knn_reciprocal([(dev, o)], 0, out=into) is into and torch.equal(into, out)


@pytest.mark.parametrize("base", [0, BIG])
def test_neighbour_graph_of_a_set(base):
    from cor_amd.retrieval import GallerySet, GalleryShard
    G, k1 = _unit(300, 64, 41).to(DEV), 20
    gs = GallerySet([GalleryShard(G[220:], offset=base + 250), GalleryShard(G[:100], offset=base), GalleryShard(G[100:100], offset=base + 500),
                     GalleryShard(G[100:220], offset=base + 130)])      # out of order, ids base + 100 .. 129 in no segment, one empty
    graph = gs.neighbour_graph(k1, batch=64)
    live = [sh for sh in gs.segments if len(sh)]
    assert graph.offsets == (base, base + 130, base + 250) and graph.lengths == (100, 120, 80) and graph.width == k1
    lists = [_lists(gs, sh.rows, k1, 64) for sh in live]
    want = ref_prune([(_np(i), int(sh.offset)) for sh, (_, i) in zip(live, lists)])
    for n, (sh, (s, _)) in enumerate(zip(live, lists)):
        assert np.array_equal(_np(graph.rnbr[n]), want[n]), f"segment {n}"
        assert np.array_equal(_np(graph.kth[n]).view(np.int32), _np(s[:, k1 - 1]).view(np.int32))
    assert sum((w >= 0).sum() for w in want) > 300 and any((w == -1).any() for w in want)
    whole = GalleryShard(G, offset=7).neighbour_graph(k1)              # the same rows as one shard: the same graph, ids shifted
    ids = np.concatenate(want)
    spans = ((base + 250, 80, 227), (base + 130, 120, 107), (base, 100, 7))    # each id to the whole shard's id of its row, all from the ids as they were
    cat = np.select([(ids >= lo) & (ids < lo + n) for lo, n, _ in spans], [ids - lo + first for lo, _, first in spans], default=-1)
    assert (cat >= 0).sum() == (ids >= 0).sum() and np.array_equal(_np(whole.rnbr[0]), cat)


# --------------------------------------------------------------------------------------------------------------------- re-ranking

@functools.lru_cache(maxsize=None)
def _synthetic(kg, k1):
    """A random graph of 5000 rows at offset 100 whose lists draw from a pool of low ids, so that A and B meet often; about a third
    of the slots are -1; no id twice in a row. -> (rnbr i64 [5000,kg], kth f32 [5000], pool size), NumPy, shared and never changed."""
    rng = np.random.default_rng(1000 * kg + k1)
    Ng, pool = 5000, max(2 * k1 + 40, kg + 10)
    rnbr = np.argsort(rng.random((Ng, pool)), axis=1)[:, :kg].astype(np.int64) + 100
    rnbr[rng.random((Ng, kg)) < 0.3] = -1
    return rnbr, rng.uniform(0.0, 1.0, Ng).astype(np.float32), pool


def _synthetic_lists(Bq, kin, k1, pool, seed):
    """Lists of pairwise different ids, the first k1 of them out of the pool, scores descending in (0, 1); every seventh entry missing."""
    rng = np.random.default_rng(seed)
    idx, sc = np.empty((Bq, kin), np.int64), np.empty((Bq, kin), np.float32)
    for b in range(Bq):
        low = rng.permutation(pool)
        idx[b] = np.concatenate([low[:k1], rng.permutation(np.concatenate([low[k1:], np.arange(pool, 5000)]))[:kin - k1]]) + 100
        sc[b] = np.sort(rng.uniform(0.0, 1.0, kin).astype(np.float32))[::-1]
    miss = rng.random((Bq, kin)) < 1 / 7
    idx[miss], sc[miss] = rng.choice([-1, 99, 5100, INT64_MIN, INT64_MAX], int(miss.sum())), np.nan
    return sc, idx


def _grid():
    """About 40 of the combinations of the issue's grid, drawn with a fixed seed; every value of every axis occurs. k1 <= kin is kept
    by clipping k1, so kin = 1 meets k1 = 1 only."""
    rng = np.random.default_rng(20261019)
    axes = dict(Bq=[1, 5, 130], kin=[1, 20, 100, 256, 1000, 4096], k1=[1, 5, 20, 256], kg=[1, 20, 256], k=[1, 10, 256], lam=[0.0, 0.3, 1.0])
    out = []
    for n in range(40):
        Bq, kin, k1, kg, k, lam = (v[n % len(v)] if n < 6 else v[int(rng.integers(len(v)))] for v in axes.values())
        out.append((Bq if kin < 4096 or kg < 256 else min(Bq, 5), kin, min(k1, kin), kg, k, lam))
    return out


GRID = _grid()


def test_grid_covers_every_axis_value():
    assert len(set(GRID)) >= 36 and all(g[2] <= g[1] for g in GRID)
    for pos, values in enumerate(([1, 5, 130], [1, 20, 100, 256, 1000, 4096], [1, 5, 20, 256], [1, 20, 256], [1, 10, 256], [0.0, 0.3, 1.0])):
        assert {g[pos] for g in GRID} >= set(values)                    # (k1 clipped to kin adds values of its own)


@pytest.mark.parametrize("Bq,kin,k1,kg,k,lam", GRID)
def test_grid_bitwise(Bq, kin, k1, kg, k, lam):
    from cor_amd import ops
    rnbr, kth, pool = _synthetic(kg, k1)
    sc, idx = _synthetic_lists(Bq, kin, k1, pool, Bq + kin + k1 + kg + k)
    got = ops.rerank_reciprocal(torch.from_numpy(sc).to(DEV), torch.from_numpy(idx).to(DEV), [(torch.from_numpy(rnbr).to(DEV), torch.from_numpy(kth).to(DEV), 100)],
                                k1, lam, k, return_pos=True)
    want = ref_rerank(sc, idx, [(rnbr, kth, 100)], k1, lam, k)
    _same(got, want)
    if kin >= 100 and k1 >= 5 and kg >= 20 and lam < 1:                # the Jaccard term is at work: some f is not lam * score
        assert (want[0] != np.float32(lam) * sc[np.arange(Bq)[:, None], np.maximum(want[2], 0)]).any()


@pytest.mark.parametrize("gdt", DTYPES)
def test_lists_from_a_search(gdt):
    from cor_amd.retrieval import GalleryShard
    sh = GalleryShard(_unit(2000, 64, 42).to(gdt).to(DEV), offset=500)
    Q = _unit(37, 64, 43).to(DEV)
    graph = sh.neighbour_graph(20)
    s, i = sh.search(Q, 100)
    for k1, lam, k in ((None, 0.3, None), (5, 0.0, 10), (20, 1.0, 100)):
        got = sh.rerank(s, i, graph, k1=k1, lam=lam, k=k)
        want = ref_rerank(_np(s), _np(i), _graph_np(graph), k1 or 20, lam, k or 100)
        _same(got, want, what=f"k1={k1} lam={lam}")
        if lam == 1.0:                                                 # the input order, and the scores as they were
            assert torch.equal(got[1], i) and torch.equal(got[0], s)
    plain = sh.rerank(s, i, graph, lam=0.3, k=100)
    assert (plain[1] != i).any()                                       # the Jaccard term does re-order something here


@pytest.mark.parametrize("offset", [0, BIG])
def test_hostile_lists(offset):
    from cor_amd import ops
    from cor_amd.retrieval import GalleryShard
    Ng, kg, kin = 50, 6, 12
    sh = GalleryShard(_unit(Ng, 64, 44).to(DEV), offset=offset)
    graph = sh.neighbour_graph(kg)
    segs = graph.segments
    nan, inf = float("nan"), float("inf")
    o = offset
    idx = torch.tensor([
        [o + 3, o + 4, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1],                                  # a -1 tail
        [o + Ng, o - 1, o + 7, o + 10 ** 12, 5 - o - 100, o + 8, INT64_MIN, INT64_MAX, o + 9, -2, o + Ng - 1, o],   # ids of no segment between real ones
        [INT64_MIN, INT64_MAX, INT64_MIN + 1, INT64_MAX - 1, o + 2 ** 31, o + 2 ** 32, o - 2 ** 32, -1, -1, -1, -1, o + 1],
        [-1] * 12,                                                                               # nothing present
        [o + Ng, o + Ng + 1, o - 1, o - 2, INT64_MAX, INT64_MIN, -1, -1, -1, -1, -1, -1],        # nothing present, hostile
        [o + 1, o + 2, o + 3, o + 4, o + 5, o + 6, o + 7, o + 8, o + 9, o + 10, o + 11, o + 12],  # +-0.0 scores: ties by id
        [o + 31, o + 30, o + 29, o + 28, o + 27, o + 26, o + 25, o + 24, o + 23, o + 22, o + 21, o + 20],   # the same, ids descending
        [o + 20, -1, o + 21, -1, o + 22, -1, o + 23, -1, o + 24, -1, o + 25, -1]], dtype=torch.int64)
    sc = torch.tensor([
        [0.9, 0.8, nan, -inf, inf, nan, nan, nan, nan, nan, nan, nan],
        [nan, nan, 0.7, nan, -inf, 0.6, nan, inf, 0.5, nan, 0.4, 0.3],
        [nan, -inf, inf, nan, nan, nan, nan, nan, nan, nan, nan, 0.5],
        [nan] * 12,
        [nan, inf, -inf, nan, 1.0, 1.0, 1.0, nan, nan, nan, nan, nan],
        [0.0, -0.0, 0.0, -0.0, 0.0, -0.0, 0.0, -0.0, 0.0, -0.0, 0.0, -0.0],
        [-0.0, 0.0, -0.0, 0.0, -0.0, 0.0, -0.0, 0.0, -0.0, 0.0, -0.0, 0.0],
        [0.5, nan, 0.5, -inf, 0.5, inf, 0.5, nan, 0.5, nan, 0.5, nan]], dtype=torch.float32)
    for k1, lam, k in ((6, 0.3, 12), (12, 0.0, 5), (1, 1.0, 12), (3, 0.5, 1), (6, 1.5, 12)):
        got = ops.rerank_reciprocal(sc.to(DEV), idx.to(DEV), segs, k1, lam, k, return_pos=True)
        want = ref_rerank(sc.numpy(), idx.numpy(), _graph_np(graph), k1, lam, k)
        assert not np.isnan(want[0]).any()
        _same(got, want, what=f"k1={k1} lam={lam} k={k}")
        assert (got[1][3] == -1).all() and (got[1][4] == -1).all() and torch.isneginf(got[0][3]).all() and (got[2][4] == -1).all()
        if lam == 1.0:
            assert got[1][5].tolist() == [o + 1 + n for n in range(12)] and got[1][6].tolist() == [o + 20 + n for n in range(12)]
    none = ops.rerank_reciprocal(sc.to(DEV), idx.to(DEV), [], 6, 0.3, 4, return_pos=True)     # no segment at all: every entry is missing
    assert torch.isneginf(none[0]).all() and (none[1] == -1).all() and (none[2] == -1).all()
    other = [(segs[0][0], segs[0][1], o + 10 ** 6)]                     # another shard's graph: every entry is missing for it, too
    assert (ops.rerank_reciprocal(sc.to(DEV), idx.to(DEV), other, 6, 0.3, 4)[1] == -1).all()


def test_ties_empty_a_and_empty_union():
    from cor_amd import ops
    from cor_amd.retrieval import GalleryShard
    half = _unit(150, 64, 45)
    sh = GalleryShard(torch.cat([half, half]).to(DEV), offset=10)       # every row twice: rows g and g + 150 score alike everywhere
    graph = sh.neighbour_graph(8)
    s, i = sh.search(_unit(21, 64, 46).to(DEV), 40)
    want = ref_rerank(_np(s), _np(i), _graph_np(graph), 8, 0.3, 40)
    _same(sh.rerank(s, i, graph), want, what="duplicated rows")
    f = want[0]
    pairs = (f[:, :-1] == f[:, 1:])
    assert pairs.sum() >= 21 and (want[1][:, :-1][pairs] < want[1][:, 1:][pairs]).all()        # equal f: the lower id first
    # an empty A: no row counts the query among its nearest (kth above every score); J = +0 everywhere, the order is the scores'
    rnbr = graph.rnbr[0]
    high = [(rnbr, torch.full_like(graph.kth[0], 2.0), 10)]
    got = ops.rerank_reciprocal(s, i, high, 8, 0.3, 40, return_pos=True)
    _same(got, ref_rerank(_np(s), _np(i), [(_np(rnbr), np.full(300, 2.0, np.float32), 10)], 8, 0.3, 40), what="empty A")
    assert torch.equal(got[0].cpu(), torch.from_numpy(np.float32(0.3) * _np(s)[np.arange(21)[:, None], _np(got[2])]))   # f = lam * score + 0
    # U == 0: A empty and every list empty
    bare = torch.full_like(rnbr, -1)
    got = ops.rerank_reciprocal(s, i, [(bare, high[0][1], 10)], 8, 0.0, 40)
    _same(got, ref_rerank(_np(s), _np(i), [(_np(bare), np.full(300, 2.0, np.float32), 10)], 8, 0.0, 40), what="U == 0")
    assert (got[0] == 0).all() and not torch.signbit(got[0]).any() and torch.equal(got[1], torch.sort(i, dim=1).values)


def test_gallery_set_rerank_equals_one_shard():
    from cor_amd.retrieval import GallerySet, GalleryShard
    Ng, k1, kin = 300, 20, 60
    Q = _unit(9, 256, 48).to(DEV)
    for gdt in DTYPES:
        G = _unit(Ng, 256, 47).to(gdt).to(DEV)
        whole = GalleryShard(G, offset=40)
        parts = GallerySet([GalleryShard(G[170:], offset=210), GalleryShard(G[:90], offset=40), GalleryShard(G[90:90], offset=1000),
                            GalleryShard(G[90:170], offset=130)])
        gw, gp = whole.neighbour_graph(k1), parts.neighbour_graph(k1, batch=50)
        assert torch.equal(torch.cat(gp.rnbr), gw.rnbr[0]) and torch.equal(torch.cat(gp.kth).view(torch.int32), gw.kth[0].view(torch.int32))
        s, i = whole.search(Q, kin)
        for kw in (dict(), dict(k1=5, lam=0.0, k=7)):
            a, b = whole.rerank(s, i, gw, **kw), parts.rerank(s, i, gp, **kw)
            assert torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
        _same(parts.rerank(s, i, gp), ref_rerank(_np(s), _np(i), _graph_np(gp), k1, 0.3, kin), what=str(gdt))
    z = GallerySet().rerank(s, i, GallerySet().neighbour_graph(k1), k=3)
    assert z[0].shape == (9, 3) and torch.isneginf(z[0]).all() and (z[1] == -1).all()


@pytest.mark.parametrize("mode", ["plain", "ne", "distinct"])
def test_reranked_search_is_the_composition(mode):
    from cor_amd import retrieval
    from cor_amd.retrieval import GalleryShard
    Ng, Bq, k, kc = 600, 17, 10, 50
    G, Q = _unit(Ng, 64, 49).to(torch.bfloat16), _unit(Bq, 64, 50).to(DEV)
    rng = np.random.default_rng(51)
    labels, groups = torch.from_numpy(rng.integers(0, 4, Ng).astype(np.int32)), torch.from_numpy(rng.integers(0, 150, Ng).astype(np.int32))
    sh = GalleryShard(G.to(DEV), offset=77, labels=labels, groups=groups)
    graph = sh.neighbour_graph(12)
    kw = dict(plain={}, ne=dict(query_labels=torch.from_numpy(rng.integers(0, 4, Bq).astype(np.int32)).to(DEV), mode="ne"), distinct=dict(distinct=True))[mode]
    for k1, lam in ((None, 0.3), (6, 0.6)):
        gs, gi = retrieval.reranked_search(Q, sh, graph, k, kc, k1=k1, lam=lam, **kw)
        s, i = sh.search(Q, kc, **kw)
        _same((gs, gi), ref_rerank(_np(s), _np(i), _graph_np(graph), k1 or 12, lam, k), what=f"{mode} k1={k1}")
        assert gs.is_cuda and gi.is_cuda and gs.shape == (Bq, k)


def test_side_stream_and_graph_replay():
    from cor_amd import ops
    rnbr, kth, pool = _synthetic(20, 20)
    sc, idx = _synthetic_lists(130, 100, 20, pool, 52)
    segs = [(torch.from_numpy(rnbr[:2500]).to(DEV), torch.from_numpy(kth[:2500]).to(DEV), 100),
            (torch.from_numpy(rnbr[2500:]).to(DEV), torch.from_numpy(kth[2500:]).to(DEV), 2600)]
    s, i = torch.from_numpy(sc).to(DEV), torch.from_numpy(idx).to(DEV)
    eager = ops.rerank_reciprocal(s, i, segs, 20, 0.3, 10, return_pos=True)
    _same(eager, ref_rerank(sc, idx, [(rnbr, kth, 100)], 20, 0.3, 10))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = ops.rerank_reciprocal(s, i, segs, 20, 0.3, 10, return_pos=True)
    side.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(on_side, eager))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.rerank_reciprocal(s, i, segs, 20, 0.3, 10, return_pos=True)
    for t in out:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0].view(torch.int32), eager[0].view(torch.int32)) and torch.equal(out[1], eager[1]) and torch.equal(out[2], eager[2])


def test_a_stale_graph_is_refused_after_add_and_drop():
    from cor_amd.retrieval import GallerySet, GalleryShard
    G = _unit(120, 64, 53).to(DEV)
    gs = GallerySet([GalleryShard(G[:50], offset=0), GalleryShard(G[50:90], offset=50)])
    graph = gs.neighbour_graph(5)
    s, i = gs.search(G[:4], 10)
    gs.rerank(s, i, graph)
    gs.add(GalleryShard(G[90:90], offset=500))                         # an empty segment changes nothing
    gs.rerank(s, i, graph)
    gs.add(GalleryShard(G[90:], offset=90))
    with pytest.raises(ValueError, match="build a new graph"):
        gs.rerank(s, i, graph)
    gs.drop(90)
    gs.rerank(s, i, graph)                                             # the segments it was built from again
    gs.drop(0)
    with pytest.raises(ValueError, match="build a new graph"):
        gs.rerank(s, i, graph)
    with pytest.raises(ValueError, match="build a new graph"):
        GalleryShard(G[:50], offset=0).rerank(s, i, graph)
    _, i2 = gs.search(G[:4], 10)
    assert gs.rerank(s, i2, gs.neighbour_graph(5))[0].shape == (4, 10)

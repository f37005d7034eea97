"""GPU tests of the query expansion (cor_expand_queries, ops.expand_queries, GalleryShard / GallerySet .expand and .augmented,
expanded_search). Every comparison of an expansion is bitwise (.view(int32 / int16)). The reference is tests/test_cpu_expand.ref_expand,
the NumPy float32 restatement of the definition in include/cor_amd.h, with torch CPU casts for the 16-bit outputs; it never calls the code
under test."""
import numpy as np
import pytest
import torch

from tests.test_cpu_expand import ref_expand, to_dtype

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
INT64_MIN, INT64_MAX = -2 ** 63, 2 ** 63 - 1
BIG = 2 ** 33 + 5


def _unit(n, C, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn((n, C), generator=g), dim=-1)


def _wide(rows):
    """Stored rows (CPU tensor of any gallery dtype) -> the f32 ndarray of the values the kernel reads."""
    return rows.float().numpy()


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same(got, want_f32, out_dtype=torch.float32, what=""):
    want = to_dtype(want_f32, out_dtype)
    assert got.dtype == out_dtype and tuple(got.shape) == tuple(want.shape), what
    assert torch.equal(_bits(got), _bits(want)), f"bits differ {what}"


def _lists(Bq, kin, lo, hi, seed):
    rng = np.random.default_rng(seed)
    return (torch.from_numpy(rng.uniform(0.1, 1.0, (Bq, kin)).astype(np.float32)), torch.from_numpy(rng.integers(lo, hi, (Bq, kin)).astype(np.int64)))


def _grid():
    """About 60 of the combinations of the issue's grid, drawn with a fixed seed; every value of every axis occurs."""
    rng = np.random.default_rng(20261018)
    axes = dict(C=[16, 48, 64, 256], m=[1, 3, 10, 64, 256], extra=[0, 7], Bq=[1, 5, 130], alpha=[0, 1, 3, 8], qw=[0.0, 1.0, 0.5],
                normalize=[True, False], gdt=[0, 1, 2], odt=[0, 1, 2])
    return [tuple(v[n % len(v)] if n < 5 else v[int(rng.integers(len(v)))] for v in axes.values()) for n in range(60)]


GRID = _grid()


def test_grid_covers_every_axis_value():
    assert len(set(GRID)) >= 55
    for pos, n in enumerate((4, 5, 2, 3, 4, 3, 2, 3, 3)):
        assert len({g[pos] for g in GRID}) == n


@pytest.mark.parametrize("C,m,extra,Bq,alpha,qw,normalize,gdt,odt", GRID)
def test_grid_bitwise(C, m, extra, Bq, alpha, qw, normalize, gdt, odt):
    from cor_amd import ops
    gdt, odt, kin, Ng = DTYPES[gdt], DTYPES[odt], m + extra, 300
    G = _unit(Ng, C, 1).to(gdt)
    Q = _unit(Bq, C, 2)
    s, i = _lists(Bq, kin, 0, Ng, C + m + Bq)
    got = ops.expand_queries(Q.to(DEV), [(G.to(DEV), 0)], s.to(DEV), i.to(DEV), m, alpha=alpha, query_weight=qw, normalize=normalize, out_dtype=odt)
    _same(got, ref_expand(Q.numpy(), qw, [(_wide(G), 0)], s.numpy(), i.numpy(), m, alpha, normalize), odt)


@pytest.mark.parametrize("gdt", DTYPES)
def test_lists_from_a_search(gdt):
    from cor_amd.retrieval import GalleryShard
    G, Q, m = _unit(2000, 256, 3).to(gdt), _unit(37, 256, 4), 10
    sh = GalleryShard(G.to(DEV), offset=500)
    s, i = sh.search(Q.to(DEV), m)
    got = sh.expand(Q.to(DEV), s, i, m)
    _same(got, ref_expand(Q.numpy(), 1.0, [(_wide(G), 500)], s.cpu().numpy(), i.cpu().numpy(), m, 3, True))


@pytest.mark.parametrize("offset", [0, BIG])
@pytest.mark.parametrize("gdt", DTYPES)
def test_hostile_lists(gdt, offset):
    from cor_amd import ops
    C, Ng, kin = 64, 50, 12
    G, Q = _unit(Ng, C, 5).to(gdt), _unit(8, C, 6)
    nan, inf = float("nan"), float("inf")
    o = offset
    idx = torch.tensor([
        [o + 3, o + 4, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1],                                  # a -1 tail
        [o + Ng, o - 1, o + 7, o + 10 ** 12, 5 - o, o + 8, INT64_MIN, INT64_MAX, o + 9, -2, o + Ng - 1, o],   # ids of no segment between real ones
        [INT64_MIN, INT64_MAX, INT64_MIN + 1, INT64_MAX - 1, o + 2 ** 31, o + 2 ** 32, o - 2 ** 32, -1, -1, -1, -1, o + 1],
        [o + 5, o + 5, o + 6, o + 5, o + 6, o + 5, o + 5, o + 5, o + 5, o + 5, o + 5, o + 5],    # a repeated id
        [-1] * 12,                                                                               # nothing present
        [o + Ng, o + Ng + 1, o - 1, o - 2, INT64_MAX, INT64_MIN, -1, -1, -1, -1, -1, -1],        # nothing present, hostile
        [o + 1, o + 2, o + 3, o + 4, o + 5, o + 6, o + 7, o + 8, o + 9, o + 10, o + 11, o + 12],  # weights of +0 on present entries
        [o + 20, -1, o + 21, -1, o + 22, -1, o + 23, -1, o + 24, -1, o + 25, -1]], dtype=torch.int64)
    sc = torch.tensor([
        [0.9, 0.8, nan, -inf, inf, nan, nan, nan, nan, nan, nan, nan],
        [nan, nan, 0.7, nan, -inf, 0.6, nan, inf, 0.5, nan, 0.4, 0.3],
        [nan, -inf, inf, nan, nan, nan, nan, nan, nan, nan, nan, 0.5],
        [0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3, 0.2, 0.1, 0.9, 0.8, 0.7],
        [nan] * 12,
        [nan, inf, -inf, nan, 1.0, 1.0, 1.0, nan, nan, nan, nan, nan],
        [-0.5, -0.0, 0.0, -inf, 0.7, -1e-30, -3.0, 0.2, -0.0, 0.0, -1.0, 0.9],
        [0.5, nan, 0.5, -inf, 0.5, inf, 0.5, nan, 0.5, nan, 0.5, nan]], dtype=torch.float32)
    for alpha, qw, normalize, m in ((1, 0.0, True, 12), (3, 1.0, True, 12), (0, 0.5, False, 12), (2, 0.0, False, 11)):
        got = ops.expand_queries(Q.to(DEV), [(G.to(DEV), offset)], sc.to(DEV), idx.to(DEV), m, alpha=alpha, query_weight=qw, normalize=normalize)
        want = ref_expand(Q.numpy(), qw, [(_wide(G), offset)], sc.numpy(), idx.numpy(), m, alpha, normalize)
        assert np.isfinite(want).all()
        _same(got, want, what=f"alpha={alpha} qw={qw}")
        if qw == 0.0:
            assert not got[4].any() and not got[5].any()                # nothing to sum: a zero row, no NaN
    got = ops.expand_queries(Q.to(DEV), [], sc.to(DEV), idx.to(DEV), 12, query_weight=0.0, out=torch.full((8, C), 7.0, device=DEV))
    assert not got.any()                                               # no segment at all: every entry is missing


def _cut(G, bounds, order, dtypes, base=0):
    """Segments [(rows, offset)] of G cut at `bounds` (pairs of row ranges), listed in `order`, each in its dtype."""
    return [(G[bounds[n][0]:bounds[n][1]].to(dtypes[n % len(dtypes)]), base + bounds[n][0]) for n in order]


@pytest.mark.parametrize("base", [0, BIG])
def test_segments(base):
    from cor_amd import ops
    C, Ng, Bq, kin, m = 64, 300, 21, 40, 33
    G32, Q = _unit(Ng, C, 7), _unit(Bq, C, 8)
    s, i = _lists(Bq, kin, base - 5, base + Ng + 5, 9)
    dev = lambda segs: [(r.to(DEV), o) for r, o in segs]
    run = lambda segs, **kw: ops.expand_queries(Q.to(DEV), dev(segs), s.to(DEV), i.to(DEV), m, **kw)
    ref = lambda segs, **kw: ref_expand(Q.numpy(), 1.0, [(_wide(r), o) for r, o in segs], s.numpy(), i.numpy(), m, kw.get("alpha", 3), True)
    sixteen = [(n * 19, n * 19 + 19) for n in range(15)] + [(285, 300)]
    three = [(0, 120), (120, 121), (121, 300)]
    for gdt in DTYPES:                                                 # equal dtypes, every row in some segment: the bits of the single shard
        G = G32.to(gdt)
        one = run([(G, base)])
        _same(one, ref([(G, base)]), what=f"one segment {gdt}")
        for bounds, order in ((three, [2, 0, 1]), (sixteen, [5, 15, 0, 9, 3, 12, 1, 14, 7, 2, 11, 4, 13, 6, 10, 8])):
            got = run(_cut(G, bounds, order, [gdt], base))
            assert torch.equal(_bits(got), _bits(one)), f"{len(bounds)} segments of {gdt} differ from the single shard"
    gap = [(0, 100), (100, 100), (130, 300), (110, 120)]               # an empty segment, rows 100..109 and 120..129 in no segment
    for dts in (DTYPES, [torch.bfloat16, torch.float16], [torch.float32]):
        for bounds, order in ((gap, [2, 1, 3, 0]), (three, [1, 2, 0]), (sixteen, list(range(15, -1, -1)))):
            segs = _cut(G32, bounds, order, dts, base)
            for alpha in (0, 3):
                _same(run(segs, alpha=alpha), ref(segs, alpha=alpha), what=f"{len(bounds)} segments {dts}")
    segs = _cut(G32, gap, [0, 1, 2, 3], DTYPES, base)
    _same(run(segs, out_dtype=torch.bfloat16), ref(segs), torch.bfloat16)


def test_gallery_set_expand_equals_one_shard():
    from cor_amd.retrieval import GallerySet, GalleryShard
    C, Ng, Bq, m = 256, 300, 9, 20
    Q = _unit(Bq, C, 11).to(DEV)
    for gdt in DTYPES:
        G = _unit(Ng, C, 10).to(gdt).to(DEV)
        whole = GalleryShard(G, offset=40)
        parts = GallerySet([GalleryShard(G[170:], offset=210), GalleryShard(G[:90], offset=40), GalleryShard(G[90:90], offset=1000),
                            GalleryShard(G[90:170], offset=130)])
        s, i = whole.search(Q, m)
        for kw in (dict(), dict(alpha=0, query_weight=0.0, normalize=False, out_dtype=torch.float16)):
            a, b = whole.expand(Q, s, i, m, **kw), parts.expand(Q, s, i, m, **kw)
            assert a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))
        _same(parts.expand(Q, s, i, m), ref_expand(Q.cpu().numpy(), 1.0, [(_wide(G.cpu()), 40)], s.cpu().numpy(), i.cpu().numpy(), m, 3, True))
    z = GallerySet().expand(Q, s, i, m, query_weight=0.0)
    assert z.shape == (Bq, C) and not z.any()


@pytest.mark.parametrize("rounds", [1, 2])
@pytest.mark.parametrize("mode", ["plain", "ne", "distinct"])
def test_expanded_search_is_the_composition(mode, rounds):
    from cor_amd import retrieval
    from cor_amd.retrieval import GalleryShard
    C, Ng, Bq, k, m = 256, 600, 17, 10, 5
    G, Q = _unit(Ng, C, 12).to(torch.bfloat16), _unit(Bq, C, 13)
    rng = np.random.default_rng(14)
    labels, groups = torch.from_numpy(rng.integers(0, 4, Ng).astype(np.int32)), torch.from_numpy(rng.integers(0, 150, Ng).astype(np.int32))
    sh = GalleryShard(G.to(DEV), offset=77, labels=labels, groups=groups)
    kw = dict(plain={}, ne=dict(query_labels=torch.from_numpy(rng.integers(0, 4, Bq).astype(np.int32)).to(DEV), mode="ne"), distinct=dict(distinct=True))[mode]
    for alpha, qw in ((3, 1.0), (0, 0.5)):
        gs, gi, gq = retrieval.expanded_search(Q.to(DEV), sh, k, m, alpha=alpha, query_weight=qw, rounds=rounds, **kw)
        q = Q
        for _ in range(rounds):
            s, i = sh.search(q.to(DEV), m, **kw)
            q = torch.from_numpy(ref_expand(q.numpy(), qw, [(_wide(G), 77)], s.cpu().numpy(), i.cpu().numpy(), m, alpha, True))
        ws, wi = sh.search(q.to(DEV), k, **kw)
        _same(gq, q.numpy(), what=f"expanded queries {mode} rounds={rounds}")
        assert torch.equal(gi, wi) and torch.equal(_bits(gs), _bits(ws))
        assert gs.is_cuda and gi.is_cuda and gq.is_cuda and gs.shape == (Bq, k)


@pytest.mark.parametrize("gdt,odt", [(torch.float32, None), (torch.bfloat16, None), (torch.float16, torch.float32), (torch.float32, torch.bfloat16)])
def test_augmented_shard(gdt, odt):
    from cor_amd.retrieval import GalleryShard
    C, Ng, m = 64, 203, 4
    G = _unit(Ng, C, 15).to(gdt)
    labels, groups = torch.arange(Ng, dtype=torch.int32) % 7, torch.arange(Ng, dtype=torch.int32) // 3
    sh = GalleryShard(G.to(DEV), offset=BIG, labels=labels, groups=groups)
    before = sh.rows.clone()
    s, i = sh.search(sh.rows.float(), m)
    assert torch.equal(i[:, 0].cpu(), torch.arange(Ng) + BIG)          # a row finds itself first
    want = ref_expand(None, 0.0, [(_wide(G), BIG)], s.cpu().numpy(), i.cpu().numpy(), m, 3, True)
    outs = []
    for batch in (4096, Ng, 50, 64, 1):                                # larger than, equal to, not dividing, smaller than the row count
        if batch == 1 and gdt != torch.float32:
            continue
        aug = sh.augmented(m, batch=batch, dtype=odt)
        assert aug is not sh and aug.offset == BIG and len(aug) == Ng and aug.rows.dtype == (odt or gdt)
        assert torch.equal(aug.labels, sh.labels) and torch.equal(aug.groups, sh.groups)
        _same(aug.rows, want, odt or gdt, what=f"batch={batch}")
        outs.append(aug)
    assert torch.equal(_bits(sh.rows), _bits(before)) and sh.rows.data_ptr() != outs[0].rows.data_ptr()
    other = GalleryShard(_unit(90, C, 16).to(DEV), offset=5)           # neighbours that are another gallery
    s2, i2 = other.search(sh.rows.float(), m)
    _same(sh.augmented(m, alpha=1, neighbours=other).rows, ref_expand(None, 0.0, [(_wide(other.rows.cpu()), 5)], s2.cpu().numpy(), i2.cpu().numpy(), m, 1, True), gdt)


def test_augmented_set():
    from cor_amd.retrieval import GallerySet, GalleryShard
    C, Ng, m = 64, 180, 5
    G = _unit(Ng, C, 17)
    parts = [GalleryShard(G[:70].to(torch.bfloat16).to(DEV), offset=0, groups=torch.arange(70)), GalleryShard(G[70:].to(DEV), offset=100, groups=torch.arange(110))]
    gs = GallerySet(parts)
    before = [p.rows.clone() for p in parts]
    aug = gs.augmented(m, alpha=2, batch=64)
    assert isinstance(aug, GallerySet) and [int(a.offset) for a in aug.segments] == [0, 100] and len(aug) == Ng
    segs = [(_wide(p.rows.cpu()), int(p.offset)) for p in parts]
    for p, a, b in zip(parts, aug.segments, before):
        s, i = gs.search(p.rows.float(), m)
        _same(a.rows, ref_expand(None, 0.0, segs, s.cpu().numpy(), i.cpu().numpy(), m, 2, True), p.rows.dtype)
        assert torch.equal(_bits(p.rows), _bits(b)) and torch.equal(a.groups, p.groups)


def test_side_stream_and_graph_replay():
    from cor_amd import ops
    C, Ng, Bq, kin, m = 256, 300, 130, 17, 10
    G16, G32, Q = _unit(Ng, C, 18).to(torch.bfloat16).to(DEV), _unit(Ng, C, 19).to(DEV), _unit(Bq, C, 20).to(DEV)
    s, i = _lists(Bq, kin, -3, 2 * Ng + 3, 21)
    s, i = s.to(DEV), i.to(DEV)
    segs = [(G32, Ng), (G16, 0)]
    eager = ops.expand_queries(Q, segs, s, i, m)
    _same(eager, ref_expand(Q.cpu().numpy(), 1.0, [(_wide(r.cpu()), o) for r, o in segs], s.cpu().numpy(), i.cpu().numpy(), m, 3, True))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = ops.expand_queries(Q, segs, s, i, m)
    side.synchronize()
    assert torch.equal(_bits(on_side), _bits(eager))
    out = torch.zeros((Bq, C), device=DEV)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.expand_queries(Q, segs, s, i, m, out=out)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(eager))

"""CPU-side checks (run under -m "not gpu") of the diffusion re-ranking's host layers: the export of cor_rerank_diffusion, its argument
checks (all made before any HIP call), the Python validation, the no-CPU-path rule, and the NumPy restatement that
tests/test_gpu_diffuse.py compares the kernel with (tests/diffuse_refs.py): on a case small enough to follow by eye, against an independent
dense float64 formulation and its closed form, on the consequences include/cor_amd.h states, and for what the method is for: rows that are
linked to the query through a chain of mutually close rows rise."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests.diffuse_refs import F, diffusion_graph, pw, ref_diffusion

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_diffusion_symbol():
    from cor_amd import _native
    lib = _native.load()
    hdr = open(os.path.join(ROOT, "include", "cor_amd.h")).read()
    proto = re.search(r"^int\s+cor_rerank_diffusion\s*\(([^)]*)\)\s*;", hdr, flags=re.M | re.S)
    assert proto, "cor_rerank_diffusion is not declared in include/cor_amd.h"
    assert len(proto.group(1).split(",")) == 21 == len(_native.SIGNATURES["cor_rerank_diffusion"])
    assert hasattr(lib, "cor_rerank_diffusion") and lib.cor_rerank_diffusion.restype is _native._i
    sig = _native.SIGNATURES["cor_rerank_diffusion"]
    assert sig[14] is _native._f and all(sig[n] is _native._i for n in (5, 8, 9, 10, 11, 12, 13, 15, 16))   # alpha; the integers
    for name, value in (("NMAX", 256), ("KDMAX", 32), ("SEGMAX", 16)):
        assert re.search(rf"^#define\s+COR_DIFFUSE_{name}\s+{value}\b", hdr, flags=re.M) and getattr(_native, f"DIFFUSE_{name}") == value


def test_diffusion_argument_errors_need_no_gpu():
    """Every argument check comes before any HIP call, so each error comes back on a machine without a device."""
    from cor_amd import _native
    lib = _native.load()
    E, N = _native.EINVAL, _native.ENOSUPPORT
    buf = torch.zeros(64, dtype=torch.int64)
    p = buf.data_ptr()

    def call(rows=(p,), scale=(None,), offs=(0,), ns=(10,), dts=(_native.F32,), nseg=None, arrays=True, scale_array=True, scores=p, idx=p,
             Bq=1, kin=8, C=64, kd=8, kq=8, gamma=3, alpha=0.9, iters=20, k=4, out_s=p, out_i=p, out_p=None):
        n = len(rows) if nseg is None else nseg
        a = (ctypes.c_void_p * max(len(rows), 1))(*rows)
        b = (ctypes.c_void_p * max(len(rows), 1))(*scale) if scale_array else None
        c = (ctypes.c_longlong * max(len(rows), 1))(*offs)
        d = (ctypes.c_int * max(len(rows), 1))(*ns)
        e = (ctypes.c_int * max(len(rows), 1))(*dts)
        if not arrays:
            a = c = d = e = None
        return lib.cor_rerank_diffusion(a, b, c, d, e, n, scores, idx, Bq, kin, C, kd, kq, gamma, alpha, iters, k, out_s, out_i, out_p, None)

    # COR_EINVAL
    assert call(scores=None) == E and call(idx=None) == E and call(out_s=None) == E and call(out_i=None) == E and call(arrays=False) == E
    assert call(Bq=-1) == E and call(kin=0) == E and call(k=0) == E and call(k=-3) == E and call(nseg=-1) == E and call(C=0) == E
    assert call(kd=0) == E and call(kq=0) == E and call(gamma=0) == E and call(iters=0) == E and call(kd=-1) == E and call(iters=-5) == E
    assert call(ns=(-1,)) == E and call(rows=(None,)) == E
    assert call(dts=(_native.I8,)) == E and call(dts=(_native.I8,), scale_array=False) == E      # an int8 segment with rows needs its scales
    assert call(alpha=float("nan")) == E and call(alpha=-0.01) == E and call(alpha=1.0) == E and call(alpha=1.5) == E and call(alpha=float("inf")) == E
    # COR_ENOSUPPORT
    assert call(kin=257) == N and call(kd=33) == N and call(gamma=5) == N and call(iters=65) == N and call(k=257) == N
    assert call(C=272) == N and call(C=24) == N and call(C=8) == N
    assert call(dts=(3,)) == N and call(dts=(5,)) == N and call(dts=(-1,)) == N                  # x3 split rows are no gallery dtype
    sixteen = dict(rows=(p,) * 16, scale=(None,) * 16, offs=tuple(range(0, 160, 10)), ns=(10,) * 16, dts=(_native.BF16,) * 16)
    seventeen = dict(rows=(p,) * 17, scale=(None,) * 17, offs=tuple(range(0, 170, 10)), ns=(10,) * 17, dts=(_native.F32,) * 17)
    assert call(**seventeen) == N
    # legal without a device: no queries; with them no segments at all is legal too (decided by the same checks)
    assert call(Bq=0) == 0 and call(Bq=0, **sixteen) == 0 and call(Bq=0, rows=(), scale=(), offs=(), ns=(), dts=(), arrays=False) == 0
    assert call(Bq=0, rows=(None,), ns=(0,)) == 0 and call(Bq=0, rows=(None,), ns=(0,), dts=(_native.I8,), scale_array=False) == 0
    assert call(Bq=0, dts=(_native.I8,), scale=(p,)) == 0 and call(Bq=0, dts=(_native.F16,), scale_array=False) == 0
    assert call(Bq=0, out_p=p) == 0 and call(Bq=0, kin=256, k=256, C=256, kd=32, kq=2 ** 31 - 1, gamma=4, alpha=0.0, iters=64) == 0
    assert call(Bq=0, kin=1, k=1, C=16, kd=1, kq=1, gamma=1, alpha=0.99, iters=1) == 0
    mixed = dict(rows=(p,) * 4, scale=(None, None, None, p), offs=(0, 10, 20, 30), ns=(10,) * 4,
                 dts=(_native.F32, _native.BF16, _native.F16, _native.I8))
    assert call(Bq=0, **mixed) == 0


def _cpu_shard(rows, offset=0):
    """A GalleryShard lives in GPU memory and its constructor says so; the methods under test only read rows and offset."""
    from cor_amd.retrieval import GalleryShard
    sh = GalleryShard.__new__(GalleryShard)
    sh.rows, sh.offset, sh.labels, sh.groups = rows, offset, None, None
    return sh


def _cpu_quantized(rows, scales, offset=0):
    from cor_amd.retrieval import QuantizedGallery
    sh = QuantizedGallery.__new__(QuantizedGallery)
    sh.rows, sh.scales, sh.offset, sh.labels, sh.groups = rows, scales, offset, None, None
    return sh


def test_diffusion_validation_and_no_cpu_path():
    from cor_amd import ops
    from cor_amd.retrieval import GallerySet, QuantizedShard
    G = torch.zeros((5, 16))
    Gq, sc = torch.zeros((5, 16), dtype=torch.int8), torch.ones(5)
    s, i = torch.ones((2, 6)), torch.zeros((2, 6), dtype=torch.int64)
    gs = GallerySet()
    gs._segments = [_cpu_shard(G, 0), _cpu_shard(G[:0], 5), _cpu_quantized(Gq, sc, 20)]   # (add() is not under test)
    for call in (lambda: ops.rerank_diffusion([(G, 0)], s, i, 3),
                 lambda: ops.rerank_diffusion([(G.half(), 0), (Gq, sc, 9)], s, i, 6, kd=32, kq=1, gamma=4, alpha=0.0, iters=64, return_pos=True),
                 lambda: ops.rerank_diffusion([], s, i, 1, kd=1, kq=10 ** 12, gamma=1, alpha=0.99, iters=1),
                 lambda: _cpu_shard(G).diffuse(s, i),
                 lambda: _cpu_shard(G, 100).diffuse(s, i, k=2, kd=4, kq=3, gamma=2, alpha=0.5, iters=5, return_pos=True),
                 lambda: _cpu_quantized(Gq, sc).diffuse(s, i, k=1),
                 lambda: gs.diffuse(s, i),
                 lambda: GallerySet().diffuse(s, i, k=4)):
        with pytest.raises(RuntimeError):                              # valid arguments, CPU tensors: there is no CPU path
            call()
    assert not hasattr(QuantizedShard, "diffuse")                      # the search-only class does not get the method
    bad = [dict(k=0), dict(k=257), dict(k=-1), dict(kd=0), dict(kd=33), dict(kq=0), dict(kq=-1), dict(gamma=0), dict(gamma=5), dict(iters=0),
           dict(iters=65), dict(alpha=-0.1), dict(alpha=1.0), dict(alpha=1.5), dict(alpha=float("nan")), dict(alpha=float("inf")),
           dict(segments=[(G[:1], n) for n in range(17)]),             # 17 segments
           dict(segments=[(G, 0), (G, 3)]),                            # overlapping id ranges
           dict(segments=[(G, 0), (torch.zeros((5, 32)), 10)]),        # two widths
           dict(segments=[(G.double(), 0)]), dict(segments=[(G[0], 0)]), dict(segments=[(torch.zeros((5, 24)), 0)]),
           dict(segments=[(torch.zeros((5, 272)), 0)]), dict(segments=[(Gq, 0)]), dict(segments=[(G, sc, 0)]),
           dict(segments=[(Gq, sc[:4], 0)]), dict(segments=[(Gq, sc.double(), 0)]), dict(segments=[(G,)]), dict(segments=[(G, sc, sc, 0)]),
           dict(scores=s.double()), dict(scores=s[0]), dict(scores=s[:, :0]), dict(idx=i.to(torch.int32)), dict(idx=i[:1])]
    for kw in bad:
        args = dict(segments=[(G, 0)], scores=s, idx=i, k=3)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.rerank_diffusion(**args)
    with pytest.raises(ValueError, match="17 segments"):
        ops.rerank_diffusion([(G[:1], n) for n in range(17)], s, i, 3)
    with pytest.raises(ValueError):
        _cpu_shard(G).diffuse(s, i[0])


class _Never:
    """A gallery that must not be touched."""

    def search(self, *a, **kw):
        raise AssertionError("searched before the arguments were validated")

    diffuse = search


def test_diffused_search_validates_first_and_composes():
    from cor_amd import retrieval
    for kw in (dict(k=0, k_coarse=5), dict(k=6, k_coarse=5), dict(k=10, k_coarse=257), dict(k=-1, k_coarse=-1), dict(k=2, k_coarse=5, kd=0),
               dict(k=2, k_coarse=5, kd=33), dict(k=2, k_coarse=5, kq=0), dict(k=2, k_coarse=5, gamma=5), dict(k=2, k_coarse=5, gamma=0),
               dict(k=2, k_coarse=5, iters=0), dict(k=2, k_coarse=5, iters=65), dict(k=2, k_coarse=5, alpha=1.0),
               dict(k=2, k_coarse=5, alpha=-0.5), dict(k=2, k_coarse=5, alpha=float("nan"))):
        with pytest.raises(ValueError):
            retrieval.diffused_search(None, _Never(), **kw)
    calls = []

    class Gallery:
        def search(self, q, k, **kw):
            calls.append(("search", q, k, kw))
            return "s", "i"

        def diffuse(self, s, i, **kw):
            calls.append(("diffuse", s, i, kw))
            return "ds", "di"

    assert retrieval.diffused_search("q", Gallery(), 10, 50, kd=4, alpha=0.8, distinct=True) == ("ds", "di")
    assert calls == [("search", "q", 50, dict(distinct=True)),
                     ("diffuse", "s", "i", dict(k=10, kd=4, kq=None, gamma=3, alpha=0.8, iters=20))]


def _bits(x):
    return np.asarray(x, dtype=F).view(np.int32)


def test_a_case_to_follow_by_eye():
    """Four rows with exact similarities: rows 10 and 11 identical (sim 1), row 12 halfway between them and row 13 (sim 0.5 to each),
    row 13 unrelated to 10 and 11. gamma = 1, so a = sim; alpha = 0.5 and dyadic scores, so every product and sum below is exact.
         a = [[0, 1, .5, 0], [1, 0, .5, 0], [.5, .5, 0, .5], [0, 0, .5, 0]]
    kd = 1: N = [1], [0], [0] (a three-way tie at .5: the lowest position), [2]; mutual: only 0 - 1. d = 1, 1, 0, 0; S(0,1) = 1.
        iters = 1: f = (.5 * .25) + .375, (.5 * .75) + .125, 0 + .25, 0 + .0625 = .5, .5, .25, .0625: a tie, the smaller id first
        iters = 2: f = (.5 * .5) + .375, (.5 * .5) + .125, .25, .0625 = .625, .375, .25, .0625
    kd = 3: every a > 0 is an edge; d = 1.5, 1.5, 1.5, .5."""
    e = np.eye(16, dtype=F)
    X = np.stack([e[0], e[0], (e[0] + e[1]) * F(0.5), e[1]])
    segs = [(X, 10)]
    idx = np.array([[10, 11, 12, 13]], np.int64)
    sc = np.array([[0.75, 0.25, 0.5, 0.125]], F)
    a, N, M = diffusion_graph(X, [0, 1, 2, 3], 1, 1)
    assert a.tolist() == [[0, 1, .5, 0], [1, 0, .5, 0], [.5, .5, 0, .5], [0, 0, .5, 0]]
    assert N == [[1], [0], [0], [2]] and M == [[1], [0], [], []]
    s, i, p = ref_diffusion(sc, idx, segs, 4, kd=1, gamma=1, alpha=0.5, iters=1)
    assert s[0].tolist() == [.5, .5, .25, .0625] and i[0].tolist() == [10, 11, 12, 13] and p[0].tolist() == [0, 1, 2, 3]
    s, i, p = ref_diffusion(sc, idx[:, ::-1].copy(), segs, 4, kd=1, gamma=1, alpha=0.5, iters=1)     # the list reversed: 13, 12, 11, 10
    # ties in the neighbour selection go by POSITION: row 12 (now at position 1) names 13 (position 0), so 13 - 12 and 11 - 10 are mutual;
    # 10 and 11 (scores .125 and .5 now): f = (.5 * .5) + .0625 and (.5 * .125) + .25, a tie that the smaller id wins from the later position
    assert diffusion_graph(X, [3, 2, 1, 0], 1, 1)[1:] == ([[1], [0], [3], [2]], [[1], [0], [3], [2]])
    assert sorted(i[0, :2].tolist()) == [12, 13] and i[0, 2:].tolist() == [10, 11] and p[0, 2:].tolist() == [3, 2] and s[0, 2:].tolist() == [.3125, .3125]
    s, i, p = ref_diffusion(sc, idx, segs, 4, kd=1, gamma=1, alpha=0.5, iters=2)
    assert s[0].tolist() == [.625, .375, .25, .0625] and i[0].tolist() == [10, 11, 12, 13]
    a, N, M = diffusion_graph(X, [0, 1, 2, 3], 3, 1)
    assert N == [[1, 2], [0, 2], [0, 1, 3], [2]] and M == N
    s, i, p = ref_diffusion(sc, idx, segs, 4, kd=3, gamma=1, alpha=0.5, iters=1)
    ra, rb = 1 / np.sqrt(1.5), 1 / np.sqrt(0.5)                       # float64, written out: f = .5 * (S y) + .5 * y
    want = [.5 * (1 * ra * ra * .25 + .5 * ra * ra * .5) + .375, .5 * (1 * ra * ra * .75 + .5 * ra * ra * .5) + .125,
            .5 * (.5 * ra * ra * .75 + .5 * ra * ra * .25 + .5 * ra * rb * .125) + .25, .5 * (.5 * rb * ra * .5) + .0625]
    assert i[0].tolist() == [10, 11, 12, 13] and np.abs(s[0].astype(np.float64) - want).max() <= 8 * 2.0 ** -24   # a handful of roundings of values < 1
    # kq = 1: only the first present entry injects mass; 12 and 13 get theirs through the graph alone
    s, i, p = ref_diffusion(sc, idx, segs, 4, kd=3, kq=1, gamma=1, alpha=0.5, iters=1)
    assert s[0, 0] == F(.375) and i[0].tolist() == [10, 11, 12, 13] and s[0, 3] == 0 and s[0, 1] > s[0, 2] > 0


def _unit(x):
    return (x / np.linalg.norm(x, axis=-1, keepdims=True)).astype(F)


def chained_lists(seed, queries=40, C=64):
    """The purpose fixture. Per query, numpy.random.default_rng(seed) drawn in this order: base = unit(N(0, I)); a chain of 24 positives,
    cur = unit(cur + 0.28 * unit(N(0, I))) starting from base (the far end of the chain is far from the query, its links are close to
    each other); 200 distractors unit(0.75 * base + unit(N(0, I))). The 128 best by X @ base (fp32, ties by index) form the list.
    -> [(X f32 [224,64] (rows 0 .. 23 the positives), scores f32 [128], idx i64 [128])]"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(queries):
        base = _unit(rng.standard_normal(C))
        cur, pos = base, []
        for _ in range(24):
            cur = _unit(cur + F(0.28) * _unit(rng.standard_normal(C)))
            pos.append(cur)
        dis = _unit(F(0.75) * base + _unit(rng.standard_normal((200, C))))
        X = np.concatenate([np.stack(pos), dis]).astype(F)
        s = (X @ base).astype(F)
        order = np.lexsort((np.arange(224), -s))[:128]
        out.append((X, s[order], order.astype(np.int64)))
    return out


def average_precision(ids, positives=24):
    hits, total = 0, 0.0
    for rank, i in enumerate(ids):
        if 0 <= i < positives:
            hits += 1
            total += hits / (rank + 1)
    return total / max(hits, 1)


def _f64_diffusion(X, scores, kd, gamma, alpha, iters):
    """An independent formulation for one query whose entries are all present, in float64 with dense matrices: A = max(X X^T, 0) ** gamma
    with a zero diagonal, the kd-NN indicator K by a stable argsort of every row, W = A where K and K^T, S = D^-1/2 W D^-1/2, y = max(s, 0)
    ** gamma, f <- alpha S f + (1 - alpha) y. -> (f after `iters` steps, the fixed point (1 - alpha) (I - alpha S)^-1 y, y, S, the least
    similarity on an edge)."""
    X64 = X.astype(np.float64)
    n = X64.shape[0]
    sim = X64 @ X64.T
    A = np.maximum(sim, 0.0) ** gamma
    np.fill_diagonal(A, 0.0)
    K = np.zeros((n, n), bool)
    for p in range(n):
        best = np.argsort(-A[p], kind="stable")[:kd]
        K[p, best[A[p, best] > 0]] = True
    W = np.where(K & K.T, A, 0.0)
    d = W.sum(1)
    r = np.where(d > 0, 1.0 / np.sqrt(np.where(d > 0, d, 1.0)), 0.0)
    S = W * r[:, None] * r[None, :]
    y = np.maximum(scores.astype(np.float64), 0.0) ** gamma
    f = y.copy()
    for _ in range(iters):
        f = alpha * (S @ f) + (1.0 - alpha) * y
    fixed = (1.0 - alpha) * np.linalg.solve(np.eye(n) - alpha * S, y)
    return f, fixed, y, S, sim[W > 0].min()


@pytest.mark.parametrize("kd,gamma,alpha,iters", [(8, 3, 0.9, 20), (8, 3, 0.9, 64), (4, 1, 0.5, 40), (16, 2, 0.99, 64), (32, 4, 0.7, 30)])
def test_restatement_against_dense_float64_and_the_closed_form(kd, gamma, alpha, iters):
    """ref_diffusion against dense float64 on three lists of the purpose fixture (n = 128, C = 64). The graph must be the same graph.
    The bounds are derived, not tuned (u = 2^-24, rows of unit norm, all terms non-negative):
      rounding. A chain is off by at most C u absolutely, so an edge's a = sim ** gamma by gamma (C / sim_min + 1) u relatively; d adds kd u,
        r = d ** -1/2 halves that and adds 2 u, S = a (r r') adds 2 u: every fp32 S entry is within delta = 2 gamma (C / sim_min + 1) u +
        (kd + 6) u of the float64 one, relatively, hence ||S32 - S||_2 <= delta ||S||_2 <= delta (S is a normalised adjacency: ||S||_2 <= 1).
        A step's fma chain of <= kd non-negative terms, two products and a sum add (kd + 3) u relatively. With ||f||_2 <= ||y||_2 for every
        iterate (induction over f <- alpha S f + (1 - alpha) y), the difference D of the two iterations obeys
        ||D'|| <= alpha (1 + delta) ||D|| + (alpha delta + (kd + 3) u) (1 + delta) ||y||, so ||D|| <= (alpha delta + (kd + 3) u) (1 + delta) ||y|| /
        (1 - alpha (1 + delta)) at every step. y itself (gamma - 1 products) starts D at gamma u ||y||, below that figure.
      limit. f(t) - f* = (alpha S)^t (y - f*), so ||f(t) - f*||_2 <= alpha^t ||y - f*||_2."""
    u = 2.0 ** -24
    for X, s, i in chained_lists(5, queries=3):
        rows = X[i]
        rs, ri, rp = ref_diffusion(s[None], np.arange(128, dtype=np.int64)[None], [(rows, 0)], 128, kd=kd, gamma=gamma, alpha=alpha, iters=iters)
        f32 = np.empty(128)
        f32[rp[0]] = rs[0]
        f64, fixed, y, S, sim_min = _f64_diffusion(rows, s, kd, gamma, alpha, iters)
        _, _, M = diffusion_graph(rows, list(range(128)), kd, gamma)
        assert [sorted(m) for m in M] == [np.flatnonzero(S[p]).tolist() for p in range(128)], "the mutual graphs differ"
        delta = 2 * gamma * (64 / sim_min + 1) * u + (kd + 6) * u
        assert alpha * (1 + delta) < 1
        rounding = (alpha * delta + (kd + 3) * u) * (1 + delta) * np.linalg.norm(y) / (1 - alpha * (1 + delta))
        limit = alpha ** iters * np.linalg.norm(y - fixed)
        print(f"kd={kd} gamma={gamma} alpha={alpha} iters={iters}: |f32 - f64| {np.linalg.norm(f32 - f64):.3e} <= {rounding:.3e}; "
              f"|f64 - f*| {np.linalg.norm(f64 - fixed):.3e} <= {limit:.3e}")
        assert np.linalg.norm(f32 - f64) <= rounding
        assert np.linalg.norm(f64 - fixed) <= limit * (1 + 1e-9) + 1e-13
        assert np.linalg.norm(f32 - fixed) <= limit + rounding


def test_consequences_of_the_definition():
    """What include/cor_amd.h lists under Consequences, and the edge cases of presence, on the restatement."""
    rng = np.random.default_rng(3)
    X = _unit(rng.standard_normal((60, 32)))
    X[50:] = -X[40:50]                                                # opposite rows
    segs = [(X, 100)]
    q = _unit(X[:3].sum(0))
    s = np.sort((X[:40] @ q).astype(F))[::-1].copy()[None]
    s = np.abs(s) + F(0.01)                                           # a searched list with positive scores, descending
    s = np.sort(s)[:, ::-1].copy()
    idx = (100 + rng.permutation(40)[None]).astype(np.int64)
    # alpha = 0 returns y exactly; with gamma = 1 and kq >= n the list comes back unchanged
    rs, ri, rp = ref_diffusion(s, idx, segs, 40, kd=8, gamma=1, alpha=0.0, iters=7)
    assert np.array_equal(_bits(rs), _bits(s)) and np.array_equal(ri, idx) and rp[0].tolist() == list(range(40))
    rs, ri, rp = ref_diffusion(s, idx, segs, 40, kd=8, gamma=3, alpha=0.0, iters=2, kq=5)
    assert np.array_equal(_bits(rs[0, :5]), _bits(pw(s[0, :5], 3))) and (rs[0, 5:] == 0).all()
    assert ri[0, 5:].tolist() == sorted(idx[0, 5:].tolist())          # f = 0 for all of them: by id
    # kd >= n - 1: M(p) is every p' with a > 0
    a, N, M = diffusion_graph(X, list(range(40)), 39, 2)
    assert all(sorted(M[p]) == [t for t in range(40) if t != p and a[p, t] > 0] for p in range(40)) and N == M
    a32, _, M32 = diffusion_graph(X, list(range(40)), 32, 2)
    assert np.array_equal(_bits(a), _bits(a.T)) and all(len(m) <= 32 for m in M32)   # bitwise symmetric
    # rows without a positive similarity to any other row: isolated, f = (alpha * 0) + (1 - alpha) y after every step
    e = np.eye(16, dtype=F)
    Y = np.stack([e[0], -e[0], e[1], e[2], (e[1] + e[2]) * F(0.5)])
    ys = np.array([[0.9, 0.8, 0.7, 0.6, 0.5]], F)
    yi = np.arange(5, dtype=np.int64)[None]
    for iters in (1, 2, 9):
        rs, ri, rp = ref_diffusion(ys, yi, [(Y, 0)], 5, kd=4, gamma=2, alpha=0.9, iters=iters)
        f = dict(zip(ri[0].tolist(), rs[0]))
        keep = (F(1) - F(0.9)) * pw(ys[0], 2)
        assert f[0] == (F(0.9) * F(0)) + keep[0] and f[1] == (F(0.9) * F(0)) + keep[1] and f[4] > keep[4]
    # n = 1, no present entry, no segment, k > n, a missing entry's NaN score, repeated ids
    rs, ri, rp = ref_diffusion(ys[:, :1], yi[:, :1], [(Y, 0)], 3, kd=4, gamma=1, alpha=0.5, iters=3)
    assert rs[0].tolist() == [(F(0.5) * F(0)) + (F(0.5) * F(0.9)), -np.inf, -np.inf] and ri[0].tolist() == [0, -1, -1] and rp[0].tolist() == [0, -1, -1]
    assert ref_diffusion(ys, yi + 7, [(Y, 0)], 2)[1].tolist() == [[-1, -1]] and ref_diffusion(ys, yi, [], 2)[2].tolist() == [[-1, -1]]
    hs = np.array([[np.nan, 0.9, np.nan, 0.7, 0.6, np.nan]], F)
    hi = np.array([[-1, 2, 2 ** 40, 3, 4, 99]], np.int64)
    rs, ri, rp = ref_diffusion(hs, hi, [(Y, 0)], 6, kd=2, gamma=1, alpha=0.5, iters=4)
    ws, wi, wp = ref_diffusion(hs[:, [1, 3, 4]], hi[:, [1, 3, 4]], [(Y, 0)], 6, kd=2, gamma=1, alpha=0.5, iters=4)
    assert np.array_equal(_bits(rs), _bits(ws)) and np.array_equal(ri, wi) and rp[0, :3].tolist() == [[1, 3, 4][t] for t in wp[0, :3]]
    rep = np.array([[2, 2, 4, 2]], np.int64)                          # a repeated id: entries of their own, neighbours of each other (sim 1)
    rs, ri, rp = ref_diffusion(np.array([[0.5, 0.5, 0.5, 0.5]], F), rep, [(Y, 0)], 4, kd=1, gamma=1, alpha=0.5, iters=1)
    assert ri[0].tolist() == [2, 2, 2, 4] and rp[0].tolist() == [0, 1, 3, 2]      # 0 - 1 mutual (.5), 3 names 0 but 0 names 1: .25; 4: .25
    assert rs[0].tolist() == [.5, .5, .25, .25]
    # segmentation does not matter
    two = [(X[30:], 130), (np.zeros((0, 32), F), 500), (X[:30], 100)]
    one, cut = ref_diffusion(s, idx, segs, 40), ref_diffusion(s, idx, two, 40)
    assert all(np.array_equal(_bits(x) if x.dtype == F else x, _bits(y) if y.dtype == F else y) for x, y in zip(one, cut))


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_diffusion_lifts_the_far_end_of_a_chain(seed):
    """What the method is for, on the restatement alone (the GPU kernel inherits it through bitwise equality): chained_lists, 40 queries per
    seed, kd = 8, gamma = 3, alpha = 0.9, iters = 20, kq = 128. Average precision over the positives inside the 128-entry list, mean over
    the queries, input order -> after diffusion, as this restatement gives them: seed 0 0.7276 -> 0.9150, seed 1 0.7051 -> 0.9093,
    seed 2 0.6999 -> 0.9038, seed 3 0.7119 -> 0.9145; better for 40 of 40 queries of every seed. The assertion is the issue's: strictly
    better for EVERY query."""
    before, after = [], []
    for X, s, i in chained_lists(seed):
        rs, ri, rp = ref_diffusion(s[None], i[None], [(X, 0)], 128, kd=8, kq=128, gamma=3, alpha=0.9, iters=20)
        before.append(average_precision(i))
        after.append(average_precision(ri[0]))
        assert sorted(ri[0].tolist()) == sorted(i.tolist())
    print(f"seed {seed}: mean AP {np.mean(before):.4f} -> {np.mean(after):.4f}, better for {sum(a > b for a, b in zip(after, before))} of 40")
    assert all(a > b for a, b in zip(after, before))

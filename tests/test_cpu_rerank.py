"""CPU-side checks (run under -m "not gpu") of the k-reciprocal re-ranking's host layers: the exports of cor_knn_reciprocal and
cor_rerank_reciprocal, their argument checks (all made before any HIP call), the Python validation including the stale-graph check, the
no-CPU-path rule, and the NumPy restatements of the two definitions that tests/test_gpu_rerank.py compares the kernels with, themselves
checked against Python sets and float64, and for what the method is for: Recall@1 on a clustered gallery with hub rows."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def ref_prune(segs):
    """The definition of cor_knn_reciprocal (include/cor_amd.h) restated: segs [(nbr i64 [n,k1], offset)] -> [pruned i64 [n,k1]].
    out[g, j] = h = nbr[g, j] if h lies in some segment and offset + g occurs in h's list, else -1. Never calls the code under test."""
    outs = []
    for nbr, off in segs:
        n = nbr.shape[0]
        out = np.full_like(nbr, -1)
        for lo in range(0, n, 128):
            H = nbr[lo:lo + 128]
            gid = (off + np.arange(lo, lo + H.shape[0], dtype=np.int64))[:, None, None]
            for nbr2, off2 in segs:
                if nbr2.shape[0] == 0:
                    continue
                inside = (H >= off2) & (H < off2 + nbr2.shape[0])
                back = (nbr2[np.where(inside, H - off2, 0)] == gid).any(-1)
                out[lo:lo + 128] = np.where(inside & back, H, out[lo:lo + 128])
        outs.append(out)
    return outs


def ref_rerank(scores, idx, segs, k1, lam, k):
    """The definition of cor_rerank_reciprocal (include/cor_amd.h) restated with elementwise np.float32 operations in the stated order.
    scores f32 / idx i64 [Bq,kin], segs [(rnbr i64 [n,kg], kth f32 [n], offset)] -> (scores f32 [Bq,k], idx i64 [Bq,k], pos i32 [Bq,k]).
    Never calls the code under test."""
    Bq, kin = idx.shape
    kg = segs[0][0].shape[1] if segs else 1
    out_s, out_i, out_p = np.full((Bq, k), -np.inf, F), np.full((Bq, k), -1, np.int64), np.full((Bq, k), -1, np.int32)
    for b in range(Bq):
        ids = idx[b]
        present, R, KT = np.zeros(kin, bool), np.full((kin, kg), -1, np.int64), np.zeros(kin, F)
        for rnbr, kth, off in segs:
            if rnbr.shape[0] == 0:
                continue
            inside = (ids >= off) & (ids < off + rnbr.shape[0])
            local = (ids - off)[inside]
            R[inside], KT[inside] = rnbr[local], kth[local]
            present |= inside
        s = np.where(present, scores[b], F(0)).astype(F)                # a missing entry's score is never used
        A = ids[:k1][present[:k1] & (s[:k1] >= KT[:k1])]
        valid = R >= 0
        nB = valid.sum(1)
        I = (np.isin(R, A) & valid).sum(1)
        U = len(A) + nB - I
        J = np.zeros(kin, F)
        J[U > 0] = I[U > 0].astype(F) / U[U > 0].astype(F)
        f = (F(lam) * s) + ((F(1) - F(lam)) * J)
        assert f.dtype == F and J.dtype == F
        order = sorted(np.flatnonzero(present).tolist(), key=lambda j: (-float(f[j]), int(ids[j])))[:k]   # -0.0 == 0.0: the id decides
        out_s[b, :len(order)], out_i[b, :len(order)], out_p[b, :len(order)] = f[order], ids[order], order
    return out_s, out_i, out_p


def np_search(Q, G, k, offset=0):
    """Top-k of Q @ G^T in float32 by (score desc, id asc), NumPy only: (scores f32 [Bq,k], idx i64 [Bq,k]); (-inf, -1) past the rows."""
    S = (Q.astype(F) @ G.astype(F).T).astype(F)
    Bq, Ng = S.shape
    s, i = np.full((Bq, k), -np.inf, F), np.full((Bq, k), -1, np.int64)
    for b in range(Bq):
        o = np.lexsort((np.arange(Ng), -S[b]))[:k]
        s[b, :len(o)], i[b, :len(o)] = S[b, o], o + offset
    return s, i


def np_graph(G, k1, offset=0):
    """[(rnbr, kth, offset)] of one segment, NumPy only: the search of every row in G, then ref_prune."""
    s, i = np_search(G, G, k1, offset)
    return [(ref_prune([(i, offset)])[0], s[:, k1 - 1].copy(), offset)]


def _proto_args(hdr, name):
    proto = re.search(r"^int\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr, flags=re.M | re.S)
    assert proto, f"{name} is not declared in include/cor_amd.h"
    return len(proto.group(1).split(","))


def test_library_exports_the_rerank_symbols():
    from cor_amd import _native
    lib = _native.load()
    hdr = open(os.path.join(ROOT, "include", "cor_amd.h")).read()
    assert _proto_args(hdr, "cor_knn_reciprocal") == 8 == len(_native.SIGNATURES["cor_knn_reciprocal"])
    assert _proto_args(hdr, "cor_rerank_reciprocal") == 17 == len(_native.SIGNATURES["cor_rerank_reciprocal"])
    assert hasattr(lib, "cor_knn_reciprocal") and lib.cor_knn_reciprocal.restype is _native._i
    assert hasattr(lib, "cor_rerank_reciprocal") and lib.cor_rerank_reciprocal.restype is _native._i
    assert _native.SIGNATURES["cor_rerank_reciprocal"][11] is _native._f          # lam
    assert re.search(r"^#define\s+COR_RERANK_SEGMAX\s+16\b", hdr, flags=re.M) and _native.RERANK_SEGMAX == 16


def test_rerank_argument_errors_need_no_gpu():
    """Every argument check comes before any HIP call, so each error comes back on a machine without a device."""
    from cor_amd import _native
    lib = _native.load()
    E, N = _native.EINVAL, _native.ENOSUPPORT
    buf = torch.zeros(64, dtype=torch.int64)
    p = buf.data_ptr()

    def call(scores=p, idx=p, rnbr=(p,), kth=(p,), offs=(0,), ns=(10,), nseg=None, arrays=True, Bq=1, kin=8, kg=4, k1=4, lam=0.3, k=4,
             out_s=p, out_i=p, out_p=None):
        n = len(rnbr) if nseg is None else nseg
        a = (ctypes.c_void_p * max(len(rnbr), 1))(*rnbr)
        b = (ctypes.c_void_p * max(len(rnbr), 1))(*kth)
        c = (ctypes.c_longlong * max(len(rnbr), 1))(*offs)
        d = (ctypes.c_int * max(len(rnbr), 1))(*ns)
        if not arrays:
            a = b = c = d = None
        return lib.cor_rerank_reciprocal(scores, idx, a, b, c, d, n, Bq, kin, kg, k1, lam, k, out_s, out_i, out_p, None)

    # COR_EINVAL
    assert call(scores=None) == E and call(idx=None) == E and call(out_s=None) == E and call(out_i=None) == E and call(arrays=False) == E
    assert call(Bq=-1) == E and call(kin=0) == E and call(kg=0) == E and call(k1=0) == E and call(k=0) == E and call(k=-3) == E
    assert call(k1=9) == E and call(kin=300, k1=301) == E                                # k1 > kin
    assert call(nseg=-1) == E and call(ns=(-1,)) == E and call(rnbr=(None,)) == E and call(kth=(None,)) == E
    # COR_ENOSUPPORT
    assert call(kin=4097) == N and call(kin=300, k1=257) == N and call(kg=257) == N and call(k=257) == N
    sixteen = dict(rnbr=(p,) * 16, kth=(p,) * 16, offs=tuple(range(0, 160, 10)), ns=(10,) * 16)
    seventeen = dict(rnbr=(p,) * 17, kth=(p,) * 17, offs=tuple(range(0, 170, 10)), ns=(10,) * 17)
    assert call(**seventeen) == N
    # legal without a device: no queries; with them, no segments at all is legal too (decided by the same checks)
    assert call(Bq=0) == 0 and call(Bq=0, rnbr=(), kth=(), offs=(), ns=(), arrays=False) == 0 and call(Bq=0, **sixteen) == 0
    assert call(Bq=0, rnbr=(None,), kth=(None,), ns=(0,)) == 0 and call(Bq=0, out_p=p) == 0
    assert call(Bq=0, kin=4096, kg=256, k1=256, k=256, lam=1.0) == 0 and call(Bq=0, kin=1, kg=1, k1=1, k=1, lam=0.0) == 0

    def prune(nbr=(p,), offs=(0,), ns=(10,), nseg=None, arrays=True, k1=4, seg=0, out=p):
        n = len(nbr) if nseg is None else nseg
        a = (ctypes.c_void_p * max(len(nbr), 1))(*nbr)
        c = (ctypes.c_longlong * max(len(nbr), 1))(*offs)
        d = (ctypes.c_int * max(len(nbr), 1))(*ns)
        if not arrays:
            a = c = d = None
        return lib.cor_knn_reciprocal(a, c, d, n, k1, seg, out, None)

    assert prune(arrays=False) == E and prune(nseg=0) == E and prune(nseg=-1) == E and prune(k1=0) == E
    assert prune(seg=-1) == E and prune(seg=1) == E and prune(ns=(-1,)) == E and prune(nbr=(None,)) == E and prune(out=None) == E
    assert prune(k1=257) == N and prune(nbr=(p,) * 17, offs=tuple(range(0, 170, 10)), ns=(10,) * 17) == N
    assert prune(ns=(0,)) == 0 and prune(ns=(0,), nbr=(None,), out=None) == 0            # nothing to prune: no launch
    assert prune(nbr=(p, None), offs=(0, 50), ns=(10, 0), seg=1, out=None, k1=256) == 0


def _cpu_shard(rows, offset=0):
    """A GalleryShard lives in GPU memory and its constructor says so; the methods under test only read rows and offset."""
    from cor_amd.retrieval import GalleryShard
    sh = GalleryShard.__new__(GalleryShard)
    sh.rows, sh.offset, sh.labels, sh.groups = rows, offset, None, None
    return sh


def _cpu_graph(n=5, kg=4, offset=0):
    from cor_amd.retrieval import NeighbourGraph
    return NeighbourGraph(kg, [offset], [n], [torch.full((n, kg), -1, dtype=torch.int64)], [torch.zeros(n)])


def test_rerank_validation_and_no_cpu_path():
    from cor_amd import ops
    from cor_amd.retrieval import GallerySet, NeighbourGraph
    G = torch.zeros((5, 16))
    rnbr, kth = torch.full((5, 4), -1, dtype=torch.int64), torch.zeros(5)
    s, i = torch.ones((2, 6)), torch.zeros((2, 6), dtype=torch.int64)
    empty = NeighbourGraph(4, [], [], [], [])
    for call in (lambda: ops.rerank_reciprocal(s, i, [(rnbr, kth, 0)], 4, 0.3, 3),
                 lambda: ops.rerank_reciprocal(s, i, [], 1, 1.0, 6, return_pos=True),
                 lambda: ops.knn_reciprocal([(rnbr, 0)], 0),
                 lambda: ops.knn_reciprocal([(rnbr, 0), (rnbr[:2], 9)], 1),
                 lambda: _cpu_shard(G).rerank(s, i, _cpu_graph()),
                 lambda: _cpu_shard(G, 100).rerank(s, i, _cpu_graph(offset=100), k1=2, lam=0.5, k=1),
                 lambda: GallerySet().rerank(s, i, empty)):
        with pytest.raises(RuntimeError):                              # valid arguments, CPU tensors: there is no CPU path
            call()
    bad = [dict(k1=0), dict(k1=7), dict(k1=-1),                        # k1 > kin
           dict(k=0), dict(k=257), dict(lam=float("nan")), dict(lam=float("inf")), dict(lam=-float("inf")),
           dict(segments=[(rnbr[:1], kth[:1], n) for n in range(17)]),  # 17 segments
           dict(segments=[(rnbr, kth, 0), (rnbr, kth, 3)]),             # overlapping id ranges
           dict(segments=[(rnbr, kth, 0), (rnbr[:, :2], kth, 10)]),     # two widths
           dict(segments=[(rnbr.to(torch.int32), kth, 0)]), dict(segments=[(rnbr[0], kth, 0)]), dict(segments=[(rnbr, kth[:4], 0)]),
           dict(segments=[(rnbr, kth.double(), 0)]), dict(segments=[(torch.zeros((5, 257), dtype=torch.int64), kth, 0)]),
           dict(scores=s.double()), dict(scores=s[0]), dict(scores=s[:, :0]), dict(idx=i.to(torch.int32)), dict(idx=i[:1])]
    for kw in bad:
        args = dict(scores=s, idx=i, segments=[(rnbr, kth, 0)], k1=4, lam=0.3, k=3)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.rerank_reciprocal(**args)
    with pytest.raises(ValueError, match="17 segments"):
        ops.rerank_reciprocal(s, i, [(rnbr[:1], kth[:1], n) for n in range(17)], 4, 0.3, 3)
    for kw in (dict(segments=[]), dict(seg=1), dict(seg=-1), dict(segments=[(rnbr, 0), (rnbr, 4)]), dict(segments=[(rnbr, 0), (rnbr[:, :2], 9)]),
               dict(segments=[(rnbr.to(torch.int32), 0)]), dict(segments=[(torch.zeros((5, 257), dtype=torch.int64), 0)]),
               dict(out=rnbr), dict(out=torch.zeros((5, 3), dtype=torch.int64)), dict(segments=[(rnbr[:1], n) for n in range(17)])):
        args = dict(segments=[(rnbr, 0)], seg=0)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.knn_reciprocal(**args)


class _Never:
    """A gallery that must not be touched."""

    def search(self, *a, **kw):
        raise AssertionError("searched before the arguments were validated")

    rerank = search


def test_graph_and_search_arguments_validate_first():
    from cor_amd import retrieval
    from cor_amd.retrieval import GallerySet
    for kw in (dict(k=0, k_coarse=5), dict(k=6, k_coarse=5), dict(k=10, k_coarse=257), dict(k=-1, k_coarse=-1)):
        with pytest.raises(ValueError):
            retrieval.reranked_search(None, _Never(), None, **kw)
    sh = _cpu_shard(torch.zeros((5, 16)))
    for kw in (dict(k1=0), dict(k1=257), dict(k1=3, batch=0)):
        with pytest.raises(ValueError):
            sh.neighbour_graph(neighbours=_Never(), **kw)
        with pytest.raises(ValueError):
            GallerySet().neighbour_graph(**kw)


def test_stale_graph_is_refused():
    """A graph names the offsets and lengths of the segments it was built from; rerank refuses any other gallery before anything runs."""
    G = torch.zeros((5, 16))
    s, i = torch.ones((2, 6)), torch.zeros((2, 6), dtype=torch.int64)
    for shard, graph in ((_cpu_shard(G), _cpu_graph(n=4)), (_cpu_shard(G, 7), _cpu_graph()), (_cpu_shard(G[:0]), _cpu_graph()),
                         (_cpu_shard(G), _cpu_graph(n=0))):
        with pytest.raises(ValueError, match="build a new graph"):
            shard.rerank(s, i, graph)
    from cor_amd.retrieval import GallerySet, NeighbourGraph
    gs = GallerySet()
    gs._segments = [_cpu_shard(G, 0), _cpu_shard(G[:0], 5), _cpu_shard(G[:3], 20)]     # (add() is not under test; an empty segment is not live)
    two = NeighbourGraph(4, [0, 20], [5, 3], [torch.full((5, 4), -1, dtype=torch.int64), torch.full((3, 4), -1, dtype=torch.int64)],
                         [torch.zeros(5), torch.zeros(3)])
    with pytest.raises(RuntimeError):                                  # the right graph passes the check and reaches the (GPU-only) op
        gs.rerank(s, i, two)
    gs._segments.append(_cpu_shard(G[:2], 30))                         # what add() does
    with pytest.raises(ValueError, match="build a new graph"):
        gs.rerank(s, i, two)
    gs._segments = gs._segments[1:3]                                   # what drop(0) and drop(30) do
    with pytest.raises(ValueError, match="build a new graph"):
        gs.rerank(s, i, two)


def test_reranked_search_composes_search_and_rerank():
    from cor_amd import retrieval
    calls = []

    class Gallery:
        def search(self, q, k, **kw):
            calls.append(("search", q, k, kw))
            return "s", "i"

        def rerank(self, s, i, graph, **kw):
            calls.append(("rerank", s, i, graph, kw))
            return "rs", "ri"

    assert retrieval.reranked_search("q", Gallery(), "g", 10, 50, k1=20, lam=0.4, distinct=True) == ("rs", "ri")
    assert calls == [("search", "q", 50, dict(distinct=True)), ("rerank", "s", "i", "g", dict(k1=20, lam=0.4, k=10))]


def _clustered(seed=3, clusters=60, per=5, C=64, hubs=12, spread=0.55, Bq=120):
    """A seeded gallery of tight clusters plus hub rows, and queries with one relevant cluster each. A hub is the normalised sum of three
    queries, so it scores high against each of them though it belongs to no cluster. -> (G f32 [n,C], Q f32 [Bq,C], label of every row
    (-1: hub), label of every query)."""
    rng = np.random.default_rng(seed)
    unit = lambda x: (x / np.linalg.norm(x, axis=-1, keepdims=True)).astype(F)
    centres = unit(rng.standard_normal((clusters, C)))
    rows = unit(np.repeat(centres, per, 0) + spread * rng.standard_normal((clusters * per, C)) / np.sqrt(C))
    qlab = rng.integers(0, clusters, Bq)
    Q = unit(centres[qlab] + 2.2 * spread * rng.standard_normal((Bq, C)) / np.sqrt(C))
    hub = unit(Q[rng.integers(0, Bq, (hubs, 3))].sum(1))
    G = np.concatenate([rows, hub])
    glab = np.concatenate([np.repeat(np.arange(clusters), per), np.full(hubs, -1)])
    perm = rng.permutation(len(G))
    return G[perm], Q, glab[perm], qlab


def test_restatement_against_sets_and_float64():
    """ref_rerank against Python sets and float64 on the clustered gallery: I and U are exact integers, so J = fl(I / U) is within 1 ulp
    (half an ulp, in fact) of the float64 quotient, and the order agrees wherever the float64 values of f differ by more than 1e-6
    (three roundings of values below 2 stay under 3 * 2^-24 * 2 < 4e-7)."""
    G, Q, _, _ = _clustered()
    k1, kin, lam = 6, 30, 0.3
    graph = np_graph(G, k1, offset=1000)
    rnbr, kth, off = graph[0]
    s, i = np_search(Q, G, kin, offset=1000)
    gs, gi, gp = ref_rerank(s, i, graph, k1, lam, kin)
    for b in range(Q.shape[0]):
        A = {int(i[b, j]) for j in range(k1) if s[b, j] >= kth[i[b, j] - off]}
        want = {}
        for j in range(kin):
            B = {int(h) for h in rnbr[i[b, j] - off] if h >= 0}
            jac = len(A & B) / len(A | B) if A | B else 0.0
            want[int(i[b, j])] = (np.float64(F(lam)) * np.float64(s[b, j]) + (1.0 - np.float64(F(lam))) * jac, jac)
        assert sorted(gi[b].tolist()) == sorted(i[b].tolist()) and (i[b, gp[b]] == gi[b]).all()
        f64 = np.array([want[int(x)][0] for x in gi[b]])
        assert np.abs(gs[b] - f64).max() <= 4e-7
        assert (f64[:-1] >= f64[1:] - 1e-6).all()                      # never out of order by more than the rounding
    # J itself, bit for bit against the rounded float64 quotient (correct rounding = within half an ulp)
    for I in range(0, 40):
        for U in range(max(I, 1), 80):
            assert F(I) / F(U) == F(np.float64(I) / np.float64(U))


def test_restatement_edge_cases():
    """Hand-checkable cases: a missing entry's NaN score is not used, lam = 1 gives the order back, an empty A and U == 0 give J = +0,
    equal f is decided by the id, -0.0 ties with +0.0."""
    rnbr = np.array([[10, 11, -1], [10, 11, 12], [-1, -1, -1], [13, -1, -1]], np.int64)      # the lists of rows 10 .. 13
    kth = np.array([0.5, 0.5, 0.9, 0.1], F)
    segs = [(rnbr, kth, 10)]
    idx = np.array([[10, 11, 12, 13, -1, 99]], np.int64)
    sc = np.array([[0.8, 0.6, 0.4, 0.2, np.nan, np.nan]], F)
    s, i, p = ref_rerank(sc, idx, segs, 3, 0.0, 6)                      # A = {10, 11}: 12 scores 0.4 < 0.9
    assert i[0].tolist() == [10, 11, 12, 13, -1, -1] and p[0].tolist() == [0, 1, 2, 3, -1, -1]
    assert s[0, 0] == 1 and s[0, 1] == F(2) / F(3) and s[0, 2] == 0 and s[0, 3] == 0 and np.isneginf(s[0, 4:]).all()
    s, i, p = ref_rerank(sc, idx, segs, 3, 1.0, 4)
    assert i[0].tolist() == [10, 11, 12, 13] and np.array_equal(s[0], sc[0, :4])
    s, i, p = ref_rerank(np.array([[0.0, -0.0, 0.0, -0.0]], F), np.array([[13, 12, 11, 10]], np.int64), segs, 1, 1.0, 4)
    assert i[0].tolist() == [10, 11, 12, 13] and p[0].tolist() == [3, 2, 1, 0] and not np.signbit(s).any()      # -0 + +0 = +0
    s, i, p = ref_rerank(sc[:, :3], np.array([[12, 12 + 2 ** 40, -2 ** 63]], np.int64), segs, 1, 0.0, 2)        # A empty, B empty: U == 0
    assert i[0].tolist() == [12, -1] and s[0, 0] == 0 and not np.signbit(s[0, 0])
    assert ref_rerank(sc, idx, [], 1, 0.5, 2)[1].tolist() == [[-1, -1]]
    pr = ref_prune([(np.array([[5, 6, 7], [5, 6, -1], [7, 99, 5]], np.int64), 5)])[0]
    assert pr.tolist() == [[5, 6, 7], [5, 6, -1], [7, -1, 5]]
    a, b = ref_prune([(np.array([[100, 0], [1, 100]], np.int64), 0), (np.array([[0, 100]], np.int64), 100), (np.zeros((0, 2), np.int64), 50)])[:2]
    assert a.tolist() == [[100, 0], [1, -1]] and b.tolist() == [[0, 100]]


def test_reranking_raises_recall_at_1_on_a_clustered_gallery_with_hubs():
    """What the method is for, on the restatement alone (the GPU kernels inherit it through bitwise equality): a hub row outscores the
    relevant cluster for the queries it was built from, but its reciprocal neighbourhood does not overlap theirs."""
    G, Q, glab, qlab = _clustered()
    k1, kin = 6, 30
    graph = np_graph(G, k1)
    s, i = np_search(Q, G, kin)
    rs, ri, _ = ref_rerank(s, i, graph, k1, 0.3, kin)
    plain, reranked = float((glab[i[:, 0]] == qlab).mean()), float((glab[ri[:, 0]] == qlab).mean())
    print(f"Recall@1 plain {plain:.3f}, re-ranked {reranked:.3f}")
    assert reranked > plain

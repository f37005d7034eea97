"""CPU-side checks (run under -m "not gpu") of the result diversification's host layers: the export of cor_diversify_mmr, its argument
checks (all made before any HIP call), the Python validation, the no-CPU-path rule, and the NumPy restatement that
tests/test_gpu_diversify.py compares the kernel with (tests/diversify_refs.py), itself checked against an independent float64 / Python-set
formulation, on hand-checkable cases, and for what the method is for: distinct clusters on the first page of a composed-object query."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests.diversify_refs import F, chain_pairs, ref_diversify

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_diversify_symbol():
    from cor_amd import _native
    lib = _native.load()
    hdr = open(os.path.join(ROOT, "include", "cor_amd.h")).read()
    proto = re.search(r"^int\s+cor_diversify_mmr\s*\(([^)]*)\)\s*;", hdr, flags=re.M | re.S)
    assert proto, "cor_diversify_mmr is not declared in include/cor_amd.h"
    assert len(proto.group(1).split(",")) == 19 == len(_native.SIGNATURES["cor_diversify_mmr"])
    assert hasattr(lib, "cor_diversify_mmr") and lib.cor_diversify_mmr.restype is _native._i
    sig = _native.SIGNATURES["cor_diversify_mmr"]
    assert sig[11] is _native._f and sig[12] is _native._f                                # lam, max_sim
    assert re.search(r"^#define\s+COR_DIVERSIFY_SEGMAX\s+16\b", hdr, flags=re.M) and _native.DIVERSIFY_SEGMAX == 16


def test_diversify_argument_errors_need_no_gpu():
    """Every argument check comes before any HIP call, so each error comes back on a machine without a device."""
    from cor_amd import _native
    lib = _native.load()
    E, N = _native.EINVAL, _native.ENOSUPPORT
    buf = torch.zeros(64, dtype=torch.int64)
    p = buf.data_ptr()
    inf = float("inf")

    def call(rows=(p,), scale=(None,), offs=(0,), ns=(10,), dts=(_native.F32,), nseg=None, arrays=True, scale_array=True, scores=p, idx=p,
             Bq=1, kin=8, C=64, lam=0.5, max_sim=inf, k=4, out_s=p, out_i=p, out_p=None, out_v=None):
        n = len(rows) if nseg is None else nseg
        a = (ctypes.c_void_p * max(len(rows), 1))(*rows)
        b = (ctypes.c_void_p * max(len(rows), 1))(*scale) if scale_array else None
        c = (ctypes.c_longlong * max(len(rows), 1))(*offs)
        d = (ctypes.c_int * max(len(rows), 1))(*ns)
        e = (ctypes.c_int * max(len(rows), 1))(*dts)
        if not arrays:
            a = c = d = e = None
        return lib.cor_diversify_mmr(a, b, c, d, e, n, scores, idx, Bq, kin, C, lam, max_sim, k, out_s, out_i, out_p, out_v, None)

    # COR_EINVAL
    assert call(scores=None) == E and call(idx=None) == E and call(out_s=None) == E and call(out_i=None) == E and call(arrays=False) == E
    assert call(Bq=-1) == E and call(kin=0) == E and call(k=0) == E and call(k=-3) == E and call(nseg=-1) == E and call(C=0) == E
    assert call(ns=(-1,)) == E and call(rows=(None,)) == E
    assert call(dts=(_native.I8,)) == E and call(dts=(_native.I8,), scale_array=False) == E      # an int8 segment with rows needs its scales
    assert call(lam=float("nan")) == E and call(lam=-0.01) == E and call(lam=1.01) == E and call(lam=inf) == E
    assert call(max_sim=float("nan")) == E
    # COR_ENOSUPPORT
    assert call(kin=4097) == N and call(k=257) == N and call(C=272) == N and call(C=24) == N and call(C=8) == N
    assert call(dts=(3,)) == N and call(dts=(5,)) == N and call(dts=(-1,)) == N                  # x3 split rows are no gallery dtype
    sixteen = dict(rows=(p,) * 16, scale=(None,) * 16, offs=tuple(range(0, 160, 10)), ns=(10,) * 16, dts=(_native.BF16,) * 16)
    seventeen = dict(rows=(p,) * 17, scale=(None,) * 17, offs=tuple(range(0, 170, 10)), ns=(10,) * 17, dts=(_native.F32,) * 17)
    assert call(**seventeen) == N
    # legal without a device: no queries; with them no segments at all is legal too (decided by the same checks)
    assert call(Bq=0) == 0 and call(Bq=0, **sixteen) == 0 and call(Bq=0, rows=(), scale=(), offs=(), ns=(), dts=(), arrays=False) == 0
    assert call(Bq=0, rows=(None,), ns=(0,)) == 0 and call(Bq=0, rows=(None,), ns=(0,), dts=(_native.I8,), scale_array=False) == 0
    assert call(Bq=0, dts=(_native.I8,), scale=(p,)) == 0 and call(Bq=0, dts=(_native.F16,), scale_array=False) == 0
    assert call(Bq=0, out_p=p, out_v=p) == 0 and call(Bq=0, kin=4096, k=256, C=256, lam=1.0, max_sim=-inf) == 0
    assert call(Bq=0, kin=1, k=1, C=16, lam=0.0, max_sim=0.0) == 0
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


def test_diversify_validation_and_no_cpu_path():
    from cor_amd import ops
    from cor_amd.retrieval import GallerySet, QuantizedShard
    G = torch.zeros((5, 16))
    Gq, sc = torch.zeros((5, 16), dtype=torch.int8), torch.ones(5)
    s, i = torch.ones((2, 6)), torch.zeros((2, 6), dtype=torch.int64)
    gs = GallerySet()
    gs._segments = [_cpu_shard(G, 0), _cpu_shard(G[:0], 5), _cpu_quantized(Gq, sc, 20)]   # (add() is not under test)
    for call in (lambda: ops.diversify_mmr([(G, 0)], s, i, 3),
                 lambda: ops.diversify_mmr([(G.half(), 0), (Gq, sc, 9)], s, i, 6, lam=1.0, max_sim=0.7, return_pos=True, return_value=True),
                 lambda: ops.diversify_mmr([], s, i, 1, lam=0.0),
                 lambda: _cpu_shard(G).diversify(s, i),
                 lambda: _cpu_shard(G, 100).diversify(s, i, k=2, lam=0.25, max_sim=0.9, return_pos=True),
                 lambda: _cpu_quantized(Gq, sc).diversify(s, i, k=1),
                 lambda: gs.diversify(s, i),
                 lambda: GallerySet().diversify(s, i, k=4)):
        with pytest.raises(RuntimeError):                              # valid arguments, CPU tensors: there is no CPU path
            call()
    assert not hasattr(QuantizedShard, "diversify")                    # the search-only class does not get the method
    bad = [dict(k=0), dict(k=257), dict(k=-1), dict(lam=-0.1), dict(lam=1.5), dict(lam=float("nan")), dict(lam=float("inf")),
           dict(max_sim=float("nan")),
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
            ops.diversify_mmr(**args)
    with pytest.raises(ValueError, match="17 segments"):
        ops.diversify_mmr([(G[:1], n) for n in range(17)], s, i, 3)
    with pytest.raises(ValueError):
        _cpu_shard(G).diversify(s, i[0])


class _Never:
    """A gallery that must not be touched."""

    def search(self, *a, **kw):
        raise AssertionError("searched before the arguments were validated")

    diversify = search


def test_diversified_search_validates_first_and_composes():
    from cor_amd import retrieval
    for kw in (dict(k=0, k_coarse=5), dict(k=6, k_coarse=5), dict(k=10, k_coarse=257), dict(k=-1, k_coarse=-1), dict(k=2, k_coarse=5, lam=-0.5),
               dict(k=2, k_coarse=5, lam=1.5), dict(k=2, k_coarse=5, lam=float("nan")), dict(k=2, k_coarse=5, max_sim=float("nan"))):
        with pytest.raises(ValueError):
            retrieval.diversified_search(None, _Never(), **kw)
    calls = []

    class Gallery:
        def search(self, q, k, **kw):
            calls.append(("search", q, k, kw))
            return "s", "i"

        def diversify(self, s, i, **kw):
            calls.append(("diversify", s, i, kw))
            return "ds", "di"

    assert retrieval.diversified_search("q", Gallery(), 10, 50, lam=0.4, max_sim=0.8, distinct=True) == ("ds", "di")
    assert calls == [("search", "q", 50, dict(distinct=True)), ("diversify", "s", "i", dict(k=10, lam=0.4, max_sim=0.8))]


def _unit(x):
    return (x / np.linalg.norm(x, axis=-1, keepdims=True)).astype(F)


def np_search(Q, G, k, offset=0):
    """Top-k of Q @ G^T in float32 by (score desc, id asc), NumPy only: (scores f32 [Bq,k], idx i64 [Bq,k])."""
    S = (Q.astype(F) @ G.astype(F).T).astype(F)
    s, i = np.empty((S.shape[0], k), F), np.empty((S.shape[0], k), np.int64)
    for b in range(S.shape[0]):
        o = np.lexsort((np.arange(S.shape[1]), -S[b]))[:k]
        s[b], i[b] = S[b, o], o + offset
    return s, i


def _f64_diversify(scores, ids, X, k, lam, max_sim):
    """An independent formulation for one query whose entries are all present: a float64 Gram matrix, Python sets, a sort per step.
    -> (chosen positions, comparable): comparable is False if any decision was closer than 1e-6 (the two best f of a step, or a
    similarity and max_sim), i.e. if fp32 rounding may legitimately decide otherwise."""
    X64 = X.astype(np.float64)
    gram = X64 @ X64.T
    lam64 = np.float64(F(lam))
    alive, m, chosen, comparable = set(range(len(ids))), {j: 0.0 for j in range(len(ids))}, [], True
    for _ in range(k):
        if not alive:
            break
        ranked = sorted(alive, key=lambda j: -(lam64 * np.float64(scores[j]) - (1.0 - lam64) * m[j]))
        fs = [lam64 * np.float64(scores[j]) - (1.0 - lam64) * m[j] for j in ranked[:2]]
        if len(fs) == 2 and fs[0] - fs[1] <= 1e-6:
            comparable = False
        w = ranked[0]
        chosen.append(w)
        alive.discard(w)
        for j in list(alive):
            v = gram[ids[j], ids[w]]
            m[j] = max(m[j], v)
            if abs(v - max_sim) <= 1e-6:
                comparable = False
            if v >= max_sim:
                alive.discard(j)
    return chosen, comparable


@pytest.mark.parametrize("lam,max_sim", [(0.5, None), (0.3, 0.5), (1.0, 0.7), (0.7, 0.9)])
def test_restatement_against_float64_and_sets(lam, max_sim):
    """ref_diversify against float64 and Python sets on seeded rows (100 groups of 4 look-alikes): wherever no decision of the float64
    run is closer than 1e-6 the selections are identical, and at least 90 % of the queries are that clear-cut. (The fp32 values differ
    from the float64 ones by the chain's rounding, about C * 2^-25 of a similarity below 1, and three roundings of f: well under 1e-6
    at C = 64.)"""
    rng = np.random.default_rng(11)
    C, n, Bq, kin, k = 64, 400, 40, 60, 12
    G = _unit(np.repeat(_unit(rng.standard_normal((n // 4, C))), 4, 0) + F(0.08) * rng.standard_normal((n, C)).astype(F))
    Q = _unit(rng.standard_normal((Bq, C)).astype(F) + G[rng.integers(0, n, Bq)])
    s, i = np_search(Q, G, kin, offset=1000)
    rs, ri, rp, rv = ref_diversify(s, i, [(G, 1000)], k, lam, max_sim)
    clear = 0
    for b in range(Bq):
        chosen, comparable = _f64_diversify(s[b], i[b] - 1000, G, k, lam, np.inf if max_sim is None else max_sim)
        got = [int(p) for p in rp[b] if p >= 0]
        assert (i[b, got] == ri[b, :len(got)]).all() and np.array_equal(rs[b, :len(got)].view(np.int32), s[b, got].view(np.int32))
        assert (ri[b, len(got):] == -1).all() and np.isneginf(rs[b, len(got):]).all() and np.isneginf(rv[b, len(got):]).all()
        if comparable:
            clear += 1
            assert got == chosen, f"query {b}"
    print(f"lam={lam} max_sim={max_sim}: {clear} of {Bq} queries clear-cut")
    assert clear >= 0.9 * Bq


def test_restatement_edge_cases():
    """Hand-checkable cases on rows whose similarities are exact: a missing entry's NaN score is not used, lam = 1 gives the
    (score desc, id asc, position asc) order back with the score bits, equal f is decided by the id and then the position, -0.0 ties with
    +0.0, a repeated id is an entry of its own, max_sim = -inf leaves one output, no segment or no present entry leaves the tail."""
    e = np.eye(16, dtype=F)
    X = np.stack([e[0], e[0], e[1], (e[0] + e[1]) * F(0.5), e[2]])     # rows 10 .. 14: 10 == 11; sim(13, 10) = 0.5, sim(13, 13) = 0.5
    segs = [(X, 10)]
    idx = np.array([[10, 11, 12, 13, 14, -1, 99, 2 ** 40]], np.int64)
    sc = np.array([[0.9, 0.8, 0.7, 0.6, 0.5, np.nan, np.nan, np.nan]], F)
    s, i, p, v = ref_diversify(sc, idx, segs, 8, 1.0, None)
    assert i[0].tolist() == [10, 11, 12, 13, 14, -1, -1, -1] and p[0].tolist() == [0, 1, 2, 3, 4, -1, -1, -1]
    assert np.array_equal(s[0, :5], sc[0, :5]) and np.isneginf(s[0, 5:]).all() and np.array_equal(v[0, :5], sc[0, :5]) and np.isneginf(v[0, 5:]).all()
    s, i, p, v = ref_diversify(sc, idx, segs, 8, 1.0, 0.5)            # 11 == 10 and 13 (sim 0.5 >= 0.5) are suppressed by 10
    assert i[0].tolist() == [10, 12, 14, -1, -1, -1, -1, -1] and p[0, :3].tolist() == [0, 2, 4]
    s, i, p, v = ref_diversify(sc, idx, segs, 3, 0.5, None)           # f: .45 | 11: .4 - .5 = -.1, 12: .35, 13: .3 - .25 = .05, 14: .25
    assert i[0].tolist() == [10, 12, 14] and v[0].tolist() == [F(0.45), F(0.35), F(0.25)] and np.array_equal(s[0], sc[0, [0, 2, 4]])
    s, i, p, v = ref_diversify(sc, idx, segs, 5, 0.0, None)           # f = -m: all-tie at step 0, the lowest id; then the unrelated rows
    assert i[0].tolist() == [10, 12, 14, 13, 11] and v[0].tolist() == [0, 0, 0, -0.5, -1] and np.array_equal(s[0], sc[0, [0, 2, 4, 3, 1]])
    assert ref_diversify(sc, idx, segs, 4, 0.5, -np.inf)[1].tolist() == [[10, -1, -1, -1]]
    z = np.array([[0.0, -0.0, 0.0, -0.0]], F)
    s, i, p, v = ref_diversify(z, np.array([[14, 12, 10, 13]], np.int64), segs, 4, 1.0, None)
    assert i[0].tolist() == [10, 12, 13, 14] and p[0].tolist() == [2, 1, 3, 0] and np.signbit(s[0]).tolist() == [False, True, True, False]
    rep = np.array([[12, 12, 14, 12]], np.int64)                       # a repeated id: entries of their own, ranked by position
    s, i, p, v = ref_diversify(np.array([[0.5, 0.5, 0.5, 0.5]], F), rep, segs, 4, 0.5, None)
    assert i[0].tolist() == [12, 14, 12, 12] and p[0].tolist() == [0, 2, 1, 3] and v[0].tolist() == [0.25, 0.25, -0.25, -0.25]
    assert ref_diversify(np.array([[0.5, 0.5, 0.5, 0.5]], F), rep, segs, 4, 0.5, 1.0)[2].tolist() == [[0, 2, -1, -1]]
    assert ref_diversify(sc, idx, [], 2, 0.5, None)[1].tolist() == [[-1, -1]]
    assert ref_diversify(sc[:, 5:], idx[:, 5:], segs, 2, 0.5, None)[3].tolist() == [[-np.inf, -np.inf]]
    two = [(X[3:], 13), (np.zeros((0, 16), F), 50), (X[:3], 10)]      # the same rows cut into segments, out of order, one empty
    for lam, ms in ((0.5, None), (0.3, 0.5), (1.0, 0.9)):
        a, b = ref_diversify(sc, idx, segs, 6, lam, ms), ref_diversify(sc, idx, two, 6, lam, ms)
        assert all(np.array_equal(x.view(np.int32) if x.dtype == F else x, y.view(np.int32) if y.dtype == F else y) for x, y in zip(a, b))
    assert chain_pairs(X, [3, 0, 3], [0, 3, 3]).tolist() == [0.5, 0.5, 0.5]


def clustered_gallery():
    """The purpose fixture: 150 clusters x 8 near-copies, C = 64, each row its unit-norm centre plus 0.05 x standard-normal noise per
    channel, re-normalised, seed 7; 40 queries, each the normalised mix of 5 cluster centres with weights 1, 0.9, 0.8, 0.7, 0.6.
    -> (G f32 [1200,64], Q f32 [40,64], cluster of every row, the 5 target clusters of every query)."""
    rng = np.random.default_rng(7)
    centres = _unit(rng.standard_normal((150, 64)))
    G = _unit(np.repeat(centres, 8, 0) + 0.05 * rng.standard_normal((1200, 64)))
    targets = np.stack([rng.choice(150, 5, replace=False) for _ in range(40)])
    w = np.array([1, 0.9, 0.8, 0.7, 0.6])
    Q = _unit((centres[targets] * w[None, :, None]).sum(1))
    return G, Q, np.repeat(np.arange(150), 8), targets


def test_diversification_fills_the_first_page_with_distinct_clusters():
    """What the method is for, on the restatement alone (the GPU kernel inherits it through bitwise equality). Mean number of distinct
    clusters among the 10 entries / mean number of the query's 5 target clusters reached, kin = 100, k = 10, as the chain restatement
    gives them: plain top-10 2.475 / 2.475; MMR at lam = 0.5 10.0 / 4.8; suppression at lam = 1, max_sim = 0.7 10.0 / 4.525 (suppression
    keeps the score order, so a fifth, weakest target cluster is reached less often than under MMR). The bounds asserted are the issue's:
    at most 3 plain, at least 9 for both diversified lists. The first entry is the plain list's for every lam > 0."""
    G, Q, cluster, targets = clustered_gallery()
    s, i = np_search(Q, G, 100)
    def stats(ids):
        return (float(np.mean([len(set(cluster[r].tolist())) for r in ids])),
                float(np.mean([len(set(cluster[r].tolist()) & set(t.tolist())) for r, t in zip(ids, targets)])))
    plain = stats(i[:, :10])
    mmr = stats(ref_diversify(s, i, [(G, 0)], 10, 0.5, None)[1])
    sup = stats(ref_diversify(s, i, [(G, 0)], 10, 1.0, 0.7)[1])
    print(f"distinct clusters / targets reached: plain {plain}, MMR(0.5) {mmr}, suppression(0.7) {sup}")
    assert plain[0] <= 3 and mmr[0] >= 9 and sup[0] >= 9
    assert mmr[1] > plain[1] and sup[1] > plain[1]
    for lam in (1.0, 0.5, 0.1):
        assert np.array_equal(ref_diversify(s, i, [(G, 0)], 3, lam, None)[1][:, 0], i[:, 0])

"""CPU-side checks (run under -m "not gpu") of the clustering's host layers: the exports of cor_kmeans_seed / cor_kmeans_update /
cor_kmeans_workspace_bytes and their argument order, every argument error and its precedence (all decided before any HIP call), the
workspace query, the Python validation and the no-CPU-path rule, and the NumPy restatements that tests/test_gpu_cluster.py compares the
kernels with (tests/cluster_refs.py): on a case small enough to follow by eye, against a float64 normalised mean, for independence from
the segmentation, and for what the feature is for: max-min seeding recovers planted modes that random centres merge."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests.cluster_refs import F, planted, purity, ref_assign, ref_cluster, ref_seed, ref_update, sequential_sum

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _proto(name, ret="int"):
    hdr = open(os.path.join(ROOT, "include", "cor_amd.h")).read()
    m = re.search(rf"^{ret}\s+{name}\s*\(([^)]*)\)\s*;", hdr, flags=re.M | re.S)
    assert m, f"{name} is not declared in include/cor_amd.h"
    return [re.sub(r"[\s*]+", " ", a).strip().split(" ")[-1] for a in m.group(1).split(",")], hdr


def test_library_exports_the_clustering_symbols_in_the_documented_order():
    from cor_amd import _native
    lib = _native.load()
    table = ["seg_rows", "seg_scale", "seg_offset", "seg_n", "seg_dtype", "nseg"]
    names, hdr = _proto("cor_kmeans_seed")
    assert names == table + ["C", "K", "first_id", "out_ids", "out_centroids", "workspace", "stream"]
    sig = _native.SIGNATURES["cor_kmeans_seed"]
    assert len(sig) == len(names) == 13 and sig[8] is _native._ll and all(sig[n] is _native._i for n in (5, 6, 7))
    names, _ = _proto("cor_kmeans_update")
    assert names == table + ["seg_assign", "seg_score", "C", "K", "prev", "out_centroids", "out_count", "out_score_sum", "workspace", "stream"]
    sig = _native.SIGNATURES["cor_kmeans_update"]
    assert len(sig) == len(names) == 16 and all(sig[n] is _native._i for n in (5, 8, 9))
    names, _ = _proto("cor_kmeans_workspace_bytes", ret="long")
    assert names == ["n_total", "K", "C"] and _native.SIGNATURES["cor_kmeans_workspace_bytes"] == [_native._l, _native._i, _native._i]
    for fn in ("cor_kmeans_seed", "cor_kmeans_update"):
        assert hasattr(lib, fn) and getattr(lib, fn).restype is _native._i
    assert lib.cor_kmeans_workspace_bytes.restype is _native._l
    for name, value in (("COR_CLUSTER_SEGMAX", 16), ("COR_KMEANS_KMAX", 16384)):
        assert re.search(rf"^#define\s+{name}\s+{value}\b", hdr, flags=re.M)
    assert _native.CLUSTER_SEGMAX == 16 and _native.KMEANS_KMAX == 16384


def _calls():
    from cor_amd import _native
    lib = _native.load()
    buf = torch.zeros(64, dtype=torch.int64)
    p = buf.data_ptr()

    def table(rows, scale, offs, ns, dts, arrays, scale_array):
        m = max(len(rows), 1)
        a = (ctypes.c_void_p * m)(*rows)
        b = (ctypes.c_void_p * m)(*scale) if scale_array else None
        c = (ctypes.c_longlong * m)(*offs)
        d = (ctypes.c_int * m)(*ns)
        e = (ctypes.c_int * m)(*dts)
        return (a, b, c, d, e) if arrays else (None, b, None, None, None)

    def seed(rows=(p,), scale=(None,), offs=(0,), ns=(10,), dts=(_native.F32,), nseg=None, arrays=True, scale_array=True, C=64, K=4, first_id=0,
             out_ids=p, out_c=p, ws=p):
        n = len(rows) if nseg is None else nseg
        return lib.cor_kmeans_seed(*table(rows, scale, offs, ns, dts, arrays, scale_array), n, C, K, first_id, out_ids, out_c, ws, None)

    def update(rows=(p,), scale=(None,), offs=(0,), ns=(10,), dts=(_native.F32,), nseg=None, arrays=True, scale_array=True, assign=(p,),
               assign_array=True, score=None, C=64, K=4, prev=None, out_c=p, out_n=p, out_s=None, ws=p):
        n = len(rows) if nseg is None else nseg
        m = max(len(rows), 1)
        sa = (ctypes.c_void_p * m)(*assign) if assign_array else None
        ss = None if score is None else (ctypes.c_void_p * m)(*score)
        return lib.cor_kmeans_update(*table(rows, scale, offs, ns, dts, arrays, scale_array), n, sa, ss, C, K, prev, out_c, out_n, out_s, ws, None)

    return _native, lib, p, seed, update


def test_every_argument_error_comes_back_without_a_gpu():
    nat, lib, p, seed, update = _calls()
    E, N = nat.EINVAL, nat.ENOSUPPORT
    for call in (seed, update):
        # (1) COR_EINVAL: null outputs / workspace, sizes, null arrays
        assert call(out_c=None) == E and call(ws=None) == E and call(nseg=-1) == E and call(K=0) == E and call(K=-5) == E and call(C=0) == E
        assert call(arrays=False) == E
        # (2) COR_ENOSUPPORT: too many segments
        many = dict(rows=(p,) * 17, scale=(None,) * 17, offs=tuple(range(0, 170, 10)), ns=(10,) * 17, dts=(nat.F32,) * 17)
        if call is update:
            many["assign"] = (p,) * 17
        assert call(**many) == N
        # (3) COR_EINVAL: the entries
        assert call(ns=(-1,)) == E and call(rows=(None,)) == E
        assert call(dts=(nat.I8,)) == E and call(dts=(nat.I8,), scale_array=False) == E      # an int8 segment with rows needs its scales
        # (4) COR_ENOSUPPORT: the limits, an unknown dtype
        assert call(K=16385) == N and call(C=272) == N and call(C=24) == N and call(C=8) == N
        assert call(dts=(3,)) == N and call(dts=(5,)) == N and call(dts=(-1,)) == N          # x3 split rows are no gallery dtype
        big = dict(rows=(p, p), scale=(None, None), offs=(0, 2 ** 31), ns=(2 ** 31 - 1, 1), dts=(nat.F32, nat.F32))
        if call is update:
            big["assign"] = (p, p)
        assert call(**big) == N                                                              # n_total = 2^31
    assert seed(out_ids=None) == E and update(out_n=None) == E
    assert update(assign_array=False) == E and update(assign=(None,)) == E
    assert update(score=(p,)) == E and update(out_s=p) == E                                  # out_score_sum NULL exactly when seg_score is
    assert update(score=(None,), out_s=p) == E                                               # a segment with rows and no scores
    # (5) the seeding: K above the row total, a first id nobody holds
    assert seed(K=11) == E and seed(ns=(0,), rows=(None,), K=1) == E
    assert seed(first_id=10) == E and seed(first_id=-1) == E and seed(offs=(100,), first_id=99) == E and seed(offs=(100,), first_id=2 ** 62) == E
    assert seed(rows=(p, p), scale=(None, None), offs=(0, 50), ns=(10, 10), dts=(nat.F32, nat.BF16), first_id=20) == E   # the gap between two segments


def test_the_precedence_of_the_errors():
    """The order include/cor_amd.h documents: (1) null pointers and sizes, (2) the segment count, (3) the entries, (4) the limits and
    the dtypes, (5) for the seeding K against the row total and first_id."""
    nat, lib, p, seed, update = _calls()
    E, N = nat.EINVAL, nat.ENOSUPPORT
    many = dict(rows=(p,) * 17, scale=(None,) * 17, offs=tuple(range(0, 170, 10)), ns=(10,) * 17, dts=(nat.F32,) * 17)
    for call, extra in ((seed, {}), (update, dict(assign=(p,) * 17))):
        assert call(out_c=None, **many, **extra) == E                                        # (1) before (2)
        assert call(K=0, **many, **extra) == E
        bad_entry = dict(many, ns=(10,) * 16 + (-1,))
        assert call(**bad_entry, **extra) == N                                               # (2) before (3): the arrays are not read
    for call in (seed, update):
        assert call(ns=(-1,), K=16385) == E and call(rows=(None,), C=24) == E                # (3) before (4)
        assert call(ns=(-1,), dts=(7,)) == E
        assert call(K=16385, dts=(7,)) == N and call(C=0, dts=(7,)) == E                     # (1) before (4)
    assert seed(K=16385, ns=(5,)) == N                                                       # (4) before (5): K > KMAX although K > n_total
    assert seed(K=11, dts=(7,)) == N and seed(first_id=77, C=24) == N
    assert seed(K=11, first_id=77) == E


def test_workspace_sweep():
    nat, lib, p, seed, update = _calls()
    ws = lib.cor_kmeans_workspace_bytes
    assert ws(-1, 4, 64) == nat.EINVAL and ws(10, 0, 64) == nat.EINVAL and ws(10, 4, 0) == nat.EINVAL
    assert ws(10, 16385, 64) == nat.ENOSUPPORT and ws(10, 4, 272) == nat.ENOSUPPORT and ws(10, 4, 24) == nat.ENOSUPPORT
    assert ws(2 ** 31, 4, 64) == nat.ENOSUPPORT and ws(2 ** 31 - 1, 1, 16) > 0
    assert ws(-1, 16385, 64) == nat.EINVAL                                                   # the sizes first
    last = {}
    for n in (0, 1, 255, 256, 2047, 2048, 2049, 5000, 10 ** 6, 10 ** 8):
        for K in (1, 2, 33, 1024, 16384):
            for C in (16, 64, 256):
                b = ws(n, K, C)
                assert b > 0 and b % 256 == 0
                # what the definition needs at the least: a member list, the tiles x K counts, a partial row per possible chunk
                tiles = -(-n // 2048)
                assert b >= 4 * n + 4 * tiles * K + 4 * C * (n // 256 + K)
                assert b <= 4 * (2 * n + 2048) + 4 * tiles * K + (4 * C + 4) * (n // 256 + K) + 8 * (K + 1) + 16 * 256 + 4096 * 16 + 4 * n
                for key in ((K, C, "n"), (n, C, "K"), (n, K, "C")):                          # monotone in every argument
                    assert b >= last.get(key, (0, 0))[1] or last[key][0] > (n, K, C)
                    last[key] = ((n, K, C), b)


def _cpu_shard(rows, offset=0):
    from cor_amd.retrieval import GalleryShard
    sh = GalleryShard.__new__(GalleryShard)
    sh.rows, sh.offset, sh.labels, sh.groups = rows, offset, None, None
    return sh


def _cpu_quantized(rows, scales, offset=0):
    from cor_amd.retrieval import QuantizedGallery
    sh = QuantizedGallery.__new__(QuantizedGallery)
    sh.rows, sh.scales, sh.offset, sh.labels, sh.groups = rows, scales, offset, None, None
    return sh


def test_validation_and_no_cpu_path():
    from cor_amd import ops
    from cor_amd.retrieval import Clustering, GallerySet, QuantizedShard
    G = torch.zeros((5, 16))
    Gq, sc = torch.zeros((5, 16), dtype=torch.int8), torch.ones(5)
    a = torch.zeros(5, dtype=torch.int32)
    gs = GallerySet()
    gs._segments = [_cpu_shard(G, 0), _cpu_shard(G[:0], 5), _cpu_quantized(Gq, sc, 20)]   # (add() is not under test)
    for call in (lambda: ops.kmeans_seed([(G, 0)], 3),
                 lambda: ops.kmeans_seed([(G.half(), 0), (Gq, sc, 9)], 10, first_id=11),
                 lambda: ops.kmeans_update([(G, 0)], [a], 3),
                 lambda: ops.kmeans_update([(G.bfloat16(), 7), (Gq, sc, 0)], [a, a], 16384, scores=[sc, sc], prev=torch.zeros((16384, 16))),
                 lambda: _cpu_shard(G).cluster(2),
                 lambda: _cpu_shard(G, 100).cluster(5, iters=1, first_id=102, batch=2),
                 lambda: _cpu_shard(G).cluster(2, init=torch.zeros((2, 16))),
                 lambda: _cpu_quantized(Gq, sc).cluster(1),
                 lambda: gs.cluster(10)):
        with pytest.raises(RuntimeError):                              # valid arguments, CPU tensors: there is no CPU path
            call()
    assert not hasattr(QuantizedShard, "cluster")                      # the search-only class does not get the method
    assert hasattr(Clustering, "assign_queries")
    bad_seed = [dict(K=0), dict(K=6), dict(K=16385), dict(first_id=5), dict(first_id=-1), dict(segments=[]),
                dict(segments=[(G[:1], n) for n in range(17)]), dict(segments=[(G, 0), (G, 3)]), dict(segments=[(G, 0), (torch.zeros((5, 32)), 10)]),
                dict(segments=[(G.double(), 0)]), dict(segments=[(torch.zeros((5, 24)), 0)]), dict(segments=[(Gq, 0)]), dict(segments=[(Gq, sc[:4], 0)])]
    for kw in bad_seed:
        args = dict(segments=[(G, 0)], K=3)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.kmeans_seed(**args)
    bad_update = [dict(K=0), dict(K=16385), dict(assigns=[]), dict(assigns=[a, a]), dict(assigns=[a.long()]), dict(assigns=[a[:4]]),
                  dict(scores=[sc.double()]), dict(scores=[sc[:4]]), dict(scores=[]), dict(prev=torch.zeros((3, 32))), dict(prev=torch.zeros((4, 16))),
                  dict(out=torch.zeros((3, 16), dtype=torch.float16)), dict(segments=[(G, 0), (G, 3)], assigns=[a, a]),
                  dict(segments=[(G[:1], n) for n in range(17)], assigns=[a[:1]] * 17)]
    for kw in bad_update:
        args = dict(segments=[(G, 0)], assigns=[a], K=3)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.kmeans_update(**args)
    same = torch.zeros((3, 16))
    with pytest.raises(ValueError):
        ops.kmeans_update([(G, 0)], [a], 3, prev=same, out=same)
    for kw in (dict(n_clusters=0), dict(n_clusters=6), dict(n_clusters=2, iters=0), dict(n_clusters=2, batch=0), dict(n_clusters=2, init="random"),
               dict(n_clusters=2, init=torch.zeros((3, 16))), dict(n_clusters=2, init=torch.zeros((2, 16), dtype=torch.float64))):
        with pytest.raises(ValueError):
            _cpu_shard(G).cluster(**kw)
    for empty in (_cpu_shard(G[:0]), GallerySet(), _cpu_quantized(Gq[:0], sc[:0])):
        with pytest.raises(ValueError):
            empty.cluster(1)


def _bits(x):
    return np.asarray(x, dtype=F).view(np.int32)


def test_sequential_sum_is_the_explicit_loop():
    rng = np.random.default_rng(0)
    x = rng.standard_normal((300, 16)).astype(F)
    x[0] = -0.0                                                        # +0 + -0 = +0: the running sum starts at +0, not at the first element
    v = np.zeros(16, F)
    for r in x:
        v = v + r
    assert np.array_equal(_bits(sequential_sum(x)), _bits(v)) and not np.signbit(sequential_sum(x[:1])).any()
    q = np.float32(0)
    for r in x[:, 3]:
        q = q + r
    assert _bits(sequential_sum(x[:, 3])) == _bits(q)                  # a vector of scores


def test_a_case_to_follow_by_eye():
    """Six rows, ids 10 .. 15, C = 16: e0, e1, e0, (e0 + e1) / 2, -e0, e2.
    Seeding from id 10: best = 1, 0, 1, .5, -1, 0 -> 14 (-e0); against -e0 nothing rises (-1, 0, -1, -.5, ., 0), ids 11 and 15 tie at 0 ->
    11 (e1); against e1 id 13 stays at .5, id 15 at 0 -> 15; then 13 (.5) before 12 (1, the twin of the first row: chosen last).
    Update with assign 0, 1, 0, 1, -1, 0: cluster 0 = e0 + e0 + e2 = (2, 0, 1), norm sqrt(5); cluster 1 = e1 + (.5, .5) = (.5, 1.5), norm
    sqrt(2.5); id 14 belongs to no cluster; dyadic scores add exactly."""
    e = np.eye(16, dtype=F)
    X = np.stack([e[0], e[1], e[0], (e[0] + e[1]) * F(0.5), -e[0], e[2]])
    segs = [(X, 10)]
    ids, cent = ref_seed(segs, 6, first_id=10)
    assert ids.tolist() == [10, 14, 11, 15, 13, 12] and np.array_equal(cent, X[[0, 4, 1, 5, 3, 2]])
    assert ref_seed(segs, 2)[0].tolist() == [10, 14] and ref_seed(segs, 3, first_id=13)[0].tolist() == [13, 14, 15]
    a = np.array([0, 1, 0, 1, -1, 0], np.int32)
    sc = np.array([1, .5, .25, .125, 64, 2], F)
    cent, counts, sums = ref_update(segs, [a], 2, scores=[sc])
    assert counts.tolist() == [3, 2] and sums.tolist() == [3.25, .625]
    want0, want1 = np.zeros(16, F), np.zeros(16, F)
    want0[0], want0[2] = F(2) / np.sqrt(F(5)), F(1) / np.sqrt(F(5))
    want1[0], want1[1] = F(.5) / np.sqrt(F(2.5)), F(1.5) / np.sqrt(F(2.5))
    assert np.array_equal(_bits(cent[0]), _bits(want0)) and np.array_equal(_bits(cent[1]), _bits(want1))
    # an empty cluster: prev bit for bit, or +0; values outside [0, K) belong to no cluster
    prev = np.full((4, 16), -0.0, F)
    prev[3, 5] = np.nan
    b = np.array([0, 4, 0, -2 ** 31, 2, 7], np.int32)
    cent, counts, sums = ref_update(segs, [b], 4, scores=[sc], prev=prev)
    assert counts.tolist() == [2, 0, 1, 0] and sums.tolist() == [1.25, 0, 64, 0]
    assert np.array_equal(_bits(cent[[1, 3]]), _bits(prev[[1, 3]])) and np.array_equal(cent[0], e[0]) and np.array_equal(cent[2], -e[0])
    cent, counts, sums = ref_update(segs, [b], 4)
    assert sums is None and np.array_equal(_bits(cent[[1, 3]]), np.zeros((2, 16), np.int32))
    # the assignment: the nearest centre, ties to the lower cluster
    idx, s = ref_assign(np.stack([e[0], e[1], e[1]]), X)
    assert idx.tolist() == [0, 1, 0, 0, 1, 0] and s.tolist() == [1, 1, 1, .5, 0, 0]


@pytest.mark.parametrize("n,K,C", [(1, 1, 16), (257, 3, 64), (1000, 7, 256), (5000, 2, 128)])
def test_the_restated_centre_is_the_normalised_mean(n, K, C):
    """Within 1e-6 of the float64 normalised sum, per coordinate: a sequential fp32 sum of m terms of magnitude <= 1 is off by at most
    m u |sum of magnitudes| relatively to the norm, and clusters of unit rows that point one way keep that far below 1e-6 at these sizes."""
    rng = np.random.default_rng(n)
    centre = rng.standard_normal((K, C))
    a = rng.integers(0, K, n).astype(np.int32)
    X = centre[a] + 0.3 * rng.standard_normal((n, C))
    X = (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(F)
    cent, counts, _ = ref_update([(X, 0)], [a], K)
    for c in range(K):
        if counts[c]:
            v = X[a == c].astype(np.float64).sum(0)
            assert np.abs(cent[c] - v / np.linalg.norm(v)).max() <= 1e-6
            assert abs(np.linalg.norm(cent[c].astype(np.float64)) - 1) <= 1e-6
    assert counts.sum() == n and np.array_equal(counts, np.bincount(a, minlength=K))


def test_the_restatements_do_not_depend_on_the_segmentation():
    rng = np.random.default_rng(7)
    X = rng.standard_normal((700, 32)).astype(F)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    a = rng.integers(-1, 6, 700).astype(np.int32)
    sc = rng.random(700).astype(F)
    off = 2 ** 33
    one = [(X, off)]
    cut = [(X[500:], off + 500), (X[:0], 5), (X[:300], off), (X[300:500], off + 300)]                # out of order, one of them empty
    cuta, cuts = [a[500:], a[:0], a[:300], a[300:500]], [sc[500:], sc[:0], sc[:300], sc[300:500]]
    for x, y in zip(ref_update(one, [a], 5, scores=[sc]), ref_update(cut, cuta, 5, scores=cuts)):
        assert np.array_equal(_bits(x) if x.dtype == F else x, _bits(y) if y.dtype == F else y)
    for kw in (dict(), dict(first_id=off + 450)):
        (i1, c1), (i2, c2) = ref_seed(one, 40, **kw), ref_seed(cut, 40, **kw)
        assert np.array_equal(i1, i2) and np.array_equal(_bits(c1), _bits(c2)) and len(set(i1.tolist())) == 40
    r1, r2 = ref_cluster(one, 6, iters=4), ref_cluster(cut, 6, iters=4)
    assert r1["objective"] == r2["objective"] and np.array_equal(_bits(r1["centroids"]), _bits(r2["centroids"]))
    assert np.array_equal(np.concatenate(r1["assign"]), np.concatenate(r2["assign"])) and [len(x) for x in r2["assign"]] == [300, 200, 200]
    # a gap in the ids moves nothing but the ids
    gap = [(X[:300], off), (X[300:], off + 1000)]
    i3 = ref_seed(gap, 40)[0]
    assert np.array_equal(np.where(i3 >= off + 1000, i3 - 700, i3), ref_seed(one, 40)[0])


def test_max_min_seeding_recovers_the_planted_modes():
    """The purpose fixture: 3 000 unit rows, C = 64, 30 planted directions from default_rng(1234), row i from direction i mod 30 plus
    0.05 N(0, 1) per coordinate, normalised. Every row's cosine to its own direction is >= 0.877 (0.87724) and to any other <= 0.525
    (0.52507), by a float32 matrix product.
    Measured with this bit-exact restatement: max-min seeding, K = 30: 2 passes, converged, objective 0.8602192 -> 0.9295681, purity 1.0,
    no empty cluster, every count 100. A skewed draw (mode m with probability ~ 1 / (1 + m)): 2 passes, 0.8598312 -> 0.9294207, purity 1.0,
    no empty cluster. K = 45: 9 passes, 0.8658 -> 0.9306, purity 1.0, no empty cluster. The same loop started from 30 rows drawn by
    torch.randperm (seeds 0 .. 4) ends at purity 0.80, 0.80, 0.87, 0.77, 0.83 with 0, 1, 0, 0, 2 empty clusters."""
    X, mode, d = planted()
    S = X @ d.T
    own = S[np.arange(3000), mode]
    S[np.arange(3000), mode] = -1
    assert round(float(own.min()), 3) == 0.877 and round(float(S.max()), 3) == 0.525      # the figures above, to the digits they are quoted with
    r = ref_cluster([(X, 0)], 30, iters=20)
    print("max-min:", r["iters"], r["converged"], r["objective"])
    assert r["iters"] <= 20 and r["converged"]
    assert purity(r["assign"][0], mode, 30) == 1.0 and (r["counts"] == 100).all()
    assert all(b - a >= -1e-6 for a, b in zip(r["objective"], r["objective"][1:]))
    assert len(set(mode[ref_seed([(X, 0)], 30)[0]].tolist())) == 30           # the seeds themselves: one per planted direction
    Xs, ms, _ = planted(skew=True)
    rs = ref_cluster([(Xs, 0)], 30)
    assert purity(rs["assign"][0], ms, 30) == 1.0 and (rs["counts"] > 0).all() and rs["converged"]
    r45 = ref_cluster([(X, 0)], 45)
    assert purity(r45["assign"][0], mode, 45) == 1.0 and (r45["counts"] > 0).all()
    assert all(b - a >= -1e-6 for a, b in zip(r45["objective"], r45["objective"][1:]))
    worst = []
    for seed in range(5):
        g = torch.Generator().manual_seed(seed)
        rr = ref_cluster([(X, 0)], 30, init=X[torch.randperm(3000, generator=g)[:30].numpy()])
        worst.append((purity(rr["assign"][0], mode, 30), int((rr["counts"] == 0).sum())))
    print("random centres:", worst)
    assert all(p < 0.9 for p, _ in worst)                              # which is why the seeding is part of the feature

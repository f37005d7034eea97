"""CPU-side checks (run under -m "not gpu") of the list fusion's host layers: the export of cor_fuse_lists and its workspace query, the
argument checks (all made before any HIP call), the Python validation, the no-CPU-path rule, and the NumPy restatement that
tests/test_gpu_fuse.py compares the kernel with (tests/fuse_refs.py), itself checked against an independent float64 / Python-dict
formulation, on hand-checkable cases, and for what the method is for: fused views find the target more often than the best single view."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests.fuse_refs import F, ref_fuse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = float("inf"), float("nan")


def _bits(x):
    return np.asarray(x, F).view(np.int32)


def test_library_exports_the_fuse_symbols():
    from cor_amd import _native
    lib = _native.load()
    hdr = open(os.path.join(ROOT, "include", "cor_amd.h")).read()
    for name, ret, arity in (("cor_fuse_lists", "int", 16), ("cor_fuse_lists_workspace_bytes", "long", 4)):
        proto = re.search(r"^%s\s+%s\s*\(([^)]*)\)\s*;" % (ret, name), hdr, flags=re.M | re.S)
        assert proto, f"{name} is not declared in include/cor_amd.h"
        assert len(proto.group(1).split(",")) == arity == len(_native.SIGNATURES[name])
        assert hasattr(lib, name)
    assert lib.cor_fuse_lists.restype is _native._i and lib.cor_fuse_lists_workspace_bytes.restype is _native._l
    sig = _native.SIGNATURES["cor_fuse_lists"]
    assert sig[9] is _native._f and sig[5] is _native._p                                  # rrf_c, weights_host
    assert re.search(r"^#define\s+COR_FUSE_PMAX\s+16\b", hdr, flags=re.M) and _native.FUSE_PMAX == 16
    for name in ("RRF", "SUM", "MAX", "NORM_NONE", "NORM_MINMAX", "MISSING_ZERO", "MISSING_FLOOR"):
        m = re.search(r"^#define\s+COR_FUSE_%s\s+(\d+)\b" % name, hdr, flags=re.M)
        assert m and int(m.group(1)) == getattr(_native, "FUSE_" + name)


def test_fuse_argument_errors_need_no_gpu():
    """Every argument check comes before any HIP call, so each error comes back on a machine without a device."""
    from cor_amd import _native as n
    lib = n.load()
    E, N = n.EINVAL, n.ENOSUPPORT
    buf = torch.zeros(64, dtype=torch.int64)
    p = buf.data_ptr()
    ones = (1.0,) * 16

    def call(scores=p, idx=p, P=2, Bq=1, kin=8, w=ones, weights=True, mode=n.FUSE_RRF, norm=n.FUSE_NORM_NONE, missing=n.FUSE_MISSING_ZERO,
             rrf_c=60.0, k=4, out_s=p, out_i=p, out_c=None):
        wa = (ctypes.c_float * max(len(w), 1))(*w) if weights else None
        return lib.cor_fuse_lists(scores, idx, P, Bq, kin, wa, mode, norm, missing, rrf_c, k, out_s, out_i, out_c, None, None)

    SUM, MAX, MM, FL = n.FUSE_SUM, n.FUSE_MAX, n.FUSE_NORM_MINMAX, n.FUSE_MISSING_FLOOR
    # COR_EINVAL
    assert call(scores=None) == E and call(idx=None) == E and call(weights=False) == E and call(out_s=None) == E and call(out_i=None) == E
    assert call(P=0) == E and call(P=-1) == E and call(Bq=-1) == E and call(kin=0) == E and call(k=0) == E and call(k=-3) == E
    assert call(mode=3) == E and call(mode=-1) == E and call(norm=2) == E and call(norm=-1) == E and call(missing=2) == E and call(missing=-1) == E
    assert call(norm=MM) == E and call(missing=FL) == E and call(norm=MM, missing=FL) == E           # RRF uses ranks alone
    assert call(mode=MAX, missing=FL) == E and call(mode=MAX, norm=MM, missing=FL) == E
    for bad in (NAN, INF, -INF):
        assert call(w=(1.0, bad)) == E and call(w=(bad, 1.0), mode=SUM) == E and call(w=(bad, 1.0), mode=MAX, Bq=0) == E
    assert call(rrf_c=NAN) == E and call(rrf_c=INF) == E and call(rrf_c=-1.0) == E and call(rrf_c=-INF) == E
    # COR_ENOSUPPORT
    assert call(P=17, kin=1, w=(1.0,) * 17) == N and call(P=2, kin=2049) == N and call(P=1, kin=4097) == N and call(P=16, kin=257) == N
    assert call(k=257) == N
    lw = lib.cor_fuse_lists_workspace_bytes
    assert lw(0, 1, 8, 4) == E and lw(2, -1, 8, 4) == E and lw(2, 1, 0, 4) == E and lw(2, 1, 8, 0) == E
    assert lw(17, 1, 1, 4) == N and lw(2, 1, 2049, 4) == N and lw(2, 1, 8, 257) == N
    assert lw(2, 1, 8, 4) == 0 and lw(16, 512, 256, 256) == 0 and lw(1, 0, 4096, 1) == 0
    # legal without a device: no queries
    assert call(Bq=0) == 0 and call(Bq=0, P=16, kin=256, k=256) == 0 and call(Bq=0, P=1, kin=4096, k=256, out_c=p) == 0
    assert call(Bq=0, P=1, kin=1, k=1, rrf_c=0.0) == 0 and call(Bq=0, w=(0.0, -2.5)) == 0
    assert call(Bq=0, mode=SUM) == 0 and call(Bq=0, mode=SUM, missing=FL) == 0 and call(Bq=0, mode=SUM, norm=MM) == 0
    assert call(Bq=0, mode=SUM, norm=MM, missing=FL, out_c=p) == 0 and call(Bq=0, mode=MAX) == 0 and call(Bq=0, mode=MAX, norm=MM) == 0
    assert call(Bq=0, mode=SUM, rrf_c=NAN) == 0 and call(Bq=0, mode=MAX, rrf_c=-1.0) == 0           # rrf_c is RRF's alone


class _Never:
    """A gallery that must not be touched."""

    def search(self, *a, **kw):
        raise AssertionError("searched before the arguments were validated")


class _CpuGallery:
    """A gallery whose search returns CPU lists: the fusion behind it has no CPU path."""

    def __init__(self):
        self.calls = []

    def search(self, q, k, **kw):
        self.calls.append((tuple(q.shape), k, kw))
        return torch.ones((q.shape[0], k)), torch.arange(k).expand(q.shape[0], k).contiguous()


def test_fuse_validation_and_no_cpu_path():
    from cor_amd import ops, retrieval
    s, i = torch.ones((3, 2, 6)), torch.zeros((3, 2, 6), dtype=torch.int64)
    gal = _CpuGallery()
    q = torch.zeros((3, 2, 16))
    for call in (lambda: ops.fuse_lists(s, i, 4),
                 lambda: ops.fuse_lists(s, i, 256, weights=[1, 0, -0.5], mode="sum", normalize="minmax", missing="floor", return_count=True),
                 lambda: ops.fuse_lists(s[:1], i[:1], 1, weights=torch.ones(1), mode="max", normalize="minmax"),
                 lambda: ops.fuse_lists(torch.ones((16, 1, 256)), torch.zeros((16, 1, 256), dtype=torch.int64), 256, rrf_c=0.0),
                 lambda: retrieval.fuse_lists_device(list(s), list(i), 4),
                 lambda: retrieval.fuse_lists_device([s[0], s[1, :, :2]], [i[0], i[1, :, :2]], 3, mode="sum", weights=(1, 2), return_count=True),
                 lambda: retrieval.fused_search(q, gal, 5, 7),
                 lambda: retrieval.fused_search(list(q), [gal, gal, gal], 5, 7, mode="sum", normalize="minmax", weights=[1, 2, 3], distinct=True)):
        with pytest.raises(RuntimeError):                              # valid arguments, CPU tensors: there is no CPU path
            call()
    assert gal.calls[:3] == [((2, 16), 7, {})] * 3 and gal.calls[3:] == [((2, 16), 7, dict(distinct=True))] * 3
    retrieval_calls = len(gal.calls)
    with pytest.raises(RuntimeError):
        retrieval.fused_search(q, gal, 5, 7, query_labels=[1, 2], filter_mode="ne")
    assert gal.calls[retrieval_calls][2] == dict(query_labels=[1, 2], mode="ne")     # the filter's mode reaches the searches as `mode`

    big_s, big_i = torch.ones((17, 1, 2)), torch.zeros((17, 1, 2), dtype=torch.int64)
    bad = [dict(scores=big_s, idx=big_i),                                                # 17 lists
           dict(scores=torch.ones((1, 1, 4097)), idx=torch.zeros((1, 1, 4097), dtype=torch.int64)),        # 4097 entries
           dict(scores=torch.ones((16, 1, 257)), idx=torch.zeros((16, 1, 257), dtype=torch.int64)),
           dict(k=0), dict(k=257), dict(k=-1),
           dict(weights=[1, 2]), dict(weights=[1, 2, 3, 4]), dict(weights=[1, NAN, 1]), dict(weights=[1, INF, 1]), dict(weights=[1, 1e39, 1]),
           dict(weights=torch.ones(3, device="meta")),                                  # a tensor that does not live on the host
           dict(normalize="minmax"), dict(missing="floor"), dict(mode="max", missing="floor"), dict(mode="rrf", rrf_c=-1.0),
           dict(rrf_c=NAN), dict(rrf_c=INF), dict(mode="mnz"), dict(normalize="zscore"), dict(missing="mean"), dict(mode=0),
           dict(scores=s.double()), dict(scores=s[0]), dict(scores=s[:, :, :0]), dict(scores=s[:0], idx=i[:0]), dict(idx=i.to(torch.int32)),
           dict(idx=i[:2]), dict(idx=i[:, :, :5]), dict(scores=s.numpy())]
    for kw in bad:
        args = dict(scores=s, idx=i, k=3)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.fuse_lists(**args)
    with pytest.raises(ValueError, match="17 lists"):
        ops.fuse_lists(big_s, big_i, 3)
    parts = lambda n, w: ([torch.ones((2, w))] * n, [torch.zeros((2, w), dtype=torch.int64)] * n)
    for sp, ip, kw in ((*parts(17, 2), {}), (*parts(2, 2049), {}), ([torch.ones((2, 4096)), torch.ones((2, 1))], [i[0, :, :1].expand(2, 4096), i[0, :, :1]], {}),
                       ([], [], {}), (list(s), list(i[:2]), {}), ([s[0], s[1, :1]], [i[0], i[1, :1]], {}), ([s[0, 0]], [i[0, 0]], {}),
                       ([s[0].half()], [i[0]], {}), ([s[0]], [i[0].int()], {}), (list(s), list(i), dict(k=0)), (list(s), list(i), dict(k=257)),
                       (list(s), list(i), dict(weights=[1, 2])), (list(s), list(i), dict(mode="rrf", normalize="minmax")),
                       (list(s), list(i), dict(mode="max", missing="floor"))):
        kw = dict(dict(k=3), **kw)
        with pytest.raises(ValueError):
            retrieval.fuse_lists_device(sp, ip, **kw)
    for kw in (dict(k=0), dict(k=257), dict(k_each=0), dict(k_each=257), dict(k_each=-1), dict(weights=[1, 2]), dict(weights=[1, 2, NAN]),
               dict(normalize="minmax"), dict(mode="max", missing="floor"), dict(rrf_c=-0.5), dict(gallery=[_Never(), _Never()]),
               dict(gallery=[_Never()] * 4), dict(queries=torch.zeros((17, 2, 16))), dict(queries=torch.zeros((2, 16))), dict(queries=[]),
               dict(queries=[q[0], q[1, :1], q[2]]), dict(queries=[q[0], q[1][0], q[2]])):
        args = dict(queries=q, gallery=_Never(), k=5, k_each=7)
        args.update(kw)
        with pytest.raises(ValueError):
            retrieval.fused_search(**args)


def _f64_fuse(scores, idx, weights, mode, rrf_c, normalize, missing, b):
    """An independent formulation for query b: float64 throughout, a Python dict per query, statistics with min() / max() over lists of
    float64 values -> {id: (fused value, sum of |c_p|, count)}."""
    P, _, kin = scores.shape
    w = [float(F(x)) for x in weights]
    lists = []
    for p in range(P):
        seen = {}
        for e in range(kin):
            i, s = int(idx[p, b, e]), float(scores[p, b, e])
            if i >= 0 and np.isfinite(s):
                seen.setdefault(i, (e + 1, s))
        lists.append(seen)
    out = {}
    for i in set(i for h in lists for i in h):
        cs, cnt = [], 0
        for p, h in enumerate(lists):
            if not h:
                continue
            lo, hi = min(v[1] for v in h.values()), max(v[1] for v in h.values())
            if i in h:
                rank, s = h[i]
                if mode == "rrf":
                    c = w[p] / (float(F(rrf_c)) + rank)
                else:
                    c = w[p] * (s if normalize == "none" else 1.0 if hi == lo else (s - lo) / (hi - lo))
                cs.append((c, True))
                cnt += 1
            elif missing == "floor":
                cs.append((w[p] * (lo if normalize == "none" else 0.0), False))
        value = max(c for c, holds in cs if holds) if mode == "max" else sum(c for c, _ in cs)
        out[i] = (value, sum(abs(c) for c, _ in cs), cnt)
    return out


COMBOS = [("rrf", "none", "zero"), ("sum", "none", "zero"), ("sum", "none", "floor"), ("sum", "minmax", "zero"), ("sum", "minmax", "floor"),
          ("max", "none", "zero"), ("max", "minmax", "zero")]


@pytest.mark.parametrize("mode,normalize,missing", COMBOS)
def test_restatement_against_float64_and_dicts(mode, normalize, missing):
    """ref_fuse against the float64 formulation on seeded lists (ids shared between the lists, holes, repeats, continuous scores): every
    fused value within (P + 3) * 2^-23 * sum|c_p| of the float64 one (twice the first-order worst case of P additions and at most 3
    roundings per term), the counts equal, and the two orders agree at every rank whose float64 value is more than twice that bound away
    from both neighbours."""
    rng = np.random.default_rng(5)
    checked = 0
    for P, Bq, kin in ((1, 4, 30), (2, 6, 25), (3, 6, 40), (5, 5, 20), (8, 4, 12), (16, 3, 10)):
        pool = max(3, P * kin // 3)
        idx = rng.integers(0, pool, (P, Bq, kin)).astype(np.int64) + 2 ** 33
        scores = rng.standard_normal((P, Bq, kin)).astype(F)
        hole = rng.random((P, Bq, kin)) < 0.1
        idx[hole] = -1
        scores[rng.random((P, Bq, kin)) < 0.03] = -np.inf
        weights = [F(x) for x in rng.choice([1.0, 0.5, 2.0, 0.3, -0.25, 0.0], P)]
        for b in range(Bq):
            want = _f64_fuse(scores, idx, weights, mode, 60.0, normalize, missing, b)
            n = len(want)
            gs, gi, gc = ref_fuse(scores[:, b:b + 1], idx[:, b:b + 1], weights, mode, 60.0, normalize, missing, n + 2)
            assert (gi[0, n:] == -1).all() and np.isneginf(gs[0, n:]).all() and (gc[0, n:] == -1).all()
            assert sorted(gi[0, :n].tolist()) == sorted(want)
            bound = {i: (P + 3) * 2.0 ** -23 * want[i][1] for i in want}
            for r in range(n):
                i = int(gi[0, r])
                assert abs(float(gs[0, r]) - want[i][0]) <= bound[i], (mode, normalize, missing, P, b, i)
                assert gc[0, r] == want[i][2]
            order = sorted(want, key=lambda i: (-want[i][0], i))
            worst = 2 * max(bound.values())
            for r, i in enumerate(order):
                clear = (r == 0 or want[order[r - 1]][0] - want[i][0] > worst) and (r == n - 1 or want[i][0] - want[order[r + 1]][0] > worst)
                if clear:
                    checked += 1
                    assert gi[0, r] == i
    assert checked > 100


A1, A2, T, B1, B2 = 10, 11, 7, 20, 21


def _two(sa, sb, ia=(A1, A2, T), ib=(B1, T, B2)):
    return np.array([[sa], [sb]], F), np.array([[ia], [ib]], np.int64)


def test_restatement_hand_cases():
    """List A = [a1, a2, t] and list B = [b1, t, b2] (ids 10, 11, 7 and 20, 7, 21), scores that are exact in binary."""
    one = F(1)
    s, i = _two([1.0, 0.75, 0.5], [1.0, 0.375, 0.25])
    # RRF, c = 60: t is third in A and second in B
    fs, fi, fc = ref_fuse(s, i, [1, 1], "rrf", 60.0, "none", "zero", 6)
    assert fi[0].tolist() == [T, A1, B1, A2, B2, -1] and fc[0].tolist() == [2, 1, 1, 1, 1, -1]
    assert _bits(fs[0, 0]) == _bits(one / F(63) + one / F(62)) and _bits(fs[0, 1]) == _bits(fs[0, 2]) == _bits(one / F(61))
    assert _bits(fs[0, 3]) == _bits(one / F(62)) and _bits(fs[0, 4]) == _bits(one / F(63)) and np.isneginf(fs[0, 5])
    # CombSUM: without the floor t's two scores add up past a2; with it every single-list row gains the other list's least score
    fs, fi, fc = ref_fuse(s, i, [1, 1], "sum", 60.0, "none", "zero", 5)
    assert fi[0].tolist() == [A1, B1, T, A2, B2] and fs[0].tolist() == [1.0, 1.0, 0.875, 0.75, 0.25] and fc[0].tolist() == [1, 1, 2, 1, 1]
    fs, fi, fc = ref_fuse(s, i, [1, 1], "sum", 60.0, "none", "floor", 5)
    assert fi[0].tolist() == [B1, A1, A2, T, B2] and fs[0].tolist() == [1.5, 1.25, 1.0, 0.875, 0.75] and fc[0].tolist() == [1, 1, 1, 2, 1]
    # CombMAX with weights (1, 0.5): t = max(0.5, 0.1875) ties with b1 = 0.5 and the id decides
    fs, fi, fc = ref_fuse(s, i, [1, 0.5], "max", 60.0, "none", "zero", 5)
    assert fi[0].tolist() == [A1, A2, T, B1, B2] and fs[0].tolist() == [1.0, 0.75, 0.5, 0.5, 0.125] and fc[0].tolist() == [1, 1, 2, 1, 1]
    # a list with mx == mn: every value of A is 1; B's are (s - 0.25) / 0.75
    sa, _ = _two([2.0, 2.0, 2.0], [1.0, 0.375, 0.25])
    fs, fi, fc = ref_fuse(sa, i, [1, 1], "sum", 60.0, "minmax", "zero", 5)
    assert fi[0].tolist() == [T, A1, A2, B1, B2] and _bits(fs[0, 0]) == _bits(one + F(0.125) / F(0.75))
    assert fs[0, 1:].tolist() == [1.0, 1.0, 1.0, 0.0]
    fs, fi, fc = ref_fuse(sa, i, [1, 1], "sum", 60.0, "minmax", "floor", 5)     # the floor under minmax is 0: nothing changes
    assert fi[0].tolist() == [T, A1, A2, B1, B2] and fs[0, 1:].tolist() == [1.0, 1.0, 1.0, 0.0]
    # a repeated id inside one list: only its lowest position counts, for the score, the rank, the count and the statistics
    rs, ri = _two([1.0, 5.0, 0.5], [1.0, 0.375, 0.25], ia=(A1, A1, T))
    fs, fi, fc = ref_fuse(rs, ri, [1, 1], "sum", 60.0, "none", "zero", 4)
    assert fi[0].tolist() == [A1, B1, T, B2] and fs[0].tolist() == [1.0, 1.0, 0.875, 0.25] and fc[0].tolist() == [1, 1, 2, 1]
    fs, fi, fc = ref_fuse(rs, ri, [1, 1], "rrf", 60.0, "none", "zero", 4)
    assert fi[0].tolist() == [T, A1, B1, B2] and _bits(fs[0, 1]) == _bits(one / F(61)) and fc[0].tolist() == [2, 1, 1, 1]
    fs, fi, fc = ref_fuse(rs, ri, [1, 1], "sum", 60.0, "minmax", "zero", 4)     # A's range is [0.5, 1], not [0.5, 5]
    assert fi[0].tolist() == [A1, B1, T, B2] and _bits(fs[0, 2]) == _bits(F(0) + F(0.125) / F(0.75))
    # a hole in the middle keeps its rank: t stays third in A
    hs, hi = _two([1.0, 9.0, 0.5], [1.0, 0.375, 0.25], ia=(A1, -1, T))
    fs, fi, fc = ref_fuse(hs, hi, [1, 1], "rrf", 60.0, "none", "zero", 5)
    assert fi[0].tolist() == [T, A1, B1, B2, -1] and _bits(fs[0, 0]) == _bits(one / F(63) + one / F(62))
    # a present -inf entry is a hole: t is held by A alone, and B's least score is 0.25, not -inf
    ns, ni = _two([1.0, 0.75, 0.5], [1.0, -np.inf, 0.25])
    fs, fi, fc = ref_fuse(ns, ni, [1, 1], "sum", 60.0, "none", "floor", 5)
    assert fi[0].tolist() == [B1, A1, A2, T, B2] and fs[0].tolist() == [1.5, 1.25, 1.0, 0.75, 0.75] and fc[0].tolist() == [1, 1, 1, 1, 1]
    for bad in (np.inf, np.nan):
        ns[1, 0, 1] = bad
        assert ref_fuse(ns, ni, [1, 1], "rrf", 60.0, "none", "zero", 5)[2][0].tolist() == [1, 1, 1, 1, 1]
    # -0.0: a sum starts at +0.0 and cannot return -0.0; a maximum can, ranks as +0.0 and keeps its bits; a list with no valid entry
    # contributes nothing, even under the floor
    zs, zi = _two([-0.0, 0.0, -0.0], [np.nan, np.nan, np.nan], ia=(3, 2, 1), ib=(-1, 5, 6))
    fs, fi, fc = ref_fuse(zs, zi, [1, 1], "sum", 60.0, "none", "floor", 4)
    assert fi[0].tolist() == [1, 2, 3, -1] and np.signbit(fs[0, :3]).tolist() == [False, False, False]
    fs, fi, fc = ref_fuse(zs, zi, [1, 1], "max", 60.0, "none", "zero", 4)
    assert fi[0].tolist() == [1, 2, 3, -1] and np.signbit(fs[0, :3]).tolist() == [True, False, True]
    assert ref_fuse(zs[1:], zi[1:], [1], "sum", 60.0, "minmax", "floor", 2)[1].tolist() == [[-1, -1]]


def _unit(x):
    return (x / np.linalg.norm(x, axis=-1, keepdims=True)).astype(F)


def np_search(Q, G, k):
    """Top-k of Q @ G^T in float32 by (score desc, id asc), NumPy only: (scores f32 [Bq,k], idx i64 [Bq,k])."""
    S = (Q.astype(F) @ G.astype(F).T).astype(F)
    s, i = np.empty((S.shape[0], k), F), np.empty((S.shape[0], k), np.int64)
    for b in range(S.shape[0]):
        o = np.lexsort((np.arange(S.shape[1]), -S[b]))[:k]
        s[b], i[b] = S[b, o], o
    return s, i


def test_fused_views_find_the_target_more_often_than_the_best_view():
    """What the method is for, on the restatement alone (the GPU kernel inherits it through bitwise equality). 3 000 unit rows, C = 64,
    seed 3; 300 requests, each with a planted target row; three views per request, each the target plus 0.30 x standard-normal noise per
    channel (independent per view), normalised; every view searched exactly at k_each = 50. Recall@1 of the three single views:
    0.3633, 0.3533, 0.3133; of their RRF fusion (c = 60, weights 1): 0.8833. (A wrong row that one view's noise lifts to the top is far
    down in the other two lists; the target is near the top of all three.)"""
    from cor_amd.retrieval import recall_at_k
    rng = np.random.default_rng(3)
    G = _unit(rng.standard_normal((3000, 64)))
    targets = rng.choice(3000, 300, replace=False)
    views = [_unit(G[targets] + F(0.30) * rng.standard_normal((300, 64)).astype(F)) for _ in range(3)]
    lists = [np_search(v, G, 50) for v in views]
    single = [recall_at_k(torch.from_numpy(i), targets.tolist(), ks=(1,))[1] for _, i in lists]
    fs, fi, fc = ref_fuse(np.stack([s for s, _ in lists]), np.stack([i for _, i in lists]), [1, 1, 1], "rrf", 60.0, "none", "zero", 10)
    fused = recall_at_k(torch.from_numpy(fi), targets.tolist(), ks=(1,))[1]
    print(f"Recall@1: views {single}, RRF {fused}")
    assert fused > max(single)

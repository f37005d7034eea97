"""CPU-side checks (run under -m "not gpu") of the query expansion's host layers: the export of cor_expand_queries, its argument checks (all
made before any HIP call), the Python validation, the no-CPU-path rule, and the NumPy restatement of the definition that
tests/test_gpu_expand.py compares the kernel with, itself checked against an fp64 evaluation."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ref_expand(Q, query_weight, segments, scores, idx, m, alpha, normalize):
    """The definition of cor_expand_queries (include/cor_amd.h) restated with elementwise np.float32 operations in the stated order.
    Q f32 [Bq,C] or None, segments [(rows f32 [n,C]: the stored values already widened, offset)], scores f32 / idx i64 [Bq,kin]
    -> f32 [Bq,C]. Never calls the code under test."""
    f = np.float32
    Bq = idx.shape[0]
    C = Q.shape[1] if Q is not None else segments[0][0].shape[1]
    out = np.zeros((Bq, C), f)
    for b in range(Bq):
        v = f(query_weight) * Q[b].astype(f) if query_weight != 0 else np.zeros(C, f)
        for j in range(m):
            i, row = int(idx[b, j]), None
            for rows, off in segments:
                if off <= i < off + rows.shape[0]:
                    row = rows[i - off]
                    break
            if row is None:
                continue
            t = f(scores[b, j]) if scores[b, j] > 0 else f(0)
            w = f(1)
            for _ in range(alpha):
                w = f(w * t)
            v = v + (w * row)
        if normalize:
            s = np.zeros(256, f)
            s[:C] = v * v
            h = 128
            while h >= 1:
                s[:h] = s[:h] + s[h:2 * h]
                h //= 2
            v = v / max(np.sqrt(s[0]), f(1e-12))
        assert v.dtype == f
        out[b] = v
    return out


def to_dtype(x, dtype):
    """f32 ndarray -> torch CPU tensor of `dtype` (round to nearest even for the 16-bit forms)."""
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype)


def test_library_exports_the_expand_symbol():
    from cor_amd import _native
    lib = _native.load()
    hdr = open(os.path.join(ROOT, "include", "cor_amd.h")).read()
    proto = re.search(r"^int\s+cor_expand_queries\s*\(([^)]*)\)\s*;", hdr, flags=re.M | re.S)
    assert proto, "cor_expand_queries is not declared in include/cor_amd.h"
    assert len(proto.group(1).split(",")) == 18 == len(_native.SIGNATURES["cor_expand_queries"])
    assert hasattr(lib, "cor_expand_queries") and lib.cor_expand_queries.restype is _native._i
    assert re.search(r"^#define\s+COR_EXPAND_SEGMAX\s+16\b", hdr, flags=re.M) and _native.EXPAND_SEGMAX == 16


def test_expand_argument_errors_need_no_gpu():
    """Every argument check comes before any HIP call, so each error comes back on a machine without a device."""
    from cor_amd import _native
    lib = _native.load()
    E, N = _native.EINVAL, _native.ENOSUPPORT
    buf = torch.zeros(64, dtype=torch.int64)
    p = buf.data_ptr()

    def call(Q=p, qw=1.0, rows=(p,), offs=(0,), ns=(10,), dts=(_native.F32,), nseg=None, arrays=True, scores=p, idx=p, Bq=1, kin=4, m=4,
             C=256, alpha=3, normalize=1, out=p, odt=_native.F32):
        n = len(rows) if nseg is None else nseg
        a = (ctypes.c_void_p * max(len(rows), 1))(*rows)
        b = (ctypes.c_longlong * max(len(rows), 1))(*offs)
        c = (ctypes.c_int * max(len(rows), 1))(*ns)
        d = (ctypes.c_int * max(len(rows), 1))(*dts)
        if not arrays:
            a = b = c = d = None
        return lib.cor_expand_queries(Q, qw, a, b, c, d, n, scores, idx, Bq, kin, m, C, alpha, normalize, out, odt, None)

    # COR_EINVAL
    assert call(scores=None) == E and call(idx=None) == E and call(out=None) == E and call(arrays=False) == E
    assert call(Bq=-1) == E and call(kin=0) == E and call(m=0) == E and call(m=5) == E          # m > kin
    assert call(alpha=-1) == E and call(alpha=9) == E and call(nseg=-1) == E
    assert call(ns=(-1,)) == E and call(rows=(None,)) == E                                     # a null segment that has rows
    assert call(odt=3) == E and call(odt=-1) == E
    assert call(Q=None) == E and call(Q=None, qw=0.5) == E
    # COR_ENOSUPPORT
    assert call(kin=300, m=257) == N
    assert call(rows=(p,) * 17, offs=tuple(range(0, 170, 10)), ns=(10,) * 17, dts=(0,) * 17) == N
    assert call(C=272) == N and call(C=24) == N and call(C=8) == N
    assert call(dts=(3,)) == N and call(dts=(-1,)) == N
    # legal without a device: no queries; with them, no segments at all is legal too (decided by the same checks)
    assert call(Bq=0) == 0 and call(Bq=0, Q=None, qw=0.0) == 0 and call(Bq=0, rows=(), offs=(), ns=(), dts=(), arrays=False) == 0
    assert call(Bq=0, rows=(None,), ns=(0,)) == 0 and call(Bq=0, alpha=0) == 0 and call(Bq=0, alpha=8, kin=256, m=256, C=16) == 0
    for dt in (_native.F32, _native.BF16, _native.F16):
        assert call(Bq=0, dts=(dt,), odt=dt) == 0
    assert call(Bq=0, rows=(p,) * 16, offs=tuple(range(0, 160, 10)), ns=(10,) * 16, dts=(0, 1, 2, 0) * 4) == 0


def _cpu_shard(rows, offset=0):
    """A GalleryShard lives in GPU memory and its constructor says so; the methods under test only read rows and offset."""
    from cor_amd.retrieval import GalleryShard
    sh = GalleryShard.__new__(GalleryShard)
    sh.rows, sh.offset, sh.labels, sh.groups = rows, offset, None, None
    return sh


def test_expand_validation_and_no_cpu_path():
    from cor_amd import ops
    from cor_amd.retrieval import GallerySet
    Q, G = torch.zeros((2, 16)), torch.zeros((5, 16))
    s, i = torch.ones((2, 3)), torch.zeros((2, 3), dtype=torch.int64)
    for call in (lambda: ops.expand_queries(Q, [(G, 0)], s, i, 3),
                 lambda: ops.expand_queries(None, [(G.to(torch.bfloat16), 7)], s, i, 2, query_weight=0.0, out_dtype=torch.float16),
                 lambda: ops.expand_queries(Q, [], s, i, 1),
                 lambda: _cpu_shard(G).expand(Q, s, i, 3),
                 lambda: _cpu_shard(G, 100).expand(None, s, i, 3, query_weight=0.0),
                 lambda: GallerySet().expand(Q, s, i, 3)):
        with pytest.raises(RuntimeError):                              # valid arguments, CPU tensors: there is no CPU path
            call()
    bad = [dict(m=0), dict(m=4), dict(m=-1),                           # m > kin
           dict(alpha=-1), dict(alpha=9), dict(alpha=1.5),
           dict(out_dtype=torch.float64), dict(out_dtype=torch.int32),
           dict(segments=[(G[:1], n) for n in range(17)]),             # 17 segments
           dict(segments=[(G, 0), (G, 3)]),                            # overlapping id ranges
           dict(segments=[(torch.zeros((5, 32)), 0)]), dict(segments=[(G.double(), 0)]), dict(segments=[(G[0], 0)]),
           dict(scores=s.double()), dict(scores=s[0]), dict(scores=s[:, :0]), dict(idx=i.to(torch.int32)), dict(idx=i[:1]),
           dict(Q=Q.double()), dict(Q=Q[:1]), dict(Q=Q[0]), dict(Q=None), dict(Q=torch.zeros((2, 24))), dict(Q=torch.zeros((2, 272))),
           dict(out=torch.zeros((2, 8))), dict(out=torch.zeros((2, 16), dtype=torch.float16))]
    for kw in bad:
        args = dict(Q=Q, segments=[(G, 0)], scores=s, idx=i, m=3)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.expand_queries(**args)
    with pytest.raises(ValueError, match="17 segments"):
        ops.expand_queries(Q, [(G[:1], n) for n in range(17)], s, i, 3)
    with pytest.raises(ValueError):
        ops.expand_queries(None, [], s, i, 3, query_weight=0.0)        # no width to be had
    with pytest.raises(ValueError):
        _cpu_shard(G).expand(Q, s, i, 4)


class _Never:
    """A gallery that must not be touched."""

    def search(self, *a, **kw):
        raise AssertionError("searched before the arguments were validated")

    expand = search


def test_expanded_search_and_augmented_validate_first():
    from cor_amd import retrieval
    for kw in (dict(k=0, m=5), dict(k=257, m=5), dict(k=10, m=0), dict(k=10, m=257), dict(k=10, m=5, rounds=0)):
        with pytest.raises(ValueError):
            retrieval.expanded_search(None, _Never(), **kw)
    sh = _cpu_shard(torch.zeros((5, 16)))
    for kw in (dict(m=0), dict(m=257), dict(m=3, batch=0)):
        with pytest.raises(ValueError):
            sh.augmented(neighbours=_Never(), **kw)


def test_expanded_search_composes_search_and_expand():
    """The plumbing, with a stub gallery: m for the expansion searches, k for the last one, the keywords for every search, each round
    expanding the query of the round before."""
    from cor_amd import retrieval
    calls = []

    class Gallery:
        def search(self, q, k, **kw):
            calls.append(("search", q, k, kw))
            return f"s({q})", f"i({q})"

        def expand(self, q, s, i, m, **kw):
            calls.append(("expand", q, s, i, m, kw))
            return q + "'"

    out = retrieval.expanded_search("q", Gallery(), 10, 5, alpha=2, query_weight=0.5, rounds=2, query_labels="ql", mode="ne")
    kw, ex = dict(query_labels="ql", mode="ne"), dict(alpha=2, query_weight=0.5)
    assert out == ("s(q'')", "i(q'')", "q''")
    assert calls == [("search", "q", 5, kw), ("expand", "q", "s(q)", "i(q)", 5, ex), ("search", "q'", 5, kw),
                     ("expand", "q'", "s(q')", "i(q')", 5, ex), ("search", "q''", 10, kw)]


def test_restatement_agrees_with_fp64():
    """The NumPy restatement against the same formula in fp64, C = 256, m = 10, within 4 (m + 9) 2^-24 relative per component: m + 1
    rounded products and m sums give a component of v at most (2m + 1) u (u = 2^-24), its square twice that plus one, the 8 tree levels
    8 more; the square root halves what the norm carries, the division adds one: below 2 (2m + 1) + 7 < 4 (m + 9) units. The bound is
    relative to the component, so it can only hold where no sum cancels: weights (scores) positive as the issue asks, and row and
    query values non-negative."""
    rng = np.random.default_rng(5)
    C, m, Ng, Bq = 256, 10, 64, 24
    G = np.abs(rng.standard_normal((Ng, C))).astype(np.float32)
    G /= np.linalg.norm(G, axis=1, keepdims=True)
    Q = np.abs(rng.standard_normal((Bq, C))).astype(np.float32)
    idx = rng.integers(0, Ng, (Bq, m)).astype(np.int64) + 1000
    scores = rng.uniform(0.1, 1.0, (Bq, m)).astype(np.float32)
    bound = 4 * (m + 9) * 2.0 ** -24
    for alpha, qw in ((0, 1.0), (1, 0.5), (3, 1.0), (8, 0.0)):
        got = ref_expand(Q, qw, [(G, 1000)], scores, idx, m, alpha, True)
        v = np.float64(np.float32(qw)) * Q.astype(np.float64) + np.einsum("bj,bjc->bc", scores.astype(np.float64) ** alpha, G.astype(np.float64)[idx - 1000])
        want = v / np.sqrt((v * v).sum(1, keepdims=True))
        rel = np.abs(got - want) / np.abs(want)
        print(f"alpha={alpha} qw={qw}: max relative error {rel.max():.3e} (bound {bound:.3e})")
        assert (want > 0).all() and rel.max() <= bound


def test_restatement_edge_cases():
    """Hand-checkable cases of the restatement: a missing entry's NaN score is not used, a negative / -0.0 score weighs +0 but the
    addition still happens, a repeat adds twice, nothing to sum gives zeros, C = 48 pads the tree with +0."""
    G = np.zeros((4, 48), np.float32)
    G[0, 0], G[1, 1], G[2, 2] = 3, 4, -1
    idx = np.array([[0, 1, -1, 99], [0, 0, 2, 2], [7, -1, 2 ** 40, -2 ** 63], [2, 1, 1, 0]], np.int64)
    sc = np.array([[1, 1, np.nan, -np.inf], [1, 1, -2, -0.0], [np.nan] * 4, [0.5, 0.5, 0.5, 0.5]], np.float32)
    out = ref_expand(None, 0.0, [(G, 0)], sc, idx, 4, 1, True)
    assert out[0, 0] == np.float32(0.6) and out[0, 1] == np.float32(0.8) and not np.isnan(out).any()
    assert out[1, 0] == 1 and out[1, 2] == 0 and not np.signbit(out[1, 2])     # +0 + (+0 * -1) = +0
    assert not out[2].any()
    raw = ref_expand(None, 0.0, [(G, 0)], sc, idx, 3, 2, False)
    assert raw[3, 2] == -0.25 and raw[3, 1] == 2.0 and raw[3, 0] == 0            # m = 3: the fourth entry is not used
    one = np.ones((1, 256), np.float32)
    assert np.array_equal(ref_expand(one, 0.5, [], sc[:1], idx[:1], 1, 0, True), np.full((1, 256), 0.0625, np.float32))

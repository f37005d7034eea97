"""CPU-side checks of the list stages over int8 galleries (cor_dequantize_rows_i8, cor_rescore_topk_i8, cor_expand_queries_sq and their
Python fronts): the exports, every argument error with its code through ctypes and without a device, the Python fronts' ValueErrors, the
no-CPU-path rule, and the restatements of tests/i8_list_refs.py against Python integers and float64 on tiny shapes."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests.i8_list_refs import RefRescore, ref_dequantize, ref_expand_sq
from tests.i8_refs import F, ref_quantize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"cor_dequantize_rows_i8": ("int", 7), "cor_rescore_i8_workspace_bytes": ("long", 3), "cor_rescore_topk_i8": ("int", 15),
       "cor_expand_queries_sq": ("int", 19)}


def test_library_exports_the_four_symbols_and_the_dtype():
    from cor_amd import _native
    lib = _native.load()
    hdr = open(os.path.join(ROOT, "include", "cor_amd.h")).read()
    for name, (ret, nargs) in NEW.items():
        proto = re.search(rf"^{ret}\s+{name}\s*\(([^)]*)\)\s*;", hdr, flags=re.M | re.S)
        assert proto, f"{name} is not declared in include/cor_amd.h"
        assert len(proto.group(1).split(",")) == nargs == len(_native.SIGNATURES[name]), name
        assert getattr(lib, name).restype is (_native._l if ret == "long" else _native._i)
    assert list(_native.SIGNATURES).index("cor_expand_queries") < list(_native.SIGNATURES).index("cor_dequantize_rows_i8")
    order = [n for n in _native.SIGNATURES if n in NEW]
    assert order == list(NEW)                                                                 # header order
    assert re.search(r"COR_I8\s*=\s*4\b", hdr) and _native.I8 == 4


def test_dequantize_argument_errors_need_no_gpu():
    from cor_amd import _native
    lib = _native.load()
    E, N = _native.EINVAL, _native.ENOSUPPORT
    buf = torch.zeros(64, dtype=torch.int64)
    p = buf.data_ptr()
    assert p % 16 == 0

    def call(q=p, scale=p, n=4, C=32, X=p, dt=_native.F32):
        return lib.cor_dequantize_rows_i8(q, scale, n, C, X, dt, None)

    assert call(q=None) == E and call(scale=None) == E and call(X=None) == E and call(n=-1) == E and call(C=0) == E and call(C=-16) == E
    assert call(C=272) == N and call(C=24) == N and call(C=8) == N
    assert call(dt=_native.BF16X3) == N and call(dt=_native.I8) == N and call(dt=-1) == N
    assert call(q=p + 8) == E and call(X=p + 4) == E and call(scale=p + 2) == E             # alignment, after the shape checks
    assert call(C=24, q=p + 8) == N                                                            # ... as in cor_quantize_rows_i8
    for dt in (_native.F32, _native.BF16, _native.F16):
        assert call(n=0, dt=dt) == 0                                                           # a successful no-op
    assert call(n=0, scale=p + 4) == 0


def test_rescore_i8_argument_errors_need_no_gpu():
    from cor_amd import _native
    lib = _native.load()
    E, N = _native.EINVAL, _native.ENOSUPPORT
    buf = torch.zeros(64, dtype=torch.int64)
    p = buf.data_ptr()

    def call(Q=p, G=p, gs=p, Bq=1, Ng=10, C=256, off=0, cand=p, kin=4, k=2, os_=p, oi=p, op=None):
        return lib.cor_rescore_topk_i8(Q, G, gs, Bq, Ng, C, off, cand, kin, k, os_, oi, op, None, None)

    assert call(Q=None) == E and call(cand=None) == E and call(os_=None) == E and call(oi=None) == E
    assert call(G=None) == E and call(gs=None) == E and call(Ng=-1) == E and call(C=0) == E
    assert call(Bq=-1) == E and call(kin=0) == E and call(k=0) == E and call(k=257) == E
    assert call(kin=4097) == N and call(C=272) == N and call(C=24) == N and call(C=8) == N
    assert call(k=0, kin=4097) == E and call(kin=4097, C=24, Q=None) == E                     # the order of cor_rescore_topk's checks
    assert call(Bq=0) == 0 and call(Bq=0, G=None, gs=None, Ng=0) == 0 and call(Bq=0, kin=4096, k=256, C=16) == 0
    w = lib.cor_rescore_i8_workspace_bytes
    assert w(5, 100, 10) == 0 and w(0, 1, 1) == 0 and w(5, 4096, 256) == 0
    assert w(-1, 4, 2) == E and w(1, 0, 2) == E and w(1, 4, 0) == E and w(1, 4, 257) == E and w(1, 4097, 2) == N
    # the float entry point keeps refusing the int8 dtype
    assert lib.cor_rescore_topk(p, p, _native.I8, 1, 10, 256, 0, p, 4, 2, p, p, None, None, None) == N


def test_expand_sq_argument_errors_need_no_gpu():
    from cor_amd import _native
    lib = _native.load()
    E, N = _native.EINVAL, _native.ENOSUPPORT
    buf = torch.zeros(64, dtype=torch.int64)
    p = buf.data_ptr()
    I8 = _native.I8

    def arrays(rows, scales, offs, ns, dts):
        n = max(len(rows), 1)
        return ((ctypes.c_void_p * n)(*rows), (ctypes.c_void_p * n)(*scales), (ctypes.c_longlong * n)(*offs), (ctypes.c_int * n)(*ns),
                (ctypes.c_int * n)(*dts))

    def call(Q=p, qw=1.0, rows=(p,), scales=(p,), offs=(0,), ns=(10,), dts=(I8,), nseg=None, arr=True, no_scales=False, scores=p, idx=p, Bq=1,
             kin=4, m=4, C=256, alpha=3, normalize=1, out=p, odt=_native.F32, old=False):
        n = len(rows) if nseg is None else nseg
        a, sc, b, c, d = arrays(rows, scales, offs, ns, dts) if arr else (None,) * 5
        if old:
            return lib.cor_expand_queries(Q, qw, a, b, c, d, n, scores, idx, Bq, kin, m, C, alpha, normalize, out, odt, None)
        return lib.cor_expand_queries_sq(Q, qw, a, None if no_scales else sc, b, c, d, n, scores, idx, Bq, kin, m, C, alpha, normalize, out, odt,
                                         None)

    # COR_EINVAL: those of cor_expand_queries
    assert call(scores=None) == E and call(idx=None) == E and call(out=None) == E and call(arr=False) == E
    assert call(Bq=-1) == E and call(kin=0) == E and call(m=0) == E and call(m=5) == E
    assert call(alpha=-1) == E and call(alpha=9) == E and call(nseg=-1) == E and call(C=0) == E
    assert call(ns=(-1,)) == E and call(rows=(None,)) == E
    assert call(odt=3) == E and call(odt=I8) == E and call(odt=-1) == E
    assert call(Q=None) == E and call(Q=None, qw=0.5) == E
    # ... and the scales of an int8 segment that has rows
    assert call(scales=(None,)) == E and call(no_scales=True) == E
    assert call(rows=(p, p), scales=(p, None), offs=(0, 10), ns=(10, 10), dts=(_native.F32, I8)) == E
    assert call(Bq=0, scales=(None,)) == E                                                     # decided before Bq == 0 returns
    # COR_ENOSUPPORT
    assert call(kin=300, m=257) == N
    assert call(rows=(p,) * 17, scales=(p,) * 17, offs=tuple(range(0, 170, 10)), ns=(10,) * 17, dts=(I8,) * 17) == N
    assert call(C=272) == N and call(C=24) == N and call(C=8) == N
    assert call(dts=(3,)) == N and call(dts=(5,)) == N and call(dts=(-1,)) == N
    # legal without a device
    assert call(Bq=0) == 0 and call(Bq=0, Q=None, qw=0.0) == 0 and call(Bq=0, rows=(), scales=(), offs=(), ns=(), dts=(), arr=False) == 0
    assert call(Bq=0, rows=(None,), scales=(None,), ns=(0,)) == 0 and call(Bq=0, alpha=8, kin=256, m=256, C=16) == 0
    assert call(Bq=0, dts=(_native.F32,), scales=(None,)) == 0 and call(Bq=0, dts=(_native.BF16,), no_scales=True) == 0   # ignored for float segments
    assert call(Bq=0, rows=(p,) * 16, scales=(p,) * 16, offs=tuple(range(0, 160, 10)), ns=(10,) * 16, dts=(0, 1, 2, I8) * 4) == 0
    # cor_expand_queries itself keeps refusing the int8 dtype, exactly as any unknown one
    assert call(old=True, Bq=0) == N and call(old=True) == N and call(old=True, dts=(3,)) == N and call(old=True, Bq=0, dts=(_native.F32,)) == 0


def _cpu_qshard(q, scale, offset=0):
    from cor_amd import retrieval
    sh = retrieval.QuantizedShard.__new__(retrieval.QuantizedShard)                 # the constructor refuses CPU tensors
    sh.rows, sh.scales, sh.offset, sh.labels, sh.groups = q, scale, offset, None, None
    g = sh.gallery()
    assert type(g) is retrieval.QuantizedGallery and g.rows is q and g.scales is scale and g.gallery() is g
    assert not hasattr(sh, "rescore") and not hasattr(sh, "expand") and not hasattr(sh, "rerank") and not hasattr(sh, "augmented")
    return g


def test_python_validation_and_no_cpu_path():
    from cor_amd import ops, retrieval
    Q = torch.zeros((2, 32))
    q, sc = torch.zeros((5, 32), dtype=torch.int8), torch.ones(5)
    cand = torch.zeros((2, 4), dtype=torch.int64)
    s = torch.zeros((2, 4))
    V = ValueError
    # dequantize_rows_i8
    for bad in (lambda: ops.dequantize_rows_i8(q.float(), sc), lambda: ops.dequantize_rows_i8(q[0], sc), lambda: ops.dequantize_rows_i8(q, sc[:4]),
                lambda: ops.dequantize_rows_i8(q, sc.double()), lambda: ops.dequantize_rows_i8(torch.zeros((5, 40), dtype=torch.int8), sc),
                lambda: ops.dequantize_rows_i8(torch.zeros((5, 512), dtype=torch.int8), sc), lambda: ops.dequantize_rows_i8(q, sc, out_dtype=torch.float64),
                lambda: ops.dequantize_rows_i8(q, sc, out=torch.zeros((5, 16))), lambda: ops.dequantize_rows_i8(q, sc, out=torch.zeros((5, 32), dtype=torch.float16))):
        with pytest.raises(V):
            bad()
    # rescore_topk_i8
    for bad in (lambda: ops.rescore_topk_i8(Q, q, sc, cand, 0), lambda: ops.rescore_topk_i8(Q, q, sc, cand, 257), lambda: ops.rescore_topk_i8(Q[0], q, sc, cand, 2),
                lambda: ops.rescore_topk_i8(Q, q[:, :16], sc, cand, 2), lambda: ops.rescore_topk_i8(Q.double(), q, sc, cand, 2),
                lambda: ops.rescore_topk_i8(Q, q.float(), sc, cand, 2), lambda: ops.rescore_topk_i8(Q, q, sc[:4], cand, 2),
                lambda: ops.rescore_topk_i8(Q, q, sc.double(), cand, 2), lambda: ops.rescore_topk_i8(Q, q, sc, cand.int(), 2),
                lambda: ops.rescore_topk_i8(Q, q, sc, cand[:1], 2), lambda: ops.rescore_topk_i8(Q, q, sc, cand[:, :0], 2), lambda: ops.rescore_topk_i8(Q, q, sc, cand[0], 2),
                lambda: ops.rescore_topk_i8(torch.zeros((2, 40)), torch.zeros((5, 40), dtype=torch.int8), sc, cand, 2)):
        with pytest.raises(V):
            bad()
    # expand_queries with int8 segments
    for bad in (lambda: ops.expand_queries(Q, [(q, sc[:4], 0)], s, cand, 2), lambda: ops.expand_queries(Q, [(q, sc.double(), 0)], s, cand, 2),
                lambda: ops.expand_queries(Q, [(q.float(), sc, 0)], s, cand, 2), lambda: ops.expand_queries(Q, [(q, 0)], s, cand, 2),
                lambda: ops.expand_queries(Q, [(q[:, :16], sc, 0)], s, cand, 2), lambda: ops.expand_queries(Q, [(q, sc, 0), (q, sc, 3)], s, cand, 2),
                lambda: ops.expand_queries(Q, [(q, sc, 0), (Q, 4)], s, cand, 2), lambda: ops.expand_queries(Q, [(q, sc, sc, 0)], s, cand, 2),
                lambda: ops.expand_queries(Q, [(q, sc, 10 * n) for n in range(17)], s, cand, 2), lambda: ops.expand_queries(None, [(q, sc, 0)], s, cand, 2)):
        with pytest.raises(V):
            bad()
    # valid arguments on the CPU: there is no CPU path
    G = "GPU only"
    with pytest.raises(RuntimeError, match=G):
        ops.dequantize_rows_i8(q, sc)
    with pytest.raises(RuntimeError, match=G):
        ops.rescore_topk_i8(Q, q, sc, cand, 2)
    with pytest.raises(RuntimeError, match=G):
        ops.expand_queries(Q, [(q, sc, 0)], s, cand, 2)
    with pytest.raises(RuntimeError, match=G):
        ops.expand_queries(None, [(q, sc, 0), (Q, 5)], s, cand, 2, query_weight=0.0)
    sh = _cpu_qshard(q, sc)
    with pytest.raises(RuntimeError, match=G):
        sh.rescore(Q, cand)
    with pytest.raises(RuntimeError, match=G):
        sh.expand(Q, s, cand, 2)
    with pytest.raises(RuntimeError, match=G):
        sh.dequantized()
    with pytest.raises(RuntimeError, match=G):
        sh.neighbour_graph(2)
    with pytest.raises(RuntimeError, match=G):
        sh.augmented(2)
    with pytest.raises(V):
        sh.rescore(Q, cand[0])
    with pytest.raises(V):
        sh.neighbour_graph(0)
    with pytest.raises(V):
        sh.neighbour_graph(2, batch=0)
    with pytest.raises(V):
        sh.augmented(0)
    with pytest.raises(V):
        sh.augmented(300)
    graph = retrieval.NeighbourGraph(2, [7], [5], [torch.zeros((5, 2), dtype=torch.int64)], [torch.zeros(5)])
    with pytest.raises(V, match="build a new graph"):
        sh.rerank(s, cand, graph)                                                              # built from other segments
    with pytest.raises(V, match="build a new graph"):
        retrieval.GallerySet([]).rerank(s, cand, graph)


def test_gallery_shard_augmented_expands_over_its_own_rows_for_a_search_only_neighbour():
    """GalleryShard.augmented(neighbours=QuantizedShard) expands over the float shard's own rows; with a QuantizedGallery, which expands,
    over the gallery's."""
    from cor_amd import retrieval
    calls = []

    class Fine(retrieval.GalleryShard):
        def __init__(self):
            self.rows, self.offset, self.labels, self.groups = torch.zeros((4, 32)), 0, None, None

        def expand(self, *a, **kw):
            calls.append("fine")

    def neighbour(base):
        class Quant(base):
            def __init__(self):
                pass

            def search(self, q, k):
                return torch.zeros((q.shape[0], k)), torch.zeros((q.shape[0], k), dtype=torch.int64)
        return Quant()

    real = retrieval.GalleryShard.__init__
    gallery_expand = retrieval.QuantizedGallery.expand
    try:
        retrieval.GalleryShard.__init__ = lambda self, rows, **kw: None                       # the result shard is not under test
        retrieval.QuantizedGallery.expand = lambda self, *a, **kw: calls.append("int8")
        Fine().augmented(2, neighbours=neighbour(retrieval.QuantizedShard))
        Fine().augmented(2, neighbours=neighbour(retrieval.QuantizedGallery))
    finally:
        retrieval.GalleryShard.__init__ = real
        retrieval.QuantizedGallery.expand = gallery_expand
    assert calls == ["fine", "int8"]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_restatements_against_python_integers_and_float64(seed):
    rng = np.random.default_rng(seed)
    n, C, Bq = 7, 16, 3
    X = rng.standard_normal((n, C)).astype(F)
    X[2] = 0
    q, scale = ref_quantize(X)
    # dequantise: int8 (8 bits) times fp32 (24 bits) is exact in float64, so rounding that product once is the one fp32 multiply
    d32 = ref_dequantize(q, scale).numpy()
    for g in range(n):
        for c in range(C):
            assert d32[g, c] == np.float32(float(int(q[g, c])) * float(scale[g]))
    assert torch.equal(ref_dequantize(q, scale, torch.float16), torch.from_numpy(d32).to(torch.float16))
    # rescore: Python integers for the dot product, float64 products (48 bits: exact) rounded once each
    Q = rng.standard_normal((Bq, C)).astype(F)
    qq, qs = ref_quantize(Q)
    off = 2 ** 33 + 5
    cand = np.array([[off + 3, off + 1, off + 3, -1, off + 6, off + 7, off - 1, off + 0],
                     [off + 2, off + 2, off + 2, off + 2, off + 2, off + 2, off + 2, off + 2],
                     [5, 6, -2 ** 63, 2 ** 63 - 1, 1, 2, 3, 4]], dtype=np.int64)
    s, i, p = RefRescore(Q, q, scale, cand, off).top(8)
    for b in range(Bq):
        want = []
        for j, v in enumerate(int(x) for x in cand[b]):
            if off <= v < off + n and v not in [w[1] for w in want]:
                d = sum(int(a) * int(e) for a, e in zip(qq[b], q[v - off]))
                sc = np.float32(float(np.float32(float(d) * float(qs[b]))) * float(scale[v - off]))
                want.append((sc, v, j))
        want.sort(key=lambda t: (-float(t[0]), t[1]))
        assert [int(x) for x in i[b, :len(want)]] == [w[1] for w in want] and [int(x) for x in p[b, :len(want)]] == [w[2] for w in want]
        assert all(np.float32(a).tobytes() == np.float32(w[0]).tobytes() or (a == 0 and w[0] == 0) for a, w in zip(s[b].numpy(), want))
        assert (i[b, len(want):] == -1).all() and (p[b, len(want):] == -1).all() and torch.isinf(s[b, len(want):]).all()
    assert [len(l[0]) for l in RefRescore(Q, q, scale, cand, off).lists] == [4, 1, 0]
    # expand: the sum over an int8 segment is the sum over its dequantised values, whatever dtype stores them and however they are cut
    sc = rng.uniform(0.1, 1.0, (Bq, 5)).astype(F)
    idx = rng.integers(0, n, (Bq, 5)).astype(np.int64)
    one = ref_expand_sq(Q, 1.0, [(q, scale, 0)], sc, idx, 5, 3, True)
    flt = ref_expand_sq(Q, 1.0, [(torch.from_numpy(d32), 0)], sc, idx, 5, 3, True)
    cut = ref_expand_sq(Q, 1.0, [(q[4:], scale[4:], 4), (torch.from_numpy(d32[:4]), 0)], sc, idx, 5, 3, True)
    assert one.tobytes() == flt.tobytes() == cut.tobytes()
    acc = np.zeros(C, np.float64)
    for j in range(5):
        acc += float(sc[0, j]) ** 3 * d32[idx[0, j]].astype(np.float64)
    acc += Q[0]
    acc /= np.sqrt((acc * acc).sum())
    assert np.abs(one[0] - acc).max() < 1e-5

"""CPU-side check (run under -m "not gpu") that the seven entry points which take a table of gallery-row segments answer the same table
faults with the same codes in the same order: they share one check (cor_amd/csrc/segrows.h). Every fault is decided before any HIP call,
so no device is touched. The order include/cor_amd.h documents for each of them: null arrays (COR_EINVAL), the segment count
(COR_ENOSUPPORT, before any array is read), the entries (COR_EINVAL), then the call's limits and the dtypes (COR_ENOSUPPORT)."""
import ctypes

import pytest
import torch

ENTRY_POINTS = ["cor_expand_queries", "cor_expand_queries_sq", "cor_diversify_mmr", "cor_rerank_diffusion", "cor_kmeans_seed", "cor_kmeans_update",
                "cor_ivf_build"]


def _caller(name):
    """call(rows, scale, offs, ns, dts, nseg, arrays, scale_array, C) -> the return code of `name` over that table, every other argument valid"""
    from cor_amd import _native as nat
    lib = nat.load()
    buf = torch.zeros(64, dtype=torch.int64)
    p = buf.data_ptr()

    def call(rows=(p,), scale=(None,), offs=(0,), ns=(10,), dts=(nat.F32,), nseg=None, arrays=True, scale_array=True, C=64):
        n = len(rows) if nseg is None else nseg
        m = max(len(rows), 1)
        a, c, d, e = (ctypes.c_void_p * m)(*rows), (ctypes.c_longlong * m)(*offs), (ctypes.c_int * m)(*ns), (ctypes.c_int * m)(*dts)
        b = (ctypes.c_void_p * m)(*scale) if scale_array else None
        if not arrays:
            a = c = d = e = None
        assign = (ctypes.c_void_p * m)(*[p] * m)
        keep = (buf, assign)                                 # alive until the call returns
        if name == "cor_expand_queries":
            return lib.cor_expand_queries(p, 1.0, a, c, d, e, n, p, p, 1, 4, 4, C, 3, 1, p, nat.F32, None)
        if name == "cor_expand_queries_sq":
            return lib.cor_expand_queries_sq(p, 1.0, a, b, c, d, e, n, p, p, 1, 4, 4, C, 3, 1, p, nat.F32, None)
        if name == "cor_diversify_mmr":
            return lib.cor_diversify_mmr(a, b, c, d, e, n, p, p, 1, 4, C, 0.5, 0.9, 2, p, p, None, None, None)
        if name == "cor_rerank_diffusion":
            return lib.cor_rerank_diffusion(a, b, c, d, e, n, p, p, 1, 4, C, 2, 4, 3, 0.9, 5, 2, p, p, None, None)
        if name == "cor_kmeans_seed":
            return lib.cor_kmeans_seed(a, b, c, d, e, n, C, 4, 0, p, p, p, None)
        if name == "cor_kmeans_update":
            return lib.cor_kmeans_update(a, b, c, d, e, n, assign, None, C, 4, None, p, p, None, p, None)
        assert name == "cor_ivf_build" and keep
        return lib.cor_ivf_build(a, b, c, d, e, n, assign, C, 4, nat.F32, p, None, p, p, p, None)

    return nat, p, call


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_table_faults_and_their_precedence(name):
    nat, p, call = _caller(name)
    E, N = nat.EINVAL, nat.ENOSUPPORT
    # cor_expand_queries takes no scales: COR_I8 is no storage dtype of its table at all, and says so where the dtypes are looked at
    no_scales = N if name == "cor_expand_queries" else E
    # the faults, one at a time
    assert call(arrays=False) == E                                                       # a null array with nseg > 0
    assert call(nseg=17) == N                                                            # 17 segments, one-entry arrays: they are not read
    assert call(ns=(-1,)) == E                                                           # n < 0
    assert call(rows=(None,)) == E                                                       # a null row pointer with n > 0
    assert call(dts=(nat.I8,)) == no_scales and call(dts=(nat.I8,), scale_array=False) == no_scales   # an int8 segment without scales
    assert call(dts=(7,)) == N and call(dts=(nat.BF16X3,)) == N and call(dts=(-1,)) == N  # an unknown dtype
    # the order: null arrays, the count, the entries, the limits and dtypes
    assert call(arrays=False, nseg=17) == E
    assert call(nseg=17, ns=(-1,)) == N and call(nseg=17, rows=(None,)) == N and call(nseg=17, dts=(7,)) == N
    assert call(ns=(-1,), dts=(7,)) == E and call(rows=(None,), dts=(7,)) == E
    assert call(ns=(-1,), C=24) == E and call(rows=(None,), C=272) == E and call(dts=(nat.I8,), C=24) == no_scales
    assert call(C=24, dts=(7,)) == N
    # an empty segment needs no pointers, but its dtype is still looked at
    assert call(rows=(None,), ns=(0,), dts=(7,)) == N

"""CPU-side checks (run under -m "not gpu") of the cell-probing search's host layers: the exports of cor_ivf_build / cor_ivf_search and their
workspace queries and the argument order, every argument error and its precedence (all decided before any HIP call), the Python validation
and the no-CPU-path rule, the NumPy restatements tests/test_gpu_ivf.py compares the kernels with (tests/ivf_refs.py), and what the feature
is for: on a planted gallery a few probed cells find most of the exact neighbours while a fraction of the rows is scored."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests.cluster_refs import F, planted, ref_cluster
from tests.ivf_refs import recall, ref_exact, ref_ivf_build, ref_ivf_search

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _proto(name, ret="int"):
    hdr = open(os.path.join(ROOT, "include", "cor_amd.h")).read()
    m = re.search(rf"^{ret}\s+{name}\s*\(([^)]*)\)\s*;", hdr, flags=re.M | re.S)
    assert m, f"{name} is not declared in include/cor_amd.h"
    return [re.sub(r"[\s*]+", " ", a).strip().split(" ")[-1] for a in m.group(1).split(",")], hdr


def test_library_exports_the_ivf_symbols_in_the_documented_order():
    from cor_amd import _native
    lib = _native.load()
    names, hdr = _proto("cor_ivf_build")
    assert names == ["seg_rows", "seg_scale", "seg_offset", "seg_n", "seg_dtype", "nseg", "seg_assign", "C", "K", "dtype", "out_rows", "out_scale",
                     "out_ids", "out_cell_start", "workspace", "stream"]
    sig = _native.SIGNATURES["cor_ivf_build"]
    assert len(sig) == len(names) == 16 and all(sig[n] is _native._i for n in (5, 7, 8, 9)) and all(sig[n] is _native._p for n in (0, 6, 10, 15))
    names, _ = _proto("cor_ivf_search")
    assert names == ["Q", "rows", "scale", "dtype", "ids", "cell_start", "K", "C", "Bq", "probes", "nprobe", "k", "max_cell", "split", "out_scores",
                     "out_idx", "out_scanned", "workspace", "stream"]
    sig = _native.SIGNATURES["cor_ivf_search"]
    assert len(sig) == len(names) == 19 and all(sig[n] is _native._i for n in (3, 6, 7, 8, 10, 11, 12, 13))
    assert all(sig[n] is _native._p for n in (0, 1, 2, 4, 5, 9, 14, 15, 16, 17, 18))
    names, _ = _proto("cor_ivf_build_workspace_bytes", ret="long")
    assert names == ["n_total", "K", "C"] and _native.SIGNATURES["cor_ivf_build_workspace_bytes"] == [_native._l, _native._i, _native._i]
    names, _ = _proto("cor_ivf_search_workspace_bytes", ret="long")
    assert names == ["Bq", "K", "C", "nprobe", "k", "split"] and _native.SIGNATURES["cor_ivf_search_workspace_bytes"] == [_native._i] * 6
    for fn in ("cor_ivf_build", "cor_ivf_search"):
        assert hasattr(lib, fn) and getattr(lib, fn).restype is _native._i
    assert lib.cor_ivf_build_workspace_bytes.restype is _native._l and lib.cor_ivf_search_workspace_bytes.restype is _native._l
    assert re.search(r"^#define\s+COR_IVF_NPROBE_MAX\s+256\b", hdr, flags=re.M) and _native.IVF_NPROBE_MAX == 256


def _calls():
    from cor_amd import _native
    lib = _native.load()
    buf = torch.zeros(1024, dtype=torch.int64)
    p = (buf.data_ptr() + 255) // 256 * 256                                                   # 256-byte aligned host memory, never dereferenced

    def build(rows=(p,), scale=(None,), offs=(0,), ns=(10,), dts=(_native.F32,), nseg=None, arrays=True, scale_array=True, assign=(p,),
              assign_array=True, C=64, K=4, dtype=_native.F32, out_rows=p, out_scale=None, out_ids=p, out_cs=p, ws=p):
        n = len(rows) if nseg is None else nseg
        m = max(len(rows), 1)
        a = (ctypes.c_void_p * m)(*rows)
        b = (ctypes.c_void_p * m)(*scale) if scale_array else None
        c = (ctypes.c_longlong * m)(*offs)
        d = (ctypes.c_int * m)(*ns)
        e = (ctypes.c_int * m)(*dts)
        sa = (ctypes.c_void_p * m)(*assign) if assign_array else None
        table = (a, b, c, d, e) if arrays else (None, b, None, None, None)
        return lib.cor_ivf_build(*table, n, sa, C, K, dtype, out_rows, out_scale, out_ids, out_cs, ws, None)

    def search(Q=p, rows=p, scale=None, dtype=_native.F32, ids=p, cs=p, K=8, C=64, Bq=2, probes=p, nprobe=4, k=10, max_cell=100, split=0,
               out_s=p, out_i=p, out_n=None, ws=p):
        return lib.cor_ivf_search(Q, rows, scale, dtype, ids, cs, K, C, Bq, probes, nprobe, k, max_cell, split, out_s, out_i, out_n, ws, None)

    return _native, lib, p, build, search


def test_every_build_argument_error_comes_back_without_a_gpu():
    nat, lib, p, build, _ = _calls()
    E, N = nat.EINVAL, nat.ENOSUPPORT
    # (1) COR_EINVAL: null outputs / workspace, sizes, null arrays
    assert build(out_rows=None) == E and build(out_ids=None) == E and build(out_cs=None) == E and build(ws=None) == E
    assert build(dtype=nat.I8, dts=(nat.I8,), scale=(p,)) == E                                # an int8 index needs out_scale
    assert build(nseg=-1) == E and build(K=0) == E and build(C=0) == E and build(arrays=False) == E and build(assign_array=False) == E
    # (2) COR_ENOSUPPORT: too many segments
    many = dict(rows=(p,) * 17, scale=(None,) * 17, offs=tuple(range(0, 170, 10)), ns=(10,) * 17, dts=(nat.F32,) * 17, assign=(p,) * 17)
    assert build(**many) == N
    # (3) COR_EINVAL: the entries
    assert build(ns=(-1,)) == E and build(rows=(None,)) == E and build(assign=(None,)) == E
    assert build(dts=(nat.I8,), dtype=nat.I8, out_scale=p) == E                               # an int8 segment with rows needs its scales
    # (4) COR_ENOSUPPORT: the limits, the dtypes
    assert build(K=16385) == N and build(C=272) == N and build(C=24) == N
    assert build(dts=(3,)) == N and build(dtype=3, dts=(3,)) == N and build(dtype=7) == N and build(dtype=-1) == N
    assert build(dtype=nat.BF16) == N and build(dts=(nat.BF16,)) == N                         # rows are copied, never converted
    two = dict(rows=(p, p), scale=(None, None), offs=(0, 50), ns=(10, 0), assign=(p, p))
    assert build(dts=(nat.F32, nat.F16), **two) == N                                          # ... an empty segment of another dtype too
    # (5) COR_EINVAL: alignment
    assert build(out_rows=p + 8) == E and build(rows=(p + 4,)) == E and build(ws=p + 16) == E
    # precedence
    assert build(out_rows=None, **many) == E                                                  # (1) before (2)
    assert build(**dict(many, ns=(10,) * 16 + (-1,))) == N                                    # (2) before (3)
    assert build(ns=(-1,), K=16385) == E and build(rows=(None,), dtype=7) == E                # (3) before (4)
    assert build(K=16385, out_rows=p + 8) == N and build(dtype=7, ws=p + 16) == N             # (4) before (5)


def test_every_search_argument_error_comes_back_without_a_gpu():
    nat, lib, p, _, search = _calls()
    E, N = nat.EINVAL, nat.ENOSUPPORT
    for name in ("Q", "rows", "ids", "cs", "probes", "out_s", "out_i", "ws"):
        assert search(**{name: None}) == E, name
    assert search(dtype=nat.I8, scale=None) == E                                              # an int8 index needs its scales
    assert search(Bq=-1) == E and search(K=0) == E and search(C=0) == E and search(k=0) == E and search(nprobe=0) == E
    assert search(max_cell=0) == E and search(max_cell=-3) == E and search(split=-1) == E
    assert search(k=257) == N and search(nprobe=257) == N and search(K=16385) == N and search(C=272) == N and search(C=24) == N
    assert search(k=10, split=410) == N and search(k=256, split=17) == N and search(k=1, split=4097) == N
    assert search(dtype=3) == N and search(dtype=9) == N and search(dtype=-1) == N
    assert search(Q=p + 4) == E and search(rows=p + 8) == E and search(ws=p + 128) == E
    assert search(Bq=0) == 0 and search(Bq=0, out_n=p) == 0                                   # a successful no-op
    # precedence: (1) null pointers and sizes, (2) the limits, then the dtype, (3) alignment; all before Bq == 0
    assert search(Q=None, k=257) == E and search(k=0, nprobe=257) == E and search(split=-1, C=24) == E
    assert search(k=257, dtype=9) == N and search(dtype=9, Q=p + 4) == N and search(k=257, ws=p + 128) == N
    assert search(Bq=0, k=257) == N and search(Bq=0, Q=p + 4) == E and search(Bq=0, max_cell=0) == E


def test_workspace_queries_report_the_same_errors():
    nat, lib, p, _, _ = _calls()
    bw, sw = lib.cor_ivf_build_workspace_bytes, lib.cor_ivf_search_workspace_bytes
    assert bw(-1, 4, 64) == nat.EINVAL and bw(10, 0, 64) == nat.EINVAL and bw(10, 4, 0) == nat.EINVAL and bw(-1, 16385, 64) == nat.EINVAL
    assert bw(10, 16385, 64) == nat.ENOSUPPORT and bw(10, 4, 24) == nat.ENOSUPPORT and bw(2 ** 31, 4, 64) == nat.ENOSUPPORT
    for n in (0, 1, 2047, 2048, 2049, 10 ** 6):
        for K in (1, 33, 16384):
            b = bw(n, K, 64)
            assert b >= 4 * n + 4 * (-(-n // 2048)) * K + 4 * (K + 1) and b % 256 == 0        # a member list, the tiles x K counts, the bases
    assert sw(-1, 8, 64, 4, 10, 0) == nat.EINVAL and sw(2, 0, 64, 4, 10, 0) == nat.EINVAL and sw(2, 8, 64, 0, 10, 0) == nat.EINVAL
    assert sw(2, 8, 64, 4, 0, 0) == nat.EINVAL and sw(2, 8, 64, 4, 10, -1) == nat.EINVAL and sw(2, 8, 0, 4, 257, 0) == nat.EINVAL
    assert sw(2, 8, 64, 4, 257, 0) == nat.ENOSUPPORT and sw(2, 8, 64, 257, 10, 0) == nat.ENOSUPPORT and sw(2, 16385, 64, 4, 10, 0) == nat.ENOSUPPORT
    assert sw(2, 8, 24, 4, 10, 0) == nat.ENOSUPPORT and sw(2, 8, 64, 4, 10, 410) == nat.ENOSUPPORT
    for Bq in (0, 1, 32, 512, 5000):
        for k in (1, 10, 256):
            for split in (0, 1, 3, 4096 // k):
                b = sw(Bq, 8, 64, 4, k, split)
                assert b >= 0 and b % 256 == 0
                lists = split if split else min(-(-1024 // max(Bq, 1)), 4096 // k)
                assert b >= Bq * lists * (12 * k + 4)                                         # a (score, id) list of k and a count per partial list


def test_python_validation_comes_before_the_device():
    from cor_amd import ops
    from cor_amd import retrieval as R
    rows = torch.zeros((10, 64))
    a = torch.zeros((10,), dtype=torch.int32)
    with pytest.raises(ValueError, match="K must be"):
        ops.ivf_build([(rows, 0)], [a], 0)
    with pytest.raises(ValueError, match="share one dtype"):
        ops.ivf_build([(rows, 0), (rows.half(), 100)], [a, a], 4)
    with pytest.raises(ValueError, match="share one dtype"):
        ops.ivf_build([(rows, 0), (rows.to(torch.int8), torch.zeros(10), 100)], [a, a], 4)
    with pytest.raises(ValueError, match="assigns"):
        ops.ivf_build([(rows, 0)], [a, a], 4)
    with pytest.raises(ValueError, match="assigns must be"):
        ops.ivf_build([(rows, 0)], [a.long()], 4)
    with pytest.raises(ValueError, match="assigns must be"):
        ops.ivf_build([(rows, 0)], [a[:9]], 4)
    with pytest.raises(ValueError, match="multiple of 16"):
        ops.ivf_build([(torch.zeros((10, 24)), 0)], [a], 4)
    with pytest.raises(ValueError, match="no segment"):
        ops.ivf_build([], [], 4)
    with pytest.raises(RuntimeError, match="GPU only"):                                       # valid arguments, CPU tensors: there is no CPU path
        ops.ivf_build([(rows, 0)], [a], 4)

    Q, ids, cs, pr = torch.zeros((2, 64)), torch.zeros((10,), dtype=torch.int64), torch.zeros((5,), dtype=torch.int32), torch.zeros((2, 3), dtype=torch.int64)
    ok = dict(Q=Q, rows=rows, scales=None, ids=ids, cell_start=cs, probes=pr, k=5, max_cell=10)
    bad = [(dict(Q=Q.half()), "Q must be"), (dict(Q=torch.zeros((2, 24)), rows=torch.zeros((10, 24))), "multiple of 16"),
           (dict(rows=torch.zeros((10, 32))), "rows must be"), (dict(rows=rows.double()), "rows must be"),
           (dict(scales=torch.zeros(10)), "scales go with"), (dict(rows=rows.to(torch.int8)), "scales go with"),
           (dict(rows=rows.to(torch.int8), scales=torch.zeros(9)), "scales must be"), (dict(ids=ids.int()), "ids must be"), (dict(ids=ids[:9]), "ids must be"),
           (dict(cell_start=cs.long()), "cell_start must be"), (dict(cell_start=cs[:1]), "cell_start must be"),
           (dict(probes=pr.int()), "probes must be"), (dict(probes=pr[:1]), "probes must be"), (dict(probes=torch.zeros((2, 257), dtype=torch.int64)), "probes must be"),
           (dict(probes=torch.zeros((2, 0), dtype=torch.int64)), "probes must be"),
           (dict(k=0), "k must be"), (dict(k=257), "k must be"), (dict(max_cell=0), "max_cell"), (dict(split=-1), "split must be"), (dict(split=820), "split must be")]
    for change, msg in bad:
        with pytest.raises(ValueError, match=msg):
            ops.ivf_search(**dict(ok, **change))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.ivf_search(**ok)
    assert hasattr(R, "IVFIndex") and all(hasattr(c, "ivf") for c in (R.GalleryShard, R.QuantizedGallery, R.GallerySet))
    with pytest.raises(ValueError, match="pass a Clustering"):
        R.IVFIndex.build(None)
    with pytest.raises(ValueError, match="pass a Clustering"):
        R.IVFIndex.build(None, centroids=rows)
    with pytest.raises(ValueError, match="pass a Clustering"):
        R.IVFIndex.build(None, object(), assign=a)


def _toy(dtype, n=600, C=32, K=9, seed=3):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, C)).astype(F)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    assign = rng.integers(-1, K + 1, n).astype(np.int32)                                      # -1 and K: rows that are left out
    if dtype == "int8":
        from tests.i8_refs import ref_quantize
        q, sc = ref_quantize(x)
        segs = [(torch.from_numpy(q[:250]), sc[:250], 1000), (torch.from_numpy(q[250:]), sc[250:], 10)]
    else:
        t = torch.from_numpy(x).to(dtype)
        segs = [(t[:250], 1000), (t[250:], 10)]
    Q = rng.standard_normal((7, C)).astype(F)
    return segs, [assign[:250], assign[250:]], assign, Q / np.linalg.norm(Q, axis=1, keepdims=True), K


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16, "int8"], ids=str)
def test_the_restatements_on_a_case_that_can_be_followed(dtype):
    segs, assigns, assign, Q, K = _toy(dtype)
    rows, scales, ids, cs = ref_ivf_build(segs, assigns, K)
    gid = np.concatenate([np.arange(250) + 1000, np.arange(350) + 10])
    assert cs[0] == 0 and cs[K] == ((assign >= 0) & (assign < K)).sum() == rows.shape[0] == ids.shape[0]
    for c in range(K):
        mine = ids[cs[c]:cs[c + 1]]
        assert np.all(np.diff(mine) > 0) and set(mine.tolist()) == set(gid[assign == c].tolist())       # a cell: its rows in ascending id
    src = torch.cat([s[0] for s in segs])
    where = {int(g): n for n, g in enumerate(gid)}
    assert all(torch.equal(rows[s], src[where[int(ids[s])]]) for s in range(0, rows.shape[0], 37))      # the stored bits travel with the id
    # the segmentation and the segments' order do not show
    again = ref_ivf_build(segs[::-1], assigns[::-1], K)
    assert torch.equal(again[0], rows) and np.array_equal(again[2], ids) and np.array_equal(again[3], cs)
    # every cell probed (with hostile entries and repeats in the list): the exact search of the indexed rows
    probes = np.tile(np.concatenate([[-1, K, 2 ** 40, -2 ** 63], np.arange(K), np.arange(K)]), (Q.shape[0], 1)).astype(np.int64)
    s, i, scanned = ref_ivf_search(Q, rows, scales, ids, cs, probes, 12)
    es, ei = ref_exact(Q, rows, scales, ids, 12)
    assert np.array_equal(s.view(np.uint32), es.view(np.uint32)) and np.array_equal(i, ei) and np.all(scanned == rows.shape[0])
    # one cell: only its rows, the (-inf, -1) tail behind them; no valid probe: only the tail
    small = int(np.argmin(np.diff(cs)))
    s, i, scanned = ref_ivf_search(Q, rows, scales, ids, cs, np.full((Q.shape[0], 2), small, np.int64), 200)
    m = int(cs[small + 1] - cs[small])
    assert np.all(scanned == m) and np.all(i[:, m:] == -1) and np.all(np.isneginf(s[:, m:]))
    assert all(set(r[:m].tolist()) == set(ids[cs[small]:cs[small + 1]].tolist()) for r in i)
    s, i, scanned = ref_ivf_search(Q, rows, scales, ids, cs, np.full((Q.shape[0], 3), -1, np.int64), 5)
    assert np.all(i == -1) and np.all(np.isneginf(s)) and np.all(scanned == 0)


def purpose_fixture():
    """The fixture of the feature's purpose: planted rows, the reference clustering, queries drawn like the rows -> everything the CPU
    test and the GPU test share."""
    from oracle import retrieval as oret
    x, _, d = planted(n=4096, modes=8, C=64, noise=0.25, seed=1234)
    cl = ref_cluster([(x, 0)], K=64, iters=6)
    rng = np.random.default_rng(1235)
    q = d[rng.integers(0, 8, 64)] + 0.25 * rng.standard_normal((64, 64))
    Q = np.ascontiguousarray(q / np.linalg.norm(q, axis=1, keepdims=True), dtype=F)
    order = oret.similarity_topk(torch.from_numpy(Q), torch.from_numpy(cl["centroids"]), 64, exact_chain=True)[1].numpy()
    return x, cl, Q, order


def test_purpose_a_few_probes_find_most_neighbours_in_a_fraction_of_the_rows():
    x, cl, Q, order = purpose_fixture()
    counts = np.asarray(cl["counts"])
    assert counts.sum() == 4096 and counts.min() >= 1
    rows, scales, ids, cs = ref_ivf_build([(torch.from_numpy(x), 0)], cl["assign"], 64)
    _, truth = ref_exact(Q, rows, None, ids, 10)
    rec, share = {}, {}
    for nprobe in (1, 2, 4, 8, 16, 64):
        _, i, scanned = ref_ivf_search(Q, rows, None, ids, cs, order[:, :nprobe], 10)
        rec[nprobe], share[nprobe] = recall(i, truth), float(scanned.mean()) / 4096
        print(f"nprobe {nprobe}: recall@10 {rec[nprobe]:.3f}, rows scanned {100 * share[nprobe]:.1f} %")
        if nprobe == 64:
            assert np.array_equal(i, truth)
    probes = sorted(rec)
    assert all(rec[a] <= rec[b] for a, b in zip(probes, probes[1:]))
    assert rec[1] < 0.5
    assert rec[8] >= 0.9 and share[8] <= 0.20
    assert rec[64] == 1.0

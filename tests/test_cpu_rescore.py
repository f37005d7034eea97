"""CPU-side checks (run under -m "not gpu") of the candidate re-scoring's host layers: the exports of cor_rescore_topk, its argument
checks (all made before any HIP call), the no-CPU-path rule and two_stage_search's validation."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_rescore_symbols():
    from cor_amd import _native
    lib = _native.load()
    hdr = open(os.path.join(ROOT, "include", "cor_amd.h")).read()
    for name, nargs, restype in (("cor_rescore_workspace_bytes", 3, "long"), ("cor_rescore_topk", 15, "int")):
        proto = re.search(r"^%s\s+%s\s*\(([^)]*)\)\s*;" % (restype, name), hdr, flags=re.M | re.S)
        assert proto, f"{name} is not declared in include/cor_amd.h"
        assert len(proto.group(1).split(",")) == nargs == len(_native.SIGNATURES[name])
        assert hasattr(lib, name)
    assert _native._RESTYPE["cor_rescore_workspace_bytes"] is _native._l
    assert "cor_rescore_topk" not in _native._RESTYPE                  # int, the default
    assert lib.cor_rescore_topk.restype is _native._i and lib.cor_rescore_workspace_bytes.restype is _native._l


def test_rescore_argument_errors_need_no_gpu():
    """Every argument check comes before any HIP call: the call returns the error, the workspace query reports those it can see."""
    from cor_amd import _native
    lib = _native.load()
    E, N = _native.EINVAL, _native.ENOSUPPORT
    buf = torch.zeros(64, dtype=torch.int64)
    p = buf.data_ptr()

    def call(Q=p, G=p, dt=_native.F32, Bq=1, Ng=10, C=256, off=0, cand=p, kin=4, k=4, os_=p, oi=p, op=None):
        return lib.cor_rescore_topk(Q, G, dt, Bq, Ng, C, off, cand, kin, k, os_, oi, op, None, None)

    assert call(Q=None) == E and call(cand=None) == E and call(oi=None) == E and call(os_=None) == E and call(G=None) == E
    assert call(k=0) == E and call(k=257) == E and call(kin=0) == E and call(Bq=-1) == E and call(Ng=-1) == E
    assert call(kin=4097) == N and call(C=8) == N and call(C=272) == N and call(C=24) == N and call(dt=3) == N and call(dt=-1) == N
    assert call(Bq=0) == 0 and call(Bq=0, op=p) == 0                   # no queries: a no-op
    for dt in (_native.F32, _native.BF16, _native.F16):
        assert call(dt=dt, Bq=0, kin=4096, k=256, C=16) == 0
    ws = lib.cor_rescore_workspace_bytes
    assert ws(1, 4, 4) == 0 and ws(0, 1, 1) == 0 and ws(512, 4096, 256) == 0
    assert ws(1, 4, 0) == E and ws(1, 4, 257) == E and ws(1, 0, 4) == E and ws(-1, 4, 4) == E
    assert ws(1, 4097, 4) == N


def _cpu_shard(rows, offset=0):
    """A GalleryShard lives in GPU memory and its constructor says so; the method under test only reads rows and offset."""
    from cor_amd.retrieval import GalleryShard
    sh = GalleryShard.__new__(GalleryShard)
    sh.rows, sh.offset, sh.labels, sh.groups = rows, offset, None, None
    return sh


def test_rescore_has_no_cpu_path():
    from cor_amd import ops
    Q, G, cand = torch.zeros((2, 16)), torch.zeros((5, 16)), torch.zeros((2, 3), dtype=torch.int64)
    with pytest.raises(RuntimeError):
        ops.rescore_topk(Q, G, cand, 3)
    with pytest.raises(RuntimeError):
        ops.rescore_topk(Q, G.to(torch.bfloat16), cand, 3, g_offset=7, return_pos=True)
    with pytest.raises(RuntimeError):
        _cpu_shard(G).rescore(Q, cand)
    with pytest.raises(RuntimeError):
        _cpu_shard(G, 100).rescore(Q, cand, k=2, return_pos=True)
    for bad in (dict(k=0), dict(k=257)):
        with pytest.raises(ValueError):
            ops.rescore_topk(Q, G, cand, **bad)
    with pytest.raises(ValueError):
        ops.rescore_topk(Q, G, cand.to(torch.int32), 3)                # ids are int64
    with pytest.raises(ValueError):
        ops.rescore_topk(Q, G, cand[:1], 3)                            # one list per query
    with pytest.raises(ValueError):
        ops.rescore_topk(Q, G, cand[0], 3)                             # not [Bq, kin]
    with pytest.raises(ValueError):
        ops.rescore_topk(Q, G, cand[:, :0], 3)                         # kin = 0
    with pytest.raises(ValueError):
        ops.rescore_topk(Q, torch.zeros((5, 32)), cand, 3)             # another width
    with pytest.raises(ValueError):
        ops.rescore_topk(Q.double(), G, cand, 3)
    with pytest.raises(ValueError):
        _cpu_shard(G).rescore(Q, cand[0])


class _Never:
    """A shard that must not be touched."""

    def search(self, *a, **kw):
        raise AssertionError("two_stage_search searched before it validated k")

    rescore = search


def test_two_stage_search_validates_k_first():
    from cor_amd import retrieval
    for k, kc in ((11, 10), (10, 257), (0, 10), (300, 300)):
        with pytest.raises(ValueError):
            retrieval.two_stage_search(None, _Never(), _Never(), k, kc)


def test_two_stage_search_composes_search_and_rescore():
    """The plumbing, with stub shards: the coarse stage gets k_coarse and the keywords, the fine stage the coarse ids, k and the second
    query vector."""
    from cor_amd import retrieval
    seen = {}

    class Coarse:
        def search(self, q, k, **kw):
            seen["coarse"] = (q, k, kw)
            return "scores", "ids"

    class Fine:
        def rescore(self, q, cand, k):
            seen["fine"] = (q, cand, k)
            return "s2", "i2"

    assert retrieval.two_stage_search("q", Coarse(), Fine(), 10, 100, query_labels="ql", mode="ne") == ("s2", "i2")
    assert seen["coarse"] == ("q", 100, dict(query_labels="ql", mode="ne")) and seen["fine"] == ("q", "ids", 10)
    retrieval.two_stage_search("q", Coarse(), Fine(), 100, 100, fine_queries="q2", distinct=True)
    assert seen["coarse"] == ("q", 100, dict(distinct=True)) and seen["fine"] == ("q2", "ids", 100)


def test_gallery_set_rescore_without_rows():
    from cor_amd.retrieval import GallerySet
    from tests.test_cpu_merge_device import _Seg
    cand = torch.tensor([[3, 4, 5], [-1, 0, 9]])
    for empty in (GallerySet(), GallerySet([_Seg(0, 3)])):
        s, i = empty.rescore(torch.zeros((2, 8)), cand, 4)
        assert torch.equal(s, torch.full((2, 4), float("-inf"))) and torch.equal(i, torch.full((2, 4), -1, dtype=torch.int64))
    with pytest.raises(ValueError):
        GallerySet().rescore(torch.zeros((2, 8)), cand, 257)

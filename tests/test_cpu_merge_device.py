"""CPU-side checks (run under -m "not gpu") of the device merge's host layers: the exports of cor_merge_topk, the no-CPU-path rule,
GallerySet's validation (with stub segments: a GalleryShard lives in GPU memory) and distributed_search's `merge` keyword on a
world-2 gloo group (ranks started as tests/test_cpu_distributed.py starts them)."""
import os
import re

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.test_cpu_distributed import _OracleShard, _free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_merge_symbols():
    from cor_amd import _native
    lib = _native.load()
    hdr = open(os.path.join(ROOT, "include", "cor_amd.h")).read()
    for name, nargs, restype in (("cor_merge_topk_workspace_bytes", 4, "long"), ("cor_merge_topk", 12, "int")):
        proto = re.search(r"^%s\s+%s\s*\(([^)]*)\)\s*;" % (restype, name), hdr, flags=re.M | re.S)
        assert proto, f"{name} is not declared in include/cor_amd.h"
        assert len(proto.group(1).split(",")) == nargs == len(_native.SIGNATURES[name])
        assert hasattr(lib, name)
    assert _native._RESTYPE["cor_merge_topk_workspace_bytes"] is _native._l
    assert _native.MERGE_NMAX == int(re.search(r"#define COR_MERGE_NMAX (\d+)", hdr).group(1)) == 4096


def test_merge_shape_errors_need_no_gpu():
    """The shape checks come before any HIP call: the workspace query reports them as negative values, the call returns them."""
    from cor_amd import _native
    lib = _native.load()
    ws = lib.cor_merge_topk_workspace_bytes
    assert ws(8, 5, 256, 256) == 0 and ws(16, 2, 256, 256) == 0 and ws(1, 0, 1, 1) == 0
    assert ws(17, 1, 256, 256) == _native.ENOSUPPORT and ws(1, 1, 4097, 10) == _native.ENOSUPPORT
    for bad in ((0, 1, 4, 4), (2, -1, 4, 4), (2, 1, 0, 4), (2, 1, 4, 0), (2, 1, 4, 257)):
        assert ws(*bad) == _native.EINVAL, bad
    buf = torch.zeros(64, dtype=torch.int64)
    p = buf.data_ptr()
    assert lib.cor_merge_topk(None, p, None, 2, 1, 4, 4, p, p, None, None, None) == _native.EINVAL      # null required pointers
    assert lib.cor_merge_topk(p, p, None, 2, 1, 4, 4, p, None, None, None, None) == _native.EINVAL
    assert lib.cor_merge_topk(p, p, None, 2, 1, 4, 257, p, p, None, None, None) == _native.EINVAL
    assert lib.cor_merge_topk(p, p, None, 17, 1, 256, 256, p, p, None, None, None) == _native.ENOSUPPORT
    assert lib.cor_merge_topk(p, p, None, 2, 0, 4, 4, p, p, None, None, None) == 0                      # no queries: a no-op


def test_merge_topk_has_no_cpu_path():
    from cor_amd import ops, retrieval
    s, i = torch.zeros((2, 3, 4)), torch.zeros((2, 3, 4), dtype=torch.int64)
    with pytest.raises(RuntimeError):
        ops.merge_topk(s, i, 4)
    with pytest.raises(RuntimeError):
        retrieval.merge_topk_device([s[0], s[1]], [i[0], i[1]], 4)
    for bad in (dict(k=0), dict(k=257)):
        with pytest.raises(ValueError):
            ops.merge_topk(s, i, **bad)
    with pytest.raises(ValueError):
        ops.merge_topk(s[0], i[0], 4)                                  # not [P, B, kin]
    with pytest.raises(ValueError):
        ops.merge_topk(s, i[:, :, :3], 4)
    with pytest.raises(ValueError):
        ops.merge_topk(s, i, 4, groups=torch.zeros((2, 3, 4), dtype=torch.int64))
    with pytest.raises(ValueError):
        retrieval.merge_topk_device([], [], 4)


class _Seg:
    """What GallerySet reads of a segment."""

    def __init__(self, n, offset, C=8, labels=False, groups=False):
        self.rows, self.offset = torch.zeros((n, C)), offset
        self.labels = torch.zeros(n, dtype=torch.int32) if labels else None
        self.groups = torch.arange(n, dtype=torch.int32) + 100 * (offset % 1000) if groups else None

    def __len__(self):
        return self.rows.shape[0]


def test_gallery_set_validation():
    from cor_amd.retrieval import GallerySet
    a, b, c = _Seg(10, 0), _Seg(5, 20), _Seg(10, 10)
    gs = GallerySet([b, a])
    assert len(gs) == 15 and gs.segments == [a, b] and gs.labels is None and gs.groups is None
    gs.add(c)
    assert len(gs) == 25 and gs.segments == [a, c, b] and tuple(gs.rows.shape) == (0, 8)
    for lo, n in ((5, 10), (19, 2), (24, 1), (0, 100), (12, 3), (10, 0)):
        with pytest.raises(ValueError):
            gs.add(_Seg(n, lo))
    with pytest.raises(ValueError):
        gs.add(_Seg(4, 100, C=16))                                    # another embedding width
    with pytest.raises(ValueError):
        gs.add(_Seg(4, 100, labels=True))                             # labels on one segment only
    with pytest.raises(ValueError):
        gs.add(_Seg(4, 100, groups=True))
    with pytest.raises(ValueError):
        GallerySet([_Seg(4, 0, groups=True), _Seg(4, 4)])
    assert len(gs) == 25 and len(gs.segments) == 3                    # a refused segment leaves the set as it was
    with pytest.raises(KeyError):
        gs.drop(5)
    assert gs.drop(10) is c and gs.segments == [a, b] and len(gs) == 15
    gs.add(_Seg(0, 15))                                               # an empty segment between the others is legal
    assert len(gs) == 15 and len(gs.segments) == 3
    assert len(GallerySet()) == 0 and GallerySet().segments == []
    with pytest.raises(ValueError):
        GallerySet().rows
    seg = gs.segments
    seg.clear()
    assert len(gs.segments) == 3                                      # `segments` is a copy


def test_gallery_set_entry_groups_and_empty_search():
    from cor_amd.retrieval import GallerySet
    gs = GallerySet([_Seg(4, 10, groups=True), _Seg(0, 14, groups=True), _Seg(3, 5 * 10 ** 9, groups=True)])
    gs.segments[2].groups[1] = -7                                     # a negative id is an id, not "missing"
    idx = torch.tensor([[10, 13, -1], [5 * 10 ** 9 + 2, 5 * 10 ** 9 + 1, 12]])
    want = torch.tensor([[1000, 1003, -1], [2, -7, 1002]], dtype=torch.int32)
    got = gs.entry_groups(idx)
    assert got.dtype == torch.int32 and torch.equal(got, want)
    for empty in (GallerySet(), GallerySet([_Seg(0, 3)])):
        s, i = empty.search(torch.zeros((2, 8)), 3)
        assert torch.equal(s, torch.full((2, 3), float("-inf"))) and torch.equal(i, torch.full((2, 3), -1, dtype=torch.int64))
    with pytest.raises(ValueError):
        GallerySet([_Seg(0, 3)]).search(torch.zeros((2, 8)), 3, distinct=True)


def test_distributed_search_rejects_an_unknown_merge():
    from cor_amd import retrieval
    with pytest.raises(ValueError):
        retrieval.distributed_search(torch.zeros((1, 8)), _OracleShard(torch.zeros((4, 8)), 0), 2, merge="bogus")


def _worker(rank, world, port, G, Q, k, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from cor_amd import retrieval
        lo, hi = retrieval.shard_bounds(G.shape[0], world, rank)
        shard = _OracleShard(G[lo:hi], lo)
        q = Q[rank * 3:(rank + 1) * 3]
        refused = 0
        for kw in (dict(), dict(dst=None), dict(defer=True)):
            try:                                                      # refused on EVERY rank before a collective: nobody hangs
                retrieval.distributed_search(q, shard, k, merge="device", **kw)
            except ValueError:
                refused += 1
        out[f"refused{rank}"] = refused
        try:
            retrieval.distributed_search(q, shard, k, merge="bogus")
        except ValueError:
            out[f"bogus{rank}"] = True
        s0, i0 = retrieval.distributed_search(q, shard, k)            # today's call
        s1, i1 = retrieval.distributed_search(q, shard, k, merge="host")
        if rank == 0:
            out["same"] = bool(torch.equal(s0, s1) and torch.equal(i0, i1))
            out["s"], out["i"] = s1, i1
        else:
            out["none"] = s1 is None and i1 is None
    finally:
        dist.destroy_process_group()


def test_merge_keyword_on_a_world2_gloo_group():
    from oracle import retrieval as oret
    gen = torch.Generator().manual_seed(3)
    G = torch.nn.functional.normalize(torch.randn((300, 256), generator=gen), dim=-1)
    G[200] = G[7]                                                     # a tie across the two shards
    Q = torch.nn.functional.normalize(torch.randn((6, 256), generator=gen), dim=-1)
    out = mp.Manager().dict()
    mp.spawn(_worker, args=(2, _free_port(), G, Q, 10, out), nprocs=2, join=True)
    assert out["refused0"] == 3 and out["refused1"] == 3 and out["bogus0"] and out["bogus1"]
    assert out["same"] and out["none"]
    rs, ri = oret.similarity_topk(Q, G, 10)
    assert torch.equal(out["i"], ri) and torch.allclose(out["s"], rs)

"""CPU side of the filtered threshold search, cor_similarity_range_filtered: the library's exports and argument checks (no device needed),
the workspace query swept over shard sizes, the Python fronts' validation and the new keywords' errors, the restatement
tests/range_filtered_refs.py against hand-checkable floors and a float64 formulation, the purpose fixture (ingest-time de-duplication:
"does this region already exist in ANOTHER image"), and distributed_search(min_score=...) under gloo with a test double whose
range_search is the restatement."""
import os
import re
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import range_filtered_refs as RF
from tests import range_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _proto_args(hdr, ret, name):
    proto = re.search(r"^" + ret + r"\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr, flags=re.M | re.S)
    assert proto, f"{name} is not declared in include/cor_amd.h"
    return len(proto.group(1).split(","))


def _unit(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def test_library_exports_the_filtered_range_symbols():
    from cor_amd import _native, ops
    lib = _native.load()
    hdr = open(os.path.join(ROOT, "include", "cor_amd.h")).read()
    assert _proto_args(hdr, "long", "cor_range_filtered_workspace_bytes") == 3 == len(_native.SIGNATURES["cor_range_filtered_workspace_bytes"])
    assert _proto_args(hdr, "int", "cor_similarity_range_filtered") == 18 == len(_native.SIGNATURES["cor_similarity_range_filtered"])
    assert lib.cor_similarity_range_filtered.restype is _native._i and lib.cor_range_filtered_workspace_bytes.restype is _native._l
    assert _native.SIGNATURES["cor_similarity_range_filtered"][8] is _native._ll   # g_offset
    assert callable(ops.similarity_range_filtered)


def test_filtered_range_argument_errors_need_no_gpu():
    """Every argument check comes before any HIP call, in cor_similarity_range's order and with its codes; the label checks are those of
    cor_similarity_topk_filtered."""
    from cor_amd import _native
    lib = _native.load()
    E, N = _native.EINVAL, _native.ENOSUPPORT
    buf = torch.zeros(4096, dtype=torch.uint8)
    p = (buf.data_ptr() + 255) & ~255                                              # 256-byte aligned, 3 KiB behind it

    def call(Q=p, G=p, dt=_native.F32, Bq=1, Ng=8, C=64, thr=p, k=4, off=0, rl=p, ql=p, mode=_native.FILTER_EQ, out_s=p, out_i=p, out_c=p,
             ws=p, flags=0):
        return lib.cor_similarity_range_filtered(Q, G, dt, Bq, Ng, C, thr, k, off, rl, ql, mode, out_s, out_i, out_c, ws, flags, None)

    assert call(Q=None) == E and call(G=None) == E and call(thr=None) == E and call(out_c=None) == E
    assert call(rl=None) == E and call(ql=None) == E
    assert call(out_s=None) == E and call(out_i=None) == E and call(ws=None) == E
    assert call(Bq=0) == E and call(Ng=0) == E and call(k=0) == E and call(Bq=-1) == E and call(k=-5) == E
    assert call(mode=2) == E and call(mode=-1) == E and call(mode=_native.FILTER_NE, Ng=0) == E
    assert call(k=257) == N and call(C=272) == N and call(C=40) == N and call(C=8) == N
    for flag in (_native.TOPK_FORCE_LISTS, _native.TOPK_FORCE_GLOBAL_THRESHOLD, _native.TOPK_WAVE_FINAL, 4, 1 << 20,
                 _native.TOPK_NO_FALLBACK | _native.TOPK_FORCE_LISTS):
        assert call(flags=flag) == N, flag
        assert call(flags=flag, k=40) == N, flag
    assert call(Q=p + 4) == E and call(G=p + 8) == E and call(ws=p + 16) == E
    assert call(rl=p + 4) == E and call(rl=p + 8) == E                             # row labels are read 16 bytes at a time
    assert call(ql=p + 4, dt=9) == N                                               # query labels need no alignment: on to the dtype
    assert call(dt=9) == N and call(dt=_native.BF16X3) == N                        # after every other check: no kernel for the dtype
    # the order: null / counts, the filter mode, the shape and the flags, the alignment, the dtype
    assert call(Q=None, k=257) == E and call(rl=None, k=257) == E and call(ql=None, flags=1) == E and call(out_c=None, flags=1) == E
    assert call(mode=2, k=257) == E and call(mode=2, flags=1) == E
    assert call(Q=p + 4, k=257) == N and call(rl=p + 4, k=257) == N and call(rl=p + 4, flags=1) == N and call(Ng=0, C=40) == E
    assert call(rl=p + 4, dt=9) == E

    ws = lib.cor_range_filtered_workspace_bytes
    assert ws(0, 10, 1) == E and ws(1, 0, 1) == E and ws(1, 10, 0) == E and ws(1, 10, 257) == E


def test_filtered_range_workspace_covers_every_shard_size():
    """Positive for Ng from 1 to 2^31 - 1 at k = 1 and 256, and at least the filtered top-k's workspace at the same arguments."""
    from cor_amd import _native
    lib = _native.load()
    sizes = sorted({1, 2, 31, 32, 33, 63, 64, 65, 4095, 4096, 4097, 20000, 125000, 1_000_000, 2 ** 31 - 1}
                   | {2 ** e for e in range(1, 31)} | {2 ** e + 1 for e in range(1, 31)} | {3 * 2 ** e - 1 for e in range(1, 29)})
    for Ng in sizes:
        for Bq in (1, 33, 256, 257, 512, 513):
            for k in (1, 33, 100, 256):
                n = lib.cor_range_filtered_workspace_bytes(Bq, Ng, k)
                assert n > 0 and n % 256 == 0, (Bq, Ng, k, n)
                assert n >= lib.cor_topk_filtered_workspace_bytes(Bq, Ng, k), (Bq, Ng, k)


def _cpu_shard(retrieval, rows, labels=None, offset=0):
    sh = retrieval.GalleryShard.__new__(retrieval.GalleryShard)                     # the constructor refuses CPU tensors
    sh.rows, sh.offset, sh.labels, sh.groups = rows, offset, labels, None
    return sh


def test_python_validation_new_keywords_and_no_cpu_path():
    from cor_amd import ops, retrieval
    Q, G = torch.zeros((2, 32)), torch.zeros((5, 32))
    rl, ql = torch.zeros(5, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    for k in (0, 257, -1):
        with pytest.raises(ValueError):
            ops.similarity_range_filtered(Q, G, 0.5, k, rl, ql)
    for bad in (torch.zeros(3), torch.zeros((2, 1)), torch.zeros(2, dtype=torch.float64), torch.zeros(2, dtype=torch.int32), "0.5"):
        with pytest.raises(ValueError):
            ops.similarity_range_filtered(Q, G, bad, 3, rl, ql)
    with pytest.raises(ValueError, match="mode"):
        ops.similarity_range_filtered(Q, G, 0.5, 3, rl, ql, mode="lt")
    for thr in (0.5, torch.zeros(2)):
        for mode in ("eq", "ne"):
            with pytest.raises(RuntimeError, match="GPU only"):                    # valid arguments on the CPU: no CPU path
                ops.similarity_range_filtered(Q, G, thr, 3, rl, ql, mode=mode)
    # the shard and the set: labels without row labels, then the same "GPU only" error through the filtered call
    bare, labelled = _cpu_shard(retrieval, G), _cpu_shard(retrieval, G, rl)
    with pytest.raises(ValueError, match="no row labels"):
        bare.range_search(Q, 0.5, 3, query_labels=ql)
    with pytest.raises(ValueError, match="no row labels"):
        retrieval.GallerySet([bare]).range_search(Q, 0.5, 3, query_labels=ql, mode="ne")
    with pytest.raises(RuntimeError, match="GPU only"):
        labelled.range_search(Q, 0.5, 3, query_labels=ql, mode="ne")
    with pytest.raises(RuntimeError, match="GPU only"):
        retrieval.GallerySet([labelled]).range_search(Q, 0.5, 3, query_labels=ql)
    with pytest.raises(ValueError, match="mode"):
        labelled.range_search(Q, 0.5, 3, query_labels=ql, mode="lt")
    with pytest.raises(ValueError):
        labelled.range_search(Q, 0.5, 300, query_labels=ql)
    # the pinned int8 behaviour stays: no range_search on a QuantizedShard, a set with an int8 segment names int8
    i8 = retrieval.QuantizedShard.__new__(retrieval.QuantizedShard)
    i8.rows, i8.scales, i8.offset, i8.labels, i8.groups = torch.zeros((5, 32), dtype=torch.int8), torch.zeros(5), 5, rl, None
    assert not hasattr(i8, "range_search")
    with pytest.raises(ValueError, match="int8"):
        retrieval.GallerySet([labelled, i8]).range_search(Q, 0.5, 3, query_labels=ql)
    # nothing to search: all-missing lists and zero counts with the keywords too
    s, i, c = retrieval.GallerySet().range_search(Q, 0.5, 3, query_labels=ql, mode="ne")
    assert s.shape == (2, 3) and torch.isneginf(s).all() and (i == -1).all() and c.dtype == torch.int32 and c.tolist() == [0, 0]
    # distributed_search: the two refusals come before anything else (no process group here)
    assert not dist.is_initialized()
    grouped = _cpu_shard(retrieval, G, rl)
    grouped.groups = rl
    with pytest.raises(ValueError, match="min_score"):
        retrieval.distributed_search(Q, grouped, 3, min_score=0.5, distinct=True)
    with pytest.raises(ValueError, match="int8"):
        retrieval.distributed_search(Q, i8, 3, min_score=0.5)
    with pytest.raises(ValueError, match="int8"):
        retrieval.distributed_search(Q, retrieval.GallerySet([labelled, i8]), 3, min_score=0.5, query_labels=ql)
    with pytest.raises(ValueError, match="min_score"):
        retrieval.distributed_search(Q, labelled, 3, min_score="0.5")
    with pytest.raises(RuntimeError, match="GPU only"):                            # a valid call reaches the shard's range_search
        retrieval.distributed_search(Q, labelled, 3, min_score=0.5, query_labels=ql)


def test_hand_checkable_filtered_floors():
    # rows 0..5 against q = e0: scores 0.5, 0.25, 0.5, -1, 0, 0.25; labels 1, 1, 2, 2, 1, 3
    G = np.zeros((6, 8), dtype=F)
    G[:, 0] = [0.5, 0.25, 0.5, -1.0, 0.0, 0.25]
    rl = np.array([1, 1, 2, 2, 1, 3], dtype=np.int32)
    Q = np.zeros((6, 8), dtype=F)
    Q[:, 0] = 1.0
    S = R.chain_scores(torch.from_numpy(Q), torch.from_numpy(G))
    assert S[0].tolist() == [0.5, 0.25, 0.5, -1.0, 0.0, 0.25]
    ql = np.array([1, 1, 2, -1, 7, 3], dtype=np.int32)
    thr = np.array([0.25, -np.inf, 0.5, 0.25, -np.inf, np.nextafter(F(0.25), F(1))], dtype=F)
    eq = RF.allow_mask(rl, ql, "eq")
    assert eq[0].tolist() == [True, True, False, False, True, False] and eq[3].all() and not eq[4].any()
    s, i, c = RF.range_from_scores(S, eq, thr, 3, g_offset=100)
    assert c.tolist() == [2, 3, 1, 4, 0, 0]
    assert i[0].tolist() == [100, 101, -1] and s[0, :2].tolist() == [0.5, 0.25] and np.isneginf(s[0, 2])
    assert i[1].tolist() == [100, 101, 104]                                        # -inf: every allowed row, and only those
    assert i[2].tolist() == [102, -1, -1]                                          # class 2: row 2 on the floor, row 3 below it
    assert i[3].tolist() == [100, 102, 101]                                        # unrestricted: the plain range search, cut at k
    assert (i[4] == -1).all() and np.isneginf(s[4]).all()                          # an absent class: count 0, only the tail
    assert (i[5] == -1).all()                                                      # the class's one row lies one ulp below the floor
    ne = RF.allow_mask(rl, ql, "ne")
    assert ne[0].tolist() == [False, False, True, True, False, True] and ne[3].all() and ne[4].all()
    s, i, c = RF.range_from_scores(S, ne, thr, 3, g_offset=100)
    assert c.tolist() == [2, 3, 1, 4, 6, 2]
    assert i[0].tolist() == [102, 105, -1] and i[1].tolist() == [102, 105, 103] and i[2].tolist() == [100, -1, -1]
    assert i[4].tolist() == [100, 102, 101] and i[5].tolist() == [100, 102, -1]     # everything but the query's own class
    # NaN, +inf and the two zeros, under a filter
    thr2 = np.array([np.nan, np.inf, 0.0, -0.0, 0.0, 0.25], dtype=F)
    s, i, c = RF.range_from_scores(S, eq, thr2, 3)
    assert c.tolist() == [0, 0, 1, 5, 0, 1] and i[2].tolist() == [2, -1, -1] and i[5].tolist() == [5, -1, -1]
    # all query labels negative: the unfiltered restatement, bit for bit
    free = RF.allow_mask(rl, np.full(6, -1), "ne")
    a, b = RF.range_from_scores(S, free, thr, 4, 9), R.range_from_scores(S, thr, 4, 9)
    assert all((x == y).all() for x, y in zip(a, b))


@pytest.mark.parametrize("mode", ["eq", "ne"])
@pytest.mark.parametrize("gdt", [torch.float32, torch.bfloat16, torch.float16])
def test_filtered_restatement_against_float64(gdt, mode):
    """Counts may differ from a float64 evaluation only where the float64 score of an ALLOWED row lies within 3.1e-5 of the floor (the
    bound oracle/retrieval.py states for unit vectors); the listed rows are allowed members in (score desc, index asc) order."""
    rng = np.random.default_rng(13)
    C, Ng, Bq, k = 64, 4000, 24, 50
    G = torch.from_numpy(_unit(rng.standard_normal((Ng, C))).astype(F)).to(gdt)
    Q = torch.from_numpy(_unit(rng.standard_normal((Bq, C))).astype(F))
    rl = rng.integers(0, 4, Ng).astype(np.int32)
    ql = rng.integers(0, 4, Bq).astype(np.int32)
    ql[::7] = -1
    thr = np.linspace(-0.05, 0.30, Bq).astype(F)
    s, i, c = RF.similarity_range_filtered(Q, G, thr, k, rl, ql, mode, g_offset=7)
    allow = RF.allow_mask(rl, ql, mode)
    Qr = Q if gdt == torch.float32 else Q.to(gdt).float()
    S64 = Qr.double().numpy() @ G.double().numpy().T
    S32 = R.chain_scores(Q, G)
    assert np.abs(S32 - S64).max() < 3.1e-5
    m64 = allow & (S64 >= thr.astype(np.float64)[:, None])
    near = allow & (np.abs(S64 - thr.astype(np.float64)[:, None]) <= 3.1e-5)
    m32 = allow & (S32 >= thr[:, None])
    assert not ((m32 != m64) & ~near).any()
    assert (np.abs(c.astype(np.int64) - m64.sum(1)) <= near.sum(1)).all()
    assert (c == m32.sum(1)).all() and c.min() < k < c.max()                       # both a tail and a cut list occur
    for b in range(Bq):
        n = min(int(c[b]), k)
        assert (i[b, n:] == -1).all() and np.isneginf(s[b, n:]).all()
        rows = i[b, :n] - 7
        assert allow[b, rows].all() and (S32[b, rows] == s[b, :n]).all() and (s[b, :n] >= thr[b]).all()
        key = list(zip((-s[b, :n]).tolist(), rows.tolist()))
        assert key == sorted(key)
        if n == k < c[b]:                                                          # the k best members: nothing better was left out
            rest = np.setdiff1d(np.nonzero(m32[b])[0], rows)
            assert S32[b, rest].max() <= s[b, n - 1]


def test_purpose_ne_on_the_image_id_finds_the_regions_that_exist_in_another_image():
    """Ingest-time de-duplication over a multi-region gallery: 3 000 unit rows at C = 64 (seed 7), 100 images x 30 regions, label = image
    id. 50 rows get a copy + 0.03 N(0, 1) per channel, renormalised, written over a row of ANOTHER image; every row is a query, floor
    0.9. Unfiltered, every row matches itself: the count is >= 1 for all 3 000 and says nothing. With `ne` on the image id the count is
    > 0 for exactly the 100 planted rows (the 50 sources and their 50 copies) and is 1 for each. The planted cosines are >= 0.959 and
    every other pair of rows <= 0.633 (plain fp32, checked here): the floor sits 0.05 and 0.26 away, a thousand times the
    chain-vs-fp32 difference."""
    rng = np.random.default_rng(7)
    G = _unit(rng.standard_normal((3000, 64)))
    lab = np.repeat(np.arange(100), 30).astype(np.int32)
    perm = rng.permutation(3000)
    src, rest, tgt, at = perm[:50], perm[50:], [], 0
    for s_ in src:                                                                 # the next unused row of another image
        while lab[rest[at]] == lab[s_]:
            at += 1
        tgt.append(rest[at]); at += 1
    tgt = np.array(tgt)
    G[tgt] = _unit(G[src] + 0.03 * rng.standard_normal((50, 64)))
    G = G.astype(F)
    planted = np.zeros(3000, dtype=bool)
    planted[src] = planted[tgt] = True
    assert planted.sum() == 100 and (lab[src] != lab[tgt]).all()
    S = G @ G.T                                                                    # plain fp32 scores
    assert S[src, tgt].min() >= 0.959
    other = S.copy()
    np.fill_diagonal(other, -1.0); other[src, tgt] = -1.0; other[tgt, src] = -1.0
    assert other.max() <= 0.633
    Gt = torch.from_numpy(G)
    Sc = R.chain_scores(Gt, Gt)
    assert np.abs(Sc - S).max() < 3.1e-5
    _, _, c_all = R.range_from_scores(Sc, 0.9, 10)
    assert (c_all >= 1).all() and (c_all[planted] == 2).all() and (c_all[~planted] == 1).all()
    s, i, c = RF.range_from_scores(Sc, RF.allow_mask(lab, lab, "ne"), 0.9, 10)
    assert ((c > 0) == planted).all() and (c[planted] == 1).all()
    assert (i[src, 0] == tgt).all() and (i[tgt, 0] == src).all() and (i[:, 1:] == -1).all() and (i[~planted] == -1).all()
    # `eq` asks the opposite question: the same region twice in ONE image; only the self-matches answer
    _, _, c_eq = RF.range_from_scores(Sc, RF.allow_mask(lab, lab, "eq"), 0.9, 10)
    assert (c_eq == 1).all()


# ----------------------------------------------------------------------------------------------------------------------------------
# distributed_search(min_score=...) under gloo: each rank's shard is a test double whose range_search is the restatement; the
# collectives, the packing, the floors' and counts' way through them and both ends of the merge are the product's code.
class _RangeOracleShard:
    def __init__(self, rows, offset, labels=None):
        self.rows, self.offset, self.labels, self.groups = rows, offset, labels, None
        self.calls = []

    def search(self, queries, k):
        raise AssertionError("a range search must not call search")

    def range_search(self, queries, min_score, k, query_labels=None, mode="eq"):
        B = queries.shape[0]
        thr = R.floors(min_score, B)
        self.calls.append((B, query_labels is not None))
        empty_q = (queries == 0).all(dim=1).numpy()
        assert np.isposinf(thr[empty_q]).all(), "a padding slot must carry a floor of +inf"
        if self.rows.shape[0] == 0:
            return torch.full((B, k), float("-inf")), torch.full((B, k), -1, dtype=torch.int64), torch.zeros(B, dtype=torch.int32)
        S = R.chain_scores(queries, self.rows)
        allow = np.ones(S.shape, dtype=bool) if query_labels is None else RF.allow_mask(self.labels, query_labels, mode)
        s, i, c = RF.range_from_scores(S, allow, thr, k, self.offset)
        return torch.from_numpy(s), torch.from_numpy(i), torch.from_numpy(c)


class _NoRangeShard:
    """What a QuantizedShard looks like to distributed_search: rows, an offset, search, no range_search."""

    def __init__(self, rows):
        self.rows, self.offset, self.labels, self.groups = rows, 0, None, torch.zeros(rows.shape[0], dtype=torch.int32)

    def search(self, queries, k, **kw):
        raise AssertionError("refused before any search")


def _same(got, want):
    s, i, c = got
    return (c.dtype == torch.int64 and torch.equal(c, torch.from_numpy(want[2].astype(np.int64))) and torch.equal(i, torch.from_numpy(want[1]))
            and torch.equal(s.view(torch.int32), torch.from_numpy(want[0]).view(torch.int32)))


def _range_worker(rank, world, port, G, rl, Q_all, ql_all, thr_all, k, split, bounds, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from cor_amd import retrieval
        lo, hi = bounds[rank], bounds[rank + 1]                      # (one shard is empty)
        shard = _RangeOracleShard(G[lo:hi], lo, rl[lo:hi])
        qlo, qhi = split[rank], split[rank + 1]                      # ragged per-rank batches with max_local
        cap = max(split[r + 1] - split[r] for r in range(world))
        Q, ql, thr = Q_all[qlo:qhi], ql_all[qlo:qhi], thr_all[qlo:qhi]
        # (1) per-query floors (with +-inf and NaN), no labels, one gather to rank 0
        res = retrieval.distributed_search(Q, shard, k, max_local=cap, min_score=thr)
        assert len(res) == 3 and shard.calls[-1] == (world * cap, False)
        if rank == 0:
            out["plain"] = res
        else:
            assert res == (None, None, None)
        # (2) labels, both modes, dst=None: every rank merges and holds the same answer
        for mode in ("eq", "ne"):
            res = retrieval.distributed_search(Q, shard, k, max_local=cap, dst=None, min_score=thr, query_labels=ql, filter_mode=mode)
            assert shard.calls[-1] == (world * cap, True)
            ref = [res] if rank == 0 else [None]
            dist.broadcast_object_list(ref, src=0)
            assert all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
                       for a, b in zip(ref[0], res))
            if rank == 0:
                out[mode] = res
        # (3) a scalar floor, deferred: the same out of PendingSearch.result(), idempotent; (None, None, None) off the destination
        pend = retrieval.distributed_search(Q, shard, k, max_local=cap, min_score=0.125, query_labels=ql, filter_mode="ne", defer=True, dst=1)
        res = pend.result()
        if rank == 1:
            out["scalar"] = res
            assert pend.result()[2] is res[2]
        else:
            assert res == (None, None, None)
        # (4) the two refusals, on every rank before any collective (a collective entered by some ranks only would hang the others)
        grouped = _RangeOracleShard(G[lo:hi], lo, rl[lo:hi])
        grouped.groups = rl[lo:hi]
        with pytest.raises(ValueError, match="min_score"):
            retrieval.distributed_search(Q, grouped, k, max_local=cap, min_score=0.5, distinct=True)
        with pytest.raises(ValueError, match="int8"):
            retrieval.distributed_search(Q, _NoRangeShard(G[lo:hi]), k, max_local=cap, min_score=0.5)
        # (5) min_score=None: the call and the two-tensor result as they were
        plain_shard = _TopkDouble(G[lo:hi], lo)
        two = retrieval.distributed_search(Q, plain_shard, k, max_local=cap)
        assert len(two) == 2 and plain_shard.kwargs == [{}]
        if rank == 0:
            out["topk"] = two
    finally:
        dist.destroy_process_group()


class _TopkDouble:
    """Records how search is called: without min_score nothing about the call may change."""

    def __init__(self, rows, offset):
        self.rows, self.offset, self.labels, self.groups, self.kwargs = rows, offset, None, None, []

    def search(self, queries, k, **kw):
        self.kwargs.append(kw)
        B = queries.shape[0]
        if self.rows.shape[0] == 0:
            return torch.full((B, k), float("-inf")), torch.full((B, k), -1, dtype=torch.int64)
        s, i, _ = R.range_from_scores(R.chain_scores(queries, self.rows), F(-np.inf), k, self.offset)
        return torch.from_numpy(s), torch.from_numpy(i)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("world,split,bounds", [(2, (0, 4, 6), (0, 700, 700)), (4, (0, 2, 3, 3, 6), (0, 250, 250, 480, 700))],
                         ids=["world2", "world4"])
def test_distributed_range_search_gloo(world, split, bounds):
    """Ragged batches with max_local (world 4: a rank without queries), one empty shard, per-query floors with -inf, +inf and NaN, with
    and without labels, dst=0, dst=1 and dst=None, defer, and the two ValueErrors: lists, and counts summed over the shards, equal the
    restatement over the whole gallery bitwise."""
    rng = np.random.default_rng(3)
    Ng, C, k = 700, 64, 12
    G = torch.from_numpy(_unit(rng.standard_normal((Ng, C))).astype(F))
    G[600] = G[3]                                                                  # a tie across two shards
    Q = torch.from_numpy(_unit(rng.standard_normal((6, C))).astype(F))
    rl = torch.from_numpy(rng.integers(0, 3, Ng).astype(np.int32))
    ql = torch.tensor([0, -1, 2, 1, 5, 0], dtype=torch.int32)                      # 5: an absent class
    S = R.chain_scores(Q, G)
    thr = torch.tensor([-np.inf, 0.1, np.inf, np.nan, 0.0, float(S[5, 3])], dtype=torch.float32)
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_range_worker, args=(world, _free_port(), G, rl, Q, ql, thr, k, split, bounds, out), nprocs=world, join=True)
    tn = thr.numpy()
    free = np.ones(S.shape, dtype=bool)
    want = RF.range_from_scores(S, free, tn, k)
    assert _same(out["plain"], want) and want[2].tolist()[:4] == [Ng, want[2][1], 0, 0] and want[2][5] >= 2
    for mode in ("eq", "ne"):
        want = RF.range_from_scores(S, RF.allow_mask(rl, ql, mode), tn, k)
        assert _same(out[mode], want), mode
        assert want[2][4] == (0 if mode == "eq" else int((S[4] >= 0).sum()))
    assert _same(out["scalar"], RF.range_from_scores(S, RF.allow_mask(rl, ql, "ne"), F(0.125), k))
    ts, ti = out["topk"]
    ws, wi, _ = R.range_from_scores(S, F(-np.inf), k)
    assert torch.equal(ti, torch.from_numpy(wi)) and torch.equal(ts.view(torch.int32), torch.from_numpy(ws).view(torch.int32))

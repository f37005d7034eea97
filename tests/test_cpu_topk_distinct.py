"""CPU side of distinct-group gallery top-k: distributed_search(distinct=True) on gloo worlds of 2 and 4 (each rank's shard is a test
double whose .search(..., distinct=True) is a plain CPU implementation of the definition and which exposes `groups`; everything else is the
product's code), the host merge on hand-made lists, retrieval.groups_of, and the unchanged non-distinct call."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

NINF = float("-inf")


def _distinct_topk(Q, rows, k, offset, groups, row_labels=None, query_labels=None, mode="eq"):
    """The definition on the CPU: rank each query's allowed rows by (score desc, index asc), keep the first row of each group (a negative
    id: the row alone), keep the first k; the tail is (-inf, -1)."""
    B, n = Q.shape[0], rows.shape[0]
    s = torch.full((B, k), NINF)
    i = torch.full((B, k), -1, dtype=torch.int64)
    if n == 0:
        return s, i
    S = Q.float() @ rows.float().T
    allow = torch.ones_like(S, dtype=torch.bool)
    if query_labels is not None:
        ql = torch.as_tensor(query_labels).reshape(-1, 1).long()
        rl = torch.as_tensor(row_labels).reshape(1, -1).long()
        allow = ((rl == ql) if mode == "eq" else (rl != ql)) | (ql < 0)
    order = torch.sort(torch.where(allow, S, torch.full_like(S, NINF)), dim=1, descending=True, stable=True).indices
    for b in range(B):
        seen, m = set(), 0
        for g in order[b].tolist():
            if not allow[b, g]:
                continue
            gid = int(groups[g])
            key = gid if gid >= 0 else ("row", g)
            if key in seen:
                continue
            seen.add(key)
            s[b, m] = S[b, g]; i[b, m] = g + offset; m += 1
            if m == k:
                break
    return s, i


class _DistinctOracleShard:
    def __init__(self, rows, offset, groups):
        self.rows, self.offset, self.groups, self.labels = rows, offset, groups, groups

    def search(self, queries, k, query_labels=None, mode="eq", distinct=False):
        assert distinct
        return _distinct_topk(queries, self.rows, k, self.offset, self.groups, self.labels, query_labels, mode)


class _RecordingShard:
    """No groups, no labels: records how distributed_search calls it."""

    def __init__(self, rows, offset, calls):
        self.rows, self.offset, self.calls = rows, offset, calls

    def search(self, *args, **kwargs):
        self.calls.append((len(args), sorted(kwargs)))
        queries, k = args
        return _distinct_topk(queries, self.rows, k, self.offset, -torch.ones(self.rows.shape[0], dtype=torch.int32))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, G, GR, Q_all, QL_all, k, split, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from cor_amd import retrieval
        lo, hi = retrieval.shard_bounds(G.shape[0], world, rank)
        shard = _DistinctOracleShard(G[lo:hi], lo, GR[lo:hi])
        qlo, qhi = split[rank], split[rank + 1]
        cap = max(split[r + 1] - split[r] for r in range(world))
        q = Q_all[qlo:qhi]
        kw = dict(distinct=True)
        if QL_all is not None:
            kw.update(query_labels=QL_all[qlo:qhi], filter_mode="ne")
        got = {}
        got["dst0"] = retrieval.distributed_search(q, shard, k, max_local=cap, **kw)
        got["dst1"] = retrieval.distributed_search(q, shard, k, max_local=cap, dst=1, **kw)
        got["all"] = retrieval.distributed_search(q, shard, k, max_local=cap, dst=None, **kw)
        got["defer"] = retrieval.distributed_search(q, shard, k, max_local=cap, defer=True, **kw).result()
        out[rank] = got
    finally:
        dist.destroy_process_group()


def _data(Ng, nq, seed):
    """image ids in runs of 1-6 rows (they straddle every shard boundary sooner or later), a few negative ids, some ids far apart"""
    gen = torch.Generator().manual_seed(seed)
    G = torch.nn.functional.normalize(torch.randn((Ng, 256), generator=gen), dim=-1)
    Q = torch.nn.functional.normalize(torch.randn((nq, 256), generator=gen), dim=-1)
    GR = torch.repeat_interleave(torch.arange(Ng), torch.randint(1, 7, (Ng,), generator=gen))[:Ng].to(torch.int32)
    far = torch.randperm(Ng, generator=gen)[:max(Ng // 10, 2)]
    GR[far] = int(GR[far[0]])                                                     # one image with regions in every shard
    GR[torch.randperm(Ng, generator=gen)[:max(Ng // 20, 1)]] = -3                # rows that are groups of their own
    QL = GR[torch.randint(0, Ng, (nq,), generator=gen)].clone()
    QL[0] = GR[far[0]]
    QL[::3] = -1
    return G, GR, Q, QL


# 9 rows over 4 ranks: rank 3's shard is empty; (0, 2, 3, 5, 6): ragged batches, max_local = 2
@pytest.mark.parametrize("world,Ng,k,split", [(2, 600, 20, (0, 3, 6)), (4, 900, 50, (0, 2, 3, 5, 6)), (4, 9, 5, (0, 2, 4, 6, 6))])
@pytest.mark.parametrize("filtered", [False, True])
def test_distributed_search_gloo_distinct(world, Ng, k, split, filtered):
    G, GR, Q, QL = _data(Ng, 6, Ng + k + world)
    # the boundaries do cut groups: some id lives on both sides of a shard boundary
    if Ng >= 600:
        from cor_amd import retrieval
        cuts = [retrieval.shard_bounds(Ng, world, r)[0] for r in range(1, world)]
        assert any(set(GR[:c][GR[:c] >= 0].tolist()) & set(GR[c:][GR[c:] >= 0].tolist()) for c in cuts)
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(world, _free_port(), G, GR, Q, QL if filtered else None, k, split, out), nprocs=world, join=True)
    rs, ri = _distinct_topk(Q, G, k, 0, GR, GR, QL if filtered else None, "ne")
    for rank in range(world):
        got = out[rank]
        for key, owner in (("dst0", 0), ("dst1", 1), ("defer", 0), ("all", rank)):
            s, i = got[key]
            if rank != owner:
                assert s is None and i is None, (key, rank)
                continue
            assert i.shape == (6, k) and s.shape == (6, k)
            assert torch.equal(i, ri), (key, rank)
            fin = torch.isfinite(rs)
            assert torch.equal(torch.isfinite(s), fin) and torch.allclose(s[fin], rs[fin], atol=1e-6)
    # no group twice in any list
    from cor_amd import retrieval
    g_of = retrieval.groups_of(ri, GR)
    for b in range(6):
        ids = [g for g, r in zip(g_of[b].tolist(), ri[b].tolist()) if r >= 0 and g >= 0]
        assert len(ids) == len(set(ids))


def test_merge_topk_distinct_host_on_hand_made_lists():
    from cor_amd.retrieval import merge_topk_distinct_host
    t = lambda *v: torch.tensor([list(v)])
    # shard 0 lists group 7 with a WORSE row (0.5) than shard 1 (0.9): the merge keeps shard 1's; group 2's equal scores in two shards: the
    # lower index wins; the negative ids (-1, -1, -4) are never merged; missing entries are dropped
    s0, i0, g0 = t(0.8, 0.5, 0.3, NINF), t(10, 11, 12, -1), t(2, 7, -1, -1)
    s1, i1, g1 = t(0.9, 0.8, 0.3, 0.2), t(100, 101, 102, 103), t(7, 2, -1, -4)
    s, i = merge_topk_distinct_host([s0, s1], [i0, i1], [g0, g1], 4)
    assert i.tolist() == [[100, 10, 12, 102]] and torch.equal(s, t(0.9, 0.8, 0.3, 0.3))
    s, i = merge_topk_distinct_host([s0, s1], [i0, i1], [g0, g1], 8)         # fewer than k groups: the tail
    assert i.tolist() == [[100, 10, 12, 102, 103, -1, -1, -1]]
    assert s[0, :5].tolist() == pytest.approx([0.9, 0.8, 0.3, 0.3, 0.2]) and torch.isneginf(s[0, 5:]).all()
    s, i = merge_topk_distinct_host([s0, s1], [i0, i1], [g0, g1], 1)
    assert i.tolist() == [[100]]
    # int32 group columns as they come out of the packed lists; an all-missing shard
    s, i = merge_topk_distinct_host([s0, torch.full((1, 2), NINF)], [i0, torch.full((1, 2), -1)], [g0.int(), torch.full((1, 2), -1).int()], 3)
    assert i.tolist() == [[10, 11, 12]]


def test_groups_of():
    from cor_amd.retrieval import groups_of
    groups = torch.tensor([5, 5, 9, -2, 7], dtype=torch.int32)
    idx = torch.tensor([[4, 0, -1], [3, 2, 1]])
    assert groups_of(idx, groups).tolist() == [[7, 5, -1], [-2, 9, 5]]
    from cor_amd.retrieval import recall_at_k
    assert recall_at_k(groups_of(idx, groups), [5, 5], ks=(1, 2)) == {1: 0.0, 2: 0.5}


def _worker_plain(rank, world, port, G, Q_all, k, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from cor_amd import retrieval
        lo, hi = retrieval.shard_bounds(G.shape[0], world, rank)
        calls, packed = [], []
        shard = _RecordingShard(G[lo:hi], lo, calls)
        pack = retrieval._pack_lists

        def spy(s, i):
            p = pack(s, i)
            packed.append(tuple(p.shape))
            return p
        retrieval._pack_lists = spy
        s, i = retrieval.distributed_search(Q_all[3 * rank:3 * rank + 3], shard, k, dst=None, distinct=False)
        out[rank] = (calls, packed, i)
    finally:
        dist.destroy_process_group()


def test_non_distinct_call_keeps_its_packing_and_its_two_argument_search():
    G, _, Q, _ = _data(200, 6, 7)
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker_plain, args=(2, _free_port(), G, Q, 10, out), nprocs=2, join=True)
    want = torch.sort(Q @ G.T, dim=1, descending=True, stable=True).indices[:, :10]
    for rank in range(2):
        calls, packed, i = out[rank]
        assert calls == [(2, [])]                                               # shard.search(slots, k): two positional arguments
        assert packed == [(6, 10, 3)]                                           # [slots, k, 3] int32, no group column
        assert torch.equal(i, want)


def test_distinct_needs_group_ids():
    from cor_amd import retrieval
    G, _, Q, _ = _data(50, 2, 3)
    with pytest.raises(ValueError):
        retrieval.distributed_search(Q, _RecordingShard(G, 0, []), 5, distinct=True)


def test_threshold_kernel_never_gets_more_sample_values_than_it_sorts():
    """The plan is host code: for every shard size, the filtered 16-bit plan included (whose slice count grows with Ng), the threshold
    kernel is handed at most the 4096 sample values its LDS sort holds."""
    from cor_amd import _native as nat
    lib = nat.load()
    for Ng in (4097, 100000, 1000000, 8400000, 9000000, 21000000, 33600000, 50000000, 500000000, 2000000000):
        for Bq in (1, 32, 300, 512, 2048):
            for k in (1, 10, 32, 64, 100, 255, 256):
                n = lib.cor_topk_distinct_sample_values(Bq, Ng, k)
                assert 0 < n <= 4096, (Bq, Ng, k, n)
    assert lib.cor_topk_distinct_sample_values(8, 4096, 10) == 0              # a tiny shard: no sample pass
    assert lib.cor_topk_distinct_sample_values(8, 5000, 257) == nat.EINVAL

"""CPU side of wide-k retrieval (k up to 256): the multi-rank search path at k = 100 / 256 (gloo world 4; each rank's shard is a
test double whose .search() is the CPU oracle, everything else is the product's code) and retrieval.recall_at_k."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp


class _OracleShard:
    def __init__(self, rows, offset):
        self.rows, self.offset = rows, offset

    def search(self, queries, k):
        from oracle import retrieval as oret
        if self.rows.shape[0] == 0:                                   # empty shard: all-missing lists
            return torch.full((queries.shape[0], k), float("-inf")), torch.full((queries.shape[0], k), -1, dtype=torch.int64)
        s, i = oret.similarity_topk(queries, self.rows, min(k, self.rows.shape[0]))
        i = i + self.offset
        if s.shape[1] < k:                                            # pad like the kernel does (score -inf, index -1)
            pad = k - s.shape[1]
            s = torch.cat([s, torch.full((s.shape[0], pad), float("-inf"))], 1)
            i = torch.cat([i, torch.full((i.shape[0], pad), -1, dtype=torch.int64)], 1)
        return s, i


def _worker(rank, world, port, G, Q_all, k, split, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from cor_amd import retrieval
        lo, hi = retrieval.shard_bounds(G.shape[0], world, rank)
        shard = _OracleShard(G[lo:hi], lo)
        qlo, qhi = split[rank], split[rank + 1]
        cap = max(split[r + 1] - split[r] for r in range(world))
        s, i = retrieval.distributed_search(Q_all[qlo:qhi], shard, k, max_local=cap)
        if rank == 0:
            out["s"], out["i"] = s, i
        else:
            assert s is None and i is None
        s2, i2 = retrieval.distributed_search(Q_all[qlo:qhi], shard, k, max_local=cap, dst=None)
        ref = [(out["s"], out["i"])] if rank == 0 else [None]
        dist.broadcast_object_list(ref, src=0)
        assert torch.equal(ref[0][1], i2) and torch.equal(ref[0][0], s2)
    finally:
        dist.destroy_process_group()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


# (9 rows over 4 ranks: shard_bounds gives rank 3 the empty range [9, 9); 1000 and 700 rows: every shard holds fewer rows than k = 256)
@pytest.mark.parametrize("Ng,k,split", [(1000, 100, (0, 2, 3, 5, 6)), (700, 256, (0, 3, 3, 5, 6)), (9, 100, (0, 2, 4, 6, 6)),
                                        (9, 256, (0, 1, 2, 3, 6))])
def test_distributed_search_world4_gloo_wide_k(Ng, k, split):
    from oracle import retrieval as oret
    from cor_amd import retrieval
    assert Ng > 100 or retrieval.shard_bounds(Ng, 4, 3)[0] == retrieval.shard_bounds(Ng, 4, 3)[1]
    gen = torch.Generator().manual_seed(Ng + k)
    G = torch.nn.functional.normalize(torch.randn((Ng, 256), generator=gen), dim=-1)
    if Ng > 600:
        G[Ng - 1] = G[3]                                  # a tie across shards
    Q = torch.nn.functional.normalize(torch.randn((6, 256), generator=gen), dim=-1)
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(4, _free_port(), G, Q, k, split, out), nprocs=4, join=True)
    kk = min(k, Ng)
    rs, ri = oret.similarity_topk(Q, G, kk)
    assert out["i"].shape == (6, k) and out["s"].shape == (6, k)
    assert torch.equal(out["i"][:, :kk], ri) and torch.allclose(out["s"][:, :kk], rs, atol=1e-6)
    if k > Ng:
        assert (out["i"][:, Ng:] == -1).all() and torch.isneginf(out["s"][:, Ng:]).all()


def test_recall_at_k_single_positive():
    from cor_amd.retrieval import recall_at_k
    idx = torch.tensor([[5, 3, 9, 7], [1, 2, 3, 4], [7, 8, 9, 10], [0, 11, 12, 13]])
    r = recall_at_k(idx, [3, 4, 99, 0], ks=(1, 2, 4))
    assert r == {1: 0.25, 2: 0.5, 4: 0.75}
    assert recall_at_k(idx, torch.tensor([3, 4, 99, 0]), ks=(1, 2, 4)) == r


def test_recall_at_k_sets_of_positives():
    from cor_amd.retrieval import recall_at_k
    idx = torch.tensor([[5, 3, 9, 7], [1, 2, 3, 4]])
    assert recall_at_k(idx, [{9, 3}, {4, 100}], ks=(1, 2, 3, 4)) == {1: 0.0, 2: 0.5, 3: 0.5, 4: 1.0}
    assert recall_at_k(idx, [[7], set()], ks=(4,)) == {4: 0.5}          # a query without positives never hits


def test_recall_at_k_missing_entries():
    """-1 marks a missing entry (a shard smaller than k): it is never a hit, not even against a positive id of -1."""
    from cor_amd.retrieval import recall_at_k
    idx = torch.tensor([[2, -1, -1], [-1, -1, -1]])
    assert recall_at_k(idx, [2, -1], ks=(1, 3)) == {1: 0.5, 3: 0.5}


def test_recall_at_k_rejects_K_beyond_the_lists():
    from cor_amd.retrieval import recall_at_k
    idx = torch.zeros((3, 50), dtype=torch.int64)
    with pytest.raises(ValueError):
        recall_at_k(idx, [0, 1, 2])                                     # default ks reach 100 > 50
    assert recall_at_k(idx, [0, 1, 2], ks=(1, 5, 10, 50)) == {1: 1 / 3, 5: 1 / 3, 10: 1 / 3, 50: 1 / 3}

"""CPU side of filtered gallery top-k: distributed_search with query labels on gloo worlds of 2 and 4 (each rank's shard is a test double
whose .search() is a filtered CPU oracle; everything else is the product's code), the unchanged two-argument shard call without labels,
and dataloader.gallery_labels."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def _filtered_topk(Q, rows, k, offset, row_labels=None, query_labels=None, mode="eq"):
    """CPU oracle: the top-k allowed rows per query by (score desc, global index asc); the tail is (-inf, -1)."""
    B, n = Q.shape[0], rows.shape[0]
    s = torch.full((B, k), float("-inf"))
    i = torch.full((B, k), -1, dtype=torch.int64)
    if n == 0:
        return s, i
    S = Q.float() @ rows.float().T
    if query_labels is not None:
        ql = torch.as_tensor(query_labels).reshape(-1, 1).long()
        rl = torch.as_tensor(row_labels).reshape(1, -1).long()
        allow = ((rl == ql) if mode == "eq" else (rl != ql)) | (ql < 0)
        S = torch.where(allow, S, torch.full_like(S, float("-inf")))
    else:
        allow = torch.ones_like(S, dtype=torch.bool)
    order = torch.sort(S, dim=1, descending=True, stable=True).indices[:, :k]     # ties: ascending row order
    kk = order.shape[1]
    ok = torch.gather(allow, 1, order)
    s[:, :kk] = torch.where(ok, torch.gather(S, 1, order), s[:, :kk])
    i[:, :kk] = torch.where(ok, order + offset, i[:, :kk])
    return s, i


class _FilteredOracleShard:
    def __init__(self, rows, offset, labels):
        self.rows, self.offset, self.labels = rows, offset, labels

    def search(self, queries, k, query_labels=None, mode="eq"):
        return _filtered_topk(queries, self.rows, k, self.offset, self.labels, query_labels, mode)


class _RecordingShard:
    """No labels anywhere: records how distributed_search calls it."""

    def __init__(self, rows, offset, calls):
        self.rows, self.offset, self.calls = rows, offset, calls

    def search(self, *args, **kwargs):
        self.calls.append((len(args), sorted(kwargs)))
        queries, k = args
        return _filtered_topk(queries, self.rows, k, self.offset)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, G, RL, Q_all, QL_all, k, split, mode, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from cor_amd import retrieval
        lo, hi = retrieval.shard_bounds(G.shape[0], world, rank)
        shard = _FilteredOracleShard(G[lo:hi], lo, RL[lo:hi])
        qlo, qhi = split[rank], split[rank + 1]
        cap = max(split[r + 1] - split[r] for r in range(world))
        q, ql = Q_all[qlo:qhi], QL_all[qlo:qhi]
        got = {}
        got["dst0"] = retrieval.distributed_search(q, shard, k, max_local=cap, query_labels=ql, filter_mode=mode)
        got["dst1"] = retrieval.distributed_search(q, shard, k, max_local=cap, dst=1, query_labels=ql, filter_mode=mode)
        got["all"] = retrieval.distributed_search(q, shard, k, max_local=cap, dst=None, query_labels=ql, filter_mode=mode)
        got["defer"] = retrieval.distributed_search(q, shard, k, max_local=cap, query_labels=ql, filter_mode=mode, defer=True).result()
        out[rank] = got
    finally:
        dist.destroy_process_group()


def _data(Ng, nq, seed, layout):
    gen = torch.Generator().manual_seed(seed)
    G = torch.nn.functional.normalize(torch.randn((Ng, 256), generator=gen), dim=-1)
    Q = torch.nn.functional.normalize(torch.randn((nq, 256), generator=gen), dim=-1)
    if layout == "classes":
        RL = torch.randint(0, 4, (Ng,), generator=gen, dtype=torch.int32)
        QL = torch.randint(0, 5, (nq,), generator=gen, dtype=torch.int32)      # label 4: a class no row carries
    else:                                                                       # image ids: runs of 1-2 rows
        RL = (torch.cumsum(torch.randint(0, 2, (Ng,), generator=gen), 0)).to(torch.int32)
        QL = RL[torch.randint(0, Ng, (nq,), generator=gen)].clone()
    QL[::3] = -1                                                                # unrestricted queries mixed in
    return G, RL, Q, QL


# 9 rows over 4 ranks: rank 3's shard is empty; (0, 2, 3, 5, 6): ragged batches, max_local = 2
@pytest.mark.parametrize("world,Ng,k,split", [(2, 600, 20, (0, 3, 6)), (4, 900, 50, (0, 2, 3, 5, 6)), (4, 9, 5, (0, 2, 4, 6, 6))])
@pytest.mark.parametrize("mode,layout", [("eq", "classes"), ("ne", "runs"), ("ne", "classes")])
def test_distributed_search_gloo_filtered(world, Ng, k, split, mode, layout):
    G, RL, Q, QL = _data(Ng, 6, Ng + k + world, layout)
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(world, _free_port(), G, RL, Q, QL, k, split, mode, out), nprocs=world, join=True)
    rs, ri = _filtered_topk(Q, G, k, 0, RL, QL, mode)
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
    if mode == "eq" and layout == "classes":
        assert (ri[QL.long() == 4] == -1).all()                                 # an absent class: only the tail


def _worker_nolabels(rank, world, port, G, Q_all, k, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from cor_amd import retrieval
        lo, hi = retrieval.shard_bounds(G.shape[0], world, rank)
        calls = []
        shard = _RecordingShard(G[lo:hi], lo, calls)
        s, i = retrieval.distributed_search(Q_all[3 * rank:3 * rank + 3], shard, k, dst=None)
        out[rank] = (calls, i)
    finally:
        dist.destroy_process_group()


def test_distributed_search_without_labels_calls_search_with_two_arguments():
    G, _, Q, _ = _data(200, 6, 7, "classes")
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker_nolabels, args=(2, _free_port(), G, Q, 10, out), nprocs=2, join=True)
    _, ri = _filtered_topk(Q, G, 10, 0)
    for rank in range(2):
        calls, i = out[rank]
        assert calls == [(2, [])]
        assert torch.equal(i, ri)
    from cor_amd import retrieval                                               # one process, no process group: the same call
    calls = []
    retrieval.distributed_search(Q, _RecordingShard(G, 0, calls), 10)
    assert calls == [(2, [])]


def test_gallery_labels_follow_the_csv_row_order(tmp_path):
    import pandas as pd
    from cor_amd import dataloader
    rows = []
    for j, (img, tgt, compose) in enumerate([("a.jpg", "car", 0), ("a.jpg", "dog", 0), ("b.jpg", "car", 1), ("c.jpg", "cat", 0),
                                             ("b.jpg", "dog", 0), ("c.jpg", "car", 0)]):
        rows.append(dict(Id=j, Query_img=img, Query_mask=f"m{j}.png", Support_img="s.jpg", Support_mask="sm.png", Text="t", Compose=compose,
                         Dataset="D", Target=tgt, query_cat="x"))
    csv = tmp_path / "pairs.csv"
    pd.DataFrame(rows).to_csv(csv, index=False)
    df = dataloader.read_pairs_csv(str(csv))                                    # the rows gallery_batches yields, in its order
    lab, names = dataloader.gallery_labels(str(csv))
    assert lab.dtype == torch.int32 and lab.tolist() == [0, 1, 2, 1, 0]
    assert names == ["car", "dog", "cat"]
    assert [names[v] for v in lab.tolist()] == df["Target"].tolist()
    img, img_names = dataloader.gallery_labels(str(csv), column="Query_img")
    assert img.tolist() == [0, 0, 1, 2, 1] and img_names == ["a.jpg", "c.jpg", "b.jpg"]
    assert [img_names[v] for v in img.tolist()] == df["Query_img"].tolist()
    with pytest.raises(ValueError):
        dataloader.gallery_labels(str(csv), column="Nope")

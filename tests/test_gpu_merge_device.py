"""Device merge of top-k lists (cor_merge_topk -> ops.merge_topk -> retrieval.merge_topk_device / GallerySet /
distributed_search(merge="device")) on the GPU. Everything is compared BITWISE, scores on their int32 view so that -0.0 is seen; the
references are retrieval.merge_topk_host / merge_topk_distinct_host on CPU copies of the same lists (the definition) and, in one test,
an independent restatement in plain Python."""
import socket

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NEG_INF = float("-inf")
BIG = 5 * 10 ** 9                                  # global ids beyond 32 bits


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _lists(P, B, kin, seed):
    """CPU lists [P,B,kin] built to hit the ordering rules: scores out of five values (ties cross list borders), indices a random
    permutation per query shifted past 2^32, every list sorted as a search returns it with a (-inf, -1) tail of random length;
    query 0: a present entry whose score is -inf and (P >= 3) a list that is entirely missing; query 1 (B >= 3): every list missing;
    the last query (B >= 2) scores with +0.0 and -0.0, holding a +0.0 in list 0 and a -0.0 in list 1 whatever is drawn, and draws its groups from three ids (fewer than k groups: the tail). Group ids repeat
    across and within lists, negative ids repeat, missing entries carry garbage ids."""
    rng = np.random.default_rng(seed)
    N = P * kin
    s = np.full((P, B, kin), -np.inf, dtype=np.float32)
    i = np.full((P, B, kin), -1, dtype=np.int64)
    g = rng.choice(np.array([0, 1, -1, -5, 2 ** 31 - 1, -2 ** 31, 7]), size=(P, B, kin)).astype(np.int32)     # garbage where missing
    for b in range(B):
        if B >= 3 and b == 1:
            continue
        last = b == B - 1 and B >= 2
        values = np.array([0.5, 0.0, -0.0, -0.25, -1.0] if last else [0.75, 0.5, 0.25, -0.125, -1.5], dtype=np.float32)
        ids = rng.permutation(N).astype(np.int64) + BIG
        for p in range(P):
            if b == 0 and P >= 3 and p == P - 1:
                continue
            n = kin if (p == 0 and b == 0) else int(rng.integers(0, kin + 1))
            if last and p < 2:
                n = max(n, 1)
            sc = values[rng.integers(0, 5, size=n)]
            ix = ids[p * kin:p * kin + n]
            if last and p < 2:
                sc[0] = values[1 + p]                                  # +0.0 in list 0, -0.0 in list 1, whatever the draw gives
            if b == 0 and p == 0 and n > 1:
                sc[0] = -np.inf                                        # present, and still ahead of every missing entry
            order = sorted(range(n), key=lambda e: (-float(sc[e]), int(ix[e])))
            s[p, b, :n], i[p, b, :n] = sc[order], ix[order]
            pool = 3 if last else max(2, N // 3)
            gr = rng.integers(0, pool, size=n)
            if not last:
                neg = rng.random(n) < 0.25
                gr[neg] = -1 - rng.integers(0, 3, size=int(neg.sum()))
            g[p, b, :n] = gr
    return torch.from_numpy(s), torch.from_numpy(i), torch.from_numpy(g)


def _host(s, i, g, k):
    """The definition on CPU lists; the plain host merge returns min(k, N) columns: the rest is the tail."""
    from cor_amd import retrieval
    if g is not None:
        return retrieval.merge_topk_distinct_host(list(s), list(i), list(g), k)
    hs, hi = retrieval.merge_topk_host(list(s), list(i), k)
    pad = k - hs.shape[1]
    if pad > 0:
        hs = torch.cat([hs, torch.full((hs.shape[0], pad), NEG_INF)], 1)
        hi = torch.cat([hi, torch.full((hi.shape[0], pad), -1, dtype=torch.int64)], 1)
    return hs, hi


def _lookup(s, i, g, out_i):
    """groups_of-style lookup: the group id the input lists give each output row id (-1 for missing)."""
    out = torch.full(out_i.shape, -1, dtype=torch.int32)
    for b in range(out_i.shape[0]):
        table = {int(x): int(y) for x, y in zip(i[:, b].reshape(-1), g[:, b].reshape(-1)) if x >= 0}
        for c in range(out_i.shape[1]):
            if out_i[b, c] >= 0:
                out[b, c] = table[int(out_i[b, c])]
    return out


CASES = [(1, 1, 1, 1), (1, 2, 5, 3), (2, 1, 1, 1), (2, 3, 4, 4), (3, 4, 7, 5), (4, 2, 10, 64), (8, 33, 10, 10), (8, 5, 256, 256), (16, 2, 256, 256)]


@pytest.mark.parametrize("distinct", [False, True], ids=["plain", "distinct"])
@pytest.mark.parametrize("P,B,kin,k", CASES)
def test_merge_kernel_equals_the_host_merge(P, B, kin, k, distinct):
    from cor_amd import ops
    s, i, g = _lists(P, B, kin, seed=1000 * P + kin)
    want = _host(s, i, g if distinct else None, k)
    got = ops.merge_topk(s.to(DEV), i.to(DEV), k, g.to(DEV) if distinct else None)
    torch.cuda.synchronize()
    assert len(got) == (3 if distinct else 2) and got[0].is_cuda
    got = [t.cpu() for t in got]
    assert torch.equal(got[1], want[1]) and _bits_equal(got[0], want[0])
    if distinct:
        assert torch.equal(got[2], _lookup(s, i, g, got[1]))


def test_merge_kernel_equals_an_independent_restatement():
    """Not only the product's own host code: rank the present entries with Python's sorted over (-score, index) tuples (-0.0 == 0.0
    there too), keep the first entry of every non-negative group, cut to k."""
    from cor_amd import ops
    P, B, kin, k = 3, 4, 7, 12
    s, i, g = _lists(P, B, kin, seed=77)
    ps, pi = ops.merge_topk(s.to(DEV), i.to(DEV), k)
    ds, di, dg = ops.merge_topk(s.to(DEV), i.to(DEV), k, g.to(DEV))
    torch.cuda.synchronize()
    for b in range(B):
        ent = [(float(s[p, b, e]), int(i[p, b, e]), int(g[p, b, e])) for p in range(P) for e in range(kin) if i[p, b, e] >= 0]
        ranked = sorted(ent, key=lambda t: (-t[0], t[1]))
        seen, first = set(), []
        for t in ranked:
            if t[2] < 0 or t[2] not in seen:
                first.append(t)
            seen.add(t[2])
        for got_s, got_i, got_g, ref in ((ps, pi, None, ranked), (ds, di, dg, first)):
            ref = (ref + [(NEG_INF, -1, -1)] * k)[:k]
            assert got_i[b].tolist() == [t[1] for t in ref], b
            assert _bits_equal(got_s[b].cpu(), torch.tensor([t[0] for t in ref], dtype=torch.float32)), b
            if got_g is not None:
                assert got_g[b].tolist() == [t[2] for t in ref], b
    zeros = s[:, -1].reshape(-1).view(torch.int32)
    assert (zeros == -2 ** 31).any() and (zeros == 0).any()            # the last query ranked both zeros


@pytest.mark.parametrize("distinct", [False, True], ids=["plain", "distinct"])
@pytest.mark.parametrize("P,B", [(17, 1), (40, 2)])
def test_merge_beyond_one_launch_goes_by_rounds(P, B, distinct):
    from cor_amd import ops, retrieval, _native
    kin = k = 256
    s, i, g = _lists(P, B, kin, seed=P)
    sd, idd, gd = s.to(DEV), i.to(DEV), g.to(DEV)
    if P == 17:
        with pytest.raises(_native.NativeError, match="no kernel for this shape"):
            ops.merge_topk(sd, idd, k, gd if distinct else None)
    want = _host(s, i, g if distinct else None, k)
    got = retrieval.merge_topk_device(list(sd), list(idd), k, list(gd) if distinct else None)
    torch.cuda.synchronize()
    assert torch.equal(got[1].cpu(), want[1]) and _bits_equal(got[0].cpu(), want[0])
    if distinct:
        assert torch.equal(got[2].cpu(), _lookup(s, i, g, want[1]))


def test_merge_topk_device_pads_unequal_lists():
    from cor_amd import retrieval
    s, i, g = _lists(3, 4, 9, seed=5)
    parts = [(s[0], i[0], g[0]), (s[1][:, :4], i[1][:, :4], g[1][:, :4].long()), (s[2][:, :1], i[2][:, :1], g[2][:, :1])]
    for grp in (False, True):
        args = ([p[0] for p in parts], [p[1] for p in parts])
        want = (retrieval.merge_topk_distinct_host(*args, [p[2] for p in parts], 6) if grp else retrieval.merge_topk_host(*args, 6))
        got = retrieval.merge_topk_device([t.to(DEV) for t in args[0]], [t.to(DEV) for t in args[1]], 6,
                                          [p[2].to(DEV) for p in parts] if grp else None)
        assert torch.equal(got[1].cpu(), want[1]) and _bits_equal(got[0].cpu(), want[0])
    es, ei = retrieval.merge_topk_device([s[0][:0].to(DEV)], [i[0][:0].to(DEV)], 3)           # no queries: empty lists
    assert tuple(es.shape) == (0, 3) and tuple(ei.shape) == (0, 3)


# ---- GallerySet end to end ---------------------------------------------------------------------------------------------------------

BOUNDS = (0, 1000, 1001, 3000)
SEARCHES = {"plain": {}, "eq": dict(filtered="eq"), "ne": dict(filtered="ne"), "distinct": dict(distinct=True),
            "distinct_ne": dict(distinct=True, filtered="ne")}


@pytest.fixture(scope="module")
def gallery():
    """3000 unit rows (C = 256, bf16) with exact duplicates planted across the segment borders 1000 | 1001, groups in runs of 1-8 rows
    that straddle them, 33 queries (the first ones close to the duplicated rows), and the single-shard answers, computed ONCE."""
    from cor_amd import retrieval
    rng = np.random.default_rng(2024)
    G = torch.nn.functional.normalize(torch.from_numpy(rng.standard_normal((3000, 256), dtype=np.float32)), dim=-1).to(torch.bfloat16)
    for a, b in ((999, 1000), (998, 1001), (5, 2500), (1000, 1700), (997, 1002)):
        G[b] = G[a]
    runs = rng.integers(1, 9, size=3000)
    groups = torch.from_numpy(np.repeat(np.arange(3000), runs)[:3000].astype(np.int32))
    groups[996:1004] = groups[996]                                    # one run of 8 rows across both borders
    groups[40:44] = -3                                                # negative ids: every row a group of its own
    labels = torch.from_numpy(rng.integers(0, 4, size=3000).astype(np.int32))
    Q = torch.from_numpy(rng.standard_normal((33, 256), dtype=np.float32))
    for n, row in enumerate((999, 998, 5, 1000, 997, 41)):
        Q[n] = G[row].float() + 0.05 * Q[n]
    Q = torch.nn.functional.normalize(Q, dim=-1).to(DEV)
    qlab = torch.from_numpy(rng.integers(-1, 4, size=33).astype(np.int32)).to(DEV)
    G = G.to(DEV)
    whole = retrieval.GalleryShard(G, offset=70, labels=labels, groups=groups)

    def run(shard, k, filtered=None, distinct=False):
        return shard.search(Q, k, query_labels=qlab if filtered else None, mode=filtered or "eq", distinct=distinct)

    want = {(name, k): tuple(t.cpu() for t in run(whole, k, **kw)) for name, kw in SEARCHES.items() for k in (10, 100)}
    torch.cuda.synchronize()
    return dict(G=G, Q=Q, qlab=qlab, labels=labels, groups=groups, run=run, want=want)


def _segments(gal, dtypes=(None, None, None), with_meta=True):
    from cor_amd import retrieval
    return [retrieval.GalleryShard(gal["G"][lo:hi], offset=70 + lo, dtype=dt, labels=gal["labels"][lo:hi] if with_meta else None,
                                   groups=gal["groups"][lo:hi] if with_meta else None)
            for lo, hi, dt in zip(BOUNDS[:-1], BOUNDS[1:], dtypes)]


@pytest.mark.parametrize("k", [10, 100])
@pytest.mark.parametrize("name", list(SEARCHES))
def test_gallery_set_equals_one_shard_over_all_rows(gallery, name, k):
    """Segments of 1000 / 1 / 1999 rows (the 1-row segment returns Ng < k tail lists) against ONE GalleryShard over the 3000 rows."""
    from cor_amd import retrieval
    gs = retrieval.GallerySet(_segments(gallery))
    assert len(gs) == 3000 and [len(x) for x in gs.segments] == [1000, 1, 1999]
    s, i = gallery["run"](gs, k, **SEARCHES[name])
    torch.cuda.synchronize()
    ws, wi = gallery["want"][(name, k)]
    assert s.is_cuda and i.is_cuda
    assert torch.equal(i.cpu(), wi) and _bits_equal(s.cpu(), ws)


def test_gallery_set_of_mixed_dtypes_add_and_drop(gallery):
    from cor_amd import retrieval
    Q = gallery["Q"]
    segs = _segments(gallery, dtypes=(torch.float16, torch.float32, torch.float16))
    gs = retrieval.GallerySet(segs)
    per = [x.search(Q, 10) for x in segs]
    ws, wi = retrieval.merge_topk_host([p[0].cpu() for p in per], [p[1].cpu() for p in per], 10)
    s, i = gs.search(Q, 10)
    assert torch.equal(i.cpu(), wi) and _bits_equal(s.cpu(), ws)
    per = [x.search(Q, 10, distinct=True) for x in segs]
    ws, wi = retrieval.merge_topk_distinct_host([p[0].cpu() for p in per], [p[1].cpu() for p in per],
                                                [retrieval.groups_of(p[1].cpu() - 70, gallery["groups"]) for p in per], 10)
    s, i = gs.search(Q, 10, distinct=True)
    assert torch.equal(i.cpu(), wi) and _bits_equal(s.cpu(), ws)
    # add a segment of new rows, then drop it: the earlier results come back; a single segment's result is returned untouched
    before = [t.cpu() for t in gs.search(Q, 10)]
    extra = retrieval.GalleryShard(gallery["G"][:50].to(torch.float16), offset=10 ** 7, labels=gallery["labels"][:50], groups=gallery["groups"][:50])
    gs.add(extra)
    grown = gs.search(Q, 10)[1].cpu()
    assert len(gs) == 3050 and (grown >= 10 ** 7).any()
    assert gs.drop(10 ** 7) is extra and len(gs) == 3000
    after = [t.cpu() for t in gs.search(Q, 10)]
    assert torch.equal(before[1], after[1]) and _bits_equal(before[0], after[0])
    one = retrieval.GallerySet([segs[0], retrieval.GalleryShard(gallery["G"][:0], offset=5000, labels=gallery["labels"][:0], groups=gallery["groups"][:0])])
    s1, i1 = one.search(Q, 10)
    s0, i0 = segs[0].search(Q, 10)
    assert torch.equal(i1, i0) and _bits_equal(s1.cpu(), s0.cpu())


def test_distributed_search_device_merge_on_a_one_rank_rccl_group(gallery):
    """merge="device" against merge="host" on the real backend, as the one-rank RCCL test of test_gpu_parity.py sets it up: plain and
    distinct, with and without defer, dst=0 and dst=None, max_local larger than the local batch (dropped slots), a filter, and once
    with a two-segment GallerySet as the shard."""
    import torch.distributed as dist
    from cor_amd import retrieval
    if dist.is_initialized():
        pytest.skip("a process group already exists in this process")
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]
    dev = torch.device(DEV)
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=dev)
    try:
        Q, qlab = gallery["Q"][:5], gallery["qlab"][:5]
        whole = retrieval.GalleryShard(gallery["G"], offset=70, labels=gallery["labels"], groups=gallery["groups"])
        segs = _segments(gallery)
        pair = retrieval.GallerySet([segs[0], segs[2]])
        common = dict(max_local=8, always_collective=True)
        for shard in (whole, pair):
            for kw in (dict(), dict(distinct=True), dict(dst=None), dict(distinct=True, dst=None, query_labels=qlab, filter_mode="ne")):
                hs, hi = retrieval.distributed_search(Q, shard, 10, merge="host", **common, **kw)
                ds, di = retrieval.distributed_search(Q, shard, 10, merge="device", **common, **kw)
                ps, pi = retrieval.distributed_search(Q, shard, 10, merge="device", defer=True, **common, **kw).result()
                assert tuple(hi.shape) == (5, 10) and not di.is_cuda
                for s_, i_ in ((ds, di), (ps, pi)):
                    assert torch.equal(i_, hi) and _bits_equal(s_, hs), (shard is pair, kw.keys())
        ws, wi = gallery["want"][("distinct", 10)]
        ds, di = retrieval.distributed_search(Q, whole, 10, merge="device", distinct=True, **common)
        assert torch.equal(di, wi[:5]) and _bits_equal(ds, ws[:5])
        assert dist.get_backend() == "nccl"
    finally:
        dist.destroy_process_group()

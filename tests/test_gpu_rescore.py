"""GPU tests of the candidate re-scoring (cor_rescore_topk, ops.rescore_topk, GalleryShard / GallerySet .rescore, two_stage_search).
Every comparison is bitwise, on scores, indices and positions. The reference is the CPU definition: range test and first occurrence
per id, the fmaf chain of oracle/c/sim_chain.c (sim_chain_pairs) on the operands the GPU multiplies (16-bit galleries: the query rounded
to the gallery dtype, the rows widened), then a sort by (score desc, id asc)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
INT64_MIN = -2 ** 63


def _chain_pairs(Qn, Gn, qi, gi):
    from oracle import retrieval as oret
    lib = oret._chain_lib()
    fp, ip = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_longlong)
    lib.sim_chain_pairs.argtypes = [fp, fp, ip, ip, ctypes.c_longlong, ctypes.c_int, fp]
    lib.sim_chain_pairs.restype = None
    qi, gi = np.ascontiguousarray(qi, dtype=np.int64), np.ascontiguousarray(gi, dtype=np.int64)
    out = np.empty(qi.shape[0], dtype=np.float32)
    lib.sim_chain_pairs(Qn.ctypes.data_as(fp), Gn.ctypes.data_as(fp), qi.ctypes.data_as(ip), gi.ctypes.data_as(ip), qi.shape[0], Qn.shape[1],
                        out.ctypes.data_as(fp))
    return out


class _Ref:
    """The CPU definition for one (query operands, row operands, candidate lists, offset): ranked once, cut to any k."""

    def __init__(self, Qm, Gm, cand, g_offset=0):
        Qn, Gn = np.ascontiguousarray(Qm.float().cpu().numpy()), np.ascontiguousarray(Gm.float().cpu().numpy())
        c = cand.cpu().numpy()
        Bq, Ng = c.shape[0], Gn.shape[0]
        present = (c >= g_offset) & (c < g_offset + Ng)
        first = np.zeros_like(present)
        for b in range(Bq):
            first[b, np.unique(c[b], return_index=True)[1]] = True
        present &= first
        qi, pj = np.nonzero(present)
        ids = c[qi, pj]
        sc = _chain_pairs(Qn, Gn, qi, ids - g_offset)
        starts = np.searchsorted(qi, np.arange(Bq + 1))
        self.lists = []
        for b in range(Bq):
            sl = slice(starts[b], starts[b + 1])
            order = np.lexsort((ids[sl], -sc[sl].astype(np.float64)))          # score desc (-0.0 ties +0.0), then id asc
            self.lists.append((sc[sl][order], ids[sl][order], pj[sl][order]))

    def top(self, k):
        Bq = len(self.lists)
        s = np.full((Bq, k), -np.inf, dtype=np.float32); i = np.full((Bq, k), -1, dtype=np.int64); p = np.full((Bq, k), -1, dtype=np.int32)
        for b, (ls, li, lp) in enumerate(self.lists):
            n = min(k, ls.shape[0])
            s[b, :n], i[b, :n], p[b, :n] = ls[:n], li[:n], lp[:n]
        return torch.from_numpy(s), torch.from_numpy(i), torch.from_numpy(p)


def _same(got, want, what=""):
    gs, gi = got[0].cpu(), got[1].cpu()
    assert torch.equal(gi, want[1]), f"indices differ {what}"
    assert torch.equal(gs.view(torch.int32), want[0].view(torch.int32)), f"score bits differ {what}"
    if len(got) > 2:
        assert got[2].dtype == torch.int32 and torch.equal(got[2].cpu(), want[2]), f"positions differ {what}"


def _unit(n, C, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn((n, C), generator=g), dim=-1)


@pytest.fixture(scope="module")
def gallery():
    """5 000 unit rows and 37 unit queries per width, on the host; never modified."""
    return {C: (_unit(5000, C, 11 + C), _unit(37, C, 12 + C), _unit(37, C, 13 + C)) for C in (64, 128, 256)}


@pytest.mark.parametrize("C", [256, 64, 128])
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_search_list_comes_back_unchanged(gallery, dtype, C):
    from cor_amd.retrieval import GalleryShard
    G, Q, _ = gallery[C]
    shard = GalleryShard(G.to(DEV), offset=1000, dtype=dtype)
    q = Q.to(DEV)
    ks = (1, 10, 32, 100, 256) if C == 256 or dtype == torch.float32 else (33, 100)    # 16-bit, C != 256, k <= 32: no chain promise
    gen = torch.Generator().manual_seed(5)
    for k in ks:
        s, i = shard.search(q, k)
        rs, ri, rp = shard.rescore(q, i, k, return_pos=True)
        want = (s.cpu(), i.cpu(), torch.arange(k, dtype=torch.int32).expand(37, k))
        _same((rs, ri, rp), want, f"k={k}")
        assert shard.rescore(q, i)[1].shape == (37, min(k, 256))                        # k defaults to min(kin, 256)
        perm = torch.stack([torch.randperm(k, generator=gen) for _ in range(37)])
        ps, pi, pp = shard.rescore(q, torch.gather(i, 1, perm.to(DEV)), k, return_pos=True)
        _same((ps, pi, pp), (want[0], want[1], torch.argsort(perm, dim=1).to(torch.int32)), f"permuted, k={k}")


@pytest.mark.parametrize("C", [16, 64, 256])
@pytest.mark.parametrize("dtype", DTYPES)
def test_against_the_cpu_chain(dtype, C):
    """Random candidate lists (not search results) with ids a little outside the shard and, by chance and at kin > Ng by necessity,
    repeats. k = 256 > kin and k > the number of present entries check the tail."""
    from cor_amd import ops
    Ng, off = 3000, 77
    G = _unit(Ng, C, 100 + C).to(dtype)
    gen = torch.Generator().manual_seed(200 + C)
    Gd = G.to(DEV)
    for Bq in (1, 70):
        Q = _unit(Bq, C, 300 + Bq)
        Qd = Q.to(DEV)
        for kin in (1, 33, 100, 257, 1000, 4096):
            cand = torch.randint(off - 40, off + Ng + 40, (Bq, kin), generator=gen)
            ref = _Ref(Q.to(dtype), G, cand, off)
            cd = cand.to(DEV)
            for k in (1, 7, 256):
                _same(ops.rescore_topk(Qd, Gd, cd, k, g_offset=off, return_pos=True), ref.top(k), f"Bq={Bq} kin={kin} k={k}")
            s, i = ops.rescore_topk(Qd, Gd, cd, 7, g_offset=off)                         # without positions
            _same((s, i), ref.top(7))


@pytest.mark.parametrize("g_offset", [0, 2 ** 33 + 5])
@pytest.mark.parametrize("dtype", DTYPES)
def test_missing_and_hostile_ids(dtype, g_offset):
    from cor_amd import ops
    Ng, C, Bq, kin = 3000, 64, 9, 40
    G, Q = _unit(Ng, C, 21).to(dtype), _unit(Bq, C, 22)
    gen = torch.Generator().manual_seed(23)
    hostile = torch.tensor([-1, -7, g_offset - 1, g_offset + Ng, 2 ** 40, INT64_MIN, 2 ** 63 - 1, g_offset + Ng + 2 ** 32, g_offset - 2 ** 32])
    cand = g_offset + torch.randint(0, Ng, (Bq, kin), generator=gen)
    bad = torch.rand((Bq, kin), generator=gen) < 0.4
    cand = torch.where(bad, hostile[torch.randint(0, hostile.shape[0], (Bq, kin), generator=gen)], cand)
    cand[3] = hostile[torch.arange(kin) % hostile.shape[0]]                              # a list without a single valid id
    cand[4, 1:] = hostile[0]
    cand[4, 0] = g_offset + Ng - 1                                                       # the shard's last row alone
    cand[5, -1] = g_offset                                                               # and its first
    ref = _Ref(Q.to(dtype), G, cand, g_offset)
    assert len(ref.lists[3][0]) == 0 and len(ref.lists[4][0]) == 1
    for k in (1, 16, 256):
        got = ops.rescore_topk(Q.to(DEV), G.to(DEV), cand.to(DEV), k, g_offset=g_offset, return_pos=True)
        torch.cuda.synchronize()                                                          # a HIP error would surface here
        _same(got, ref.top(k), f"k={k}")
    assert torch.equal(got[1][3].cpu(), torch.full((256,), -1, dtype=torch.int64))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_duplicates_and_ties(dtype):
    from cor_amd import ops
    Ng, C, Bq = 400, 64, 6
    G, Q = _unit(Ng, C, 31), _unit(Bq, C, 32)
    G[100:164] = G[100].clone()                                                          # 64 copies of one row: tied scores
    G = G.to(dtype)
    gen = torch.Generator().manual_seed(33)
    # ids repeated 2..50 times inside a list
    base = torch.randint(0, Ng, (Bq, 24), generator=gen)
    reps = torch.randint(2, 51, (Bq, 24), generator=gen)
    lists = []
    for b in range(Bq):
        l = torch.repeat_interleave(base[b], reps[b])
        lists.append(l[torch.randperm(l.shape[0], generator=gen)][:700])
    kin = min(l.shape[0] for l in lists)
    cand = torch.stack([l[:kin] for l in lists])
    ref = _Ref(Q.to(dtype), G, cand)
    for k in (5, 64):
        got = ops.rescore_topk(Q.to(DEV), G.to(DEV), cand.to(DEV), k, return_pos=True)
        _same(got, ref.top(k), f"repeats, k={k}")
        i, p = got[1].cpu(), got[2].cpu()
        for b in range(Bq):
            live = i[b][i[b] >= 0]
            assert live.unique().shape[0] == live.shape[0]                                # every id once
            for r in range(live.shape[0]):
                assert int(p[b, r]) == int((cand[b] == live[r]).nonzero()[0])            # at its first occurrence
    # the 64 copies, arriving in descending id order among other rows: ascending id order out
    cand = torch.cat([torch.arange(199, 59, -1), torch.arange(100, 164)]).expand(Bq, -1).contiguous()
    ref = _Ref(Q.to(dtype), G, cand)
    got = ops.rescore_topk(Q.to(DEV), G.to(DEV), cand.to(DEV), 140, return_pos=True)
    _same(got, ref.top(140), "tied rows")
    for b in range(Bq):
        run = [int(x) for x in got[1][b].cpu() if 100 <= int(x) < 164]
        assert run == list(range(100, 164))
        at = got[1][b].cpu().tolist().index(100)
        assert got[1][b, at:at + 64].cpu().tolist() == run                                # one block of equal scores
        assert got[0][b, at:at + 64].cpu().view(torch.int32).unique().shape[0] == 1
    # all-zero rows (+0.0 and -0.0 stored) against queries with negative entries: +-0.0 scores tie, the id decides, bits as computed
    Z = torch.zeros((50, C))
    Z[::3] = -0.0
    Z = Z.to(dtype)
    Qn = -Q.abs()
    cand = torch.stack([torch.randperm(50, generator=gen) for _ in range(Bq)])
    ref = _Ref(Qn.to(dtype), Z, cand)
    got = ops.rescore_topk(Qn.to(DEV), Z.to(DEV), cand.to(DEV), 50, return_pos=True)
    _same(got, ref.top(50), "zero scores")
    assert torch.equal(got[1].cpu(), torch.arange(50).expand(Bq, 50)) and bool((got[0] == 0).all())


def test_two_stages(gallery):
    from cor_amd.retrieval import GalleryShard, two_stage_search
    from oracle import retrieval as oret
    G, Q, Q2 = gallery[256]
    Gb = G.to(torch.bfloat16)
    groups = torch.arange(5000, dtype=torch.int32) // 3
    labels = torch.arange(5000, dtype=torch.int32) % 7
    coarse = GalleryShard(Gb.to(DEV), labels=labels, groups=groups)
    fine = GalleryShard(G.to(DEV))
    q, q2 = Q.to(DEV), Q2.to(DEV)
    _, ci = oret.similarity_topk_chain(Q.to(torch.bfloat16).float(), Gb.float(), 100)
    _same(two_stage_search(q, coarse, fine, 10, 100), _Ref(Q, G, ci).top(10)[:2], "bf16 coarse, fp32 fine")
    _same(two_stage_search(q, coarse, fine, 10, 100, fine_queries=q2), _Ref(Q2, G, ci).top(10)[:2], "a second query vector")
    _same(two_stage_search(q, coarse, fine, 100, 100), _Ref(Q, G, ci).top(100)[:2], "k = k_coarse")
    ql = torch.arange(37, dtype=torch.int32) % 7
    ql[5] = -1
    for kw in (dict(query_labels=ql.to(DEV), mode="ne"), dict(distinct=True), dict(query_labels=ql.to(DEV), mode="eq", distinct=True)):
        _, si = coarse.search(q, 100, **kw)                                               # the coarse stage is the corresponding search
        got = two_stage_search(q, coarse, fine, 10, 100, **kw)
        _same(got, _Ref(Q, G, si.cpu()).top(10)[:2], str(sorted(kw)))                     # and the second stage only re-orders its rows
        gi = got[1].cpu()
        if "mode" in kw and kw["mode"] == "ne":
            assert bool(((labels[gi] != ql[:, None]) | (ql[:, None] < 0)).all())
        if kw.get("distinct"):
            assert all(groups[gi[b]].unique().shape[0] == 10 for b in range(37))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_gallery_set_rescore(gallery, dtype):
    from cor_amd.retrieval import GalleryShard, GallerySet
    G, Q, _ = gallery[256]
    G = G.to(DEV).to(dtype)
    q = Q.to(DEV)
    # segments [0, 1000), [1000, 3500), a gap [3500, 3600) with an empty segment in it, [3600, 5100): 1 500 rows
    tail = torch.cat([G[3600:], G[:100]])
    segs = {"a": GalleryShard(G[:1000], 0), "e": GalleryShard(G[:0], 3500), "b": GalleryShard(G[1000:3500], 1000),
            "c": GalleryShard(tail, 3600)}
    assert [len(s) for s in segs.values()] == [1000, 0, 2500, 1500]
    gs = GallerySet([segs["c"], segs["a"]])
    gs.add(segs["b"]); gs.add(segs["e"])                                                  # out of order
    whole = GalleryShard(torch.cat([G[:3600], tail]), 0)                                  # rows 3500..3599 exist here only
    gen = torch.Generator().manual_seed(41)
    cand = torch.randint(-20, 5200, (37, 300), generator=gen)
    cand[:, 7] = 3550                                                                     # an id in the gap, in every list
    masked = torch.where((cand >= 3500) & (cand < 3600), torch.full_like(cand, -1), cand)
    for k in (10, 256):
        got = gs.rescore(q, cand.to(DEV), k)
        want = whole.rescore(q, masked.to(DEV), k)
        _same(got, (want[0].cpu(), want[1].cpu()), f"k={k}")
        assert got[0].device == q.device and not bool((got[1] == 3550).any())
    one = GallerySet([segs["e"], segs["b"]])                                              # one live segment: its result as it is
    _same(one.rescore(q, cand.to(DEV), 10), tuple(t.cpu() for t in segs["b"].rescore(q, cand.to(DEV), 10)))
    s, i = GallerySet([segs["e"]]).rescore(q, cand.to(DEV), 10)                           # none
    assert s.is_cuda and bool((s == float("-inf")).all()) and bool((i == -1).all()) and s.shape == i.shape == (37, 10)
    s, i, p = segs["e"].rescore(q, cand.to(DEV), return_pos=True)                         # an empty shard: all missing, k = min(kin, 256)
    assert s.shape == (37, 256) and bool((s == float("-inf")).all()) and bool((i == -1).all()) and bool((p == -1).all())
    s, i = segs["a"].rescore(q[:0], cand[:0].to(DEV), 5)                                  # no queries
    assert s.shape == i.shape == (0, 5) and s.is_cuda


def test_stream_and_device(gallery):
    from cor_amd import ops
    G, Q, _ = gallery[64]
    Gd, q = G.to(DEV).to(torch.float16), Q.to(DEV)
    cand = torch.randint(-5, 5005, (37, 500), generator=torch.Generator().manual_seed(51)).to(DEV)
    want = ops.rescore_topk(q, Gd, cand, 20, return_pos=True)
    torch.cuda.synchronize()
    st = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(st):
        got = ops.rescore_topk(q, Gd, cand, 20, return_pos=True)
    st.synchronize()
    _same(got, tuple(t.cpu() for t in want))
    assert all(t.device == q.device for t in got)

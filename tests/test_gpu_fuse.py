"""GPU tests of the list fusion (cor_fuse_lists, ops.fuse_lists, retrieval.fuse_lists_device, retrieval.fused_search). Every comparison is
bitwise, on score bits (so that +-0 are seen), ids and counts. The reference is the CPU restatement of the definition, tests/fuse_refs.py."""
import functools

import numpy as np
import pytest
import torch

from tests.fuse_refs import F, ref_fuse

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(1, 1, 1, 1), (1, 2, 4096, 256), (2, 3, 4, 4), (3, 4, 7, 5), (4, 2, 10, 64), (5, 3, 100, 256), (8, 33, 10, 10), (16, 2, 256, 256)]
COMBOS = [("rrf", "none", "zero"), ("sum", "none", "zero"), ("sum", "none", "floor"), ("sum", "minmax", "zero"), ("sum", "minmax", "floor"),
          ("max", "none", "zero"), ("max", "minmax", "zero")]
WEIGHTS = [0.5, 1.0, 0.0, -0.25, 2.0]


def _bits(x):
    x = torch.as_tensor(x).cpu()
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def _same(got, want, what=""):
    """got: the GPU's tuple (scores, idx[, count]); want: ref_fuse's three arrays (or tensors)."""
    names = ("score bits", "ids", "counts")
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.int64 and (len(got) < 3 or got[2].dtype == torch.int32)
    for n, g in enumerate(got):
        assert torch.equal(_bits(g), _bits(want[n])), f"{names[n]} differ {what}"


@functools.lru_cache(maxsize=None)
def hostile_lists(P, Bq, kin):
    """Seeded lists built to hit the rules: ids drawn per query from a pool of about n / 3 ids shifted past 2^32 (most ids occur in several
    lists, and again inside a list), a forced repeat inside every list, holes (idx -1) in the middle, present entries with -inf, +inf
    and NaN, scores out of five values (fused ties are frequent and the id decides); Bq >= 3: query 1 has only +-0.0 scores; list P - 1
    of query 2 (Bq >= 4) or else of query 0 (P >= 3) has one score throughout; P >= 2: list 1 of query 0 is missing entirely; Bq >= 2:
    the last query has every list missing. -> (scores f32 [P,Bq,kin], idx i64 [P,Bq,kin], weights), NumPy, never modified."""
    rng = np.random.default_rng(1000 * P + 10 * Bq + kin)
    n = P * kin
    pool = max(2, n // 3)
    idx = np.empty((P, Bq, kin), np.int64)
    for b in range(Bq):
        ids = rng.choice(10 * pool, pool, replace=False).astype(np.int64) + 2 ** 32 + 7
        idx[:, b] = ids[rng.integers(0, pool, (P, kin))]
    scores = rng.choice(np.array([0.25, 0.5, 1.0, -0.75, 2.0], F), (P, Bq, kin))
    if kin >= 2:
        idx[:, :, kin - 1] = idx[:, :, 0]                              # a repeat inside every list, with a score of its own
    if Bq >= 3:
        scores[:, 1] = rng.choice(np.array([0.0, -0.0], F), (P, kin))
    if Bq >= 4 or P >= 3:
        scores[P - 1, 2 if Bq >= 4 else 0] = F(0.5)
    bad = rng.random((P, Bq, kin)) < 0.06
    scores[bad] = rng.choice(np.array([-np.inf, np.inf, np.nan], F), int(bad.sum()))
    idx[rng.random((P, Bq, kin)) < 0.1] = -1
    if P >= 2:
        idx[1, 0] = -1
    if Bq >= 2:
        idx[:, Bq - 1] = -1
    scores.setflags(write=False)
    idx.setflags(write=False)
    return scores, idx, [WEIGHTS[p % len(WEIGHTS)] for p in range(P)]


@pytest.mark.parametrize("mode,normalize,missing", COMBOS)
@pytest.mark.parametrize("P,Bq,kin,k", SHAPES)
def test_kernel_against_the_restatement(P, Bq, kin, k, mode, normalize, missing):
    from cor_amd import ops
    scores, idx, w = hostile_lists(P, Bq, kin)
    want = ref_fuse(scores, idx, w, mode, 60.0, normalize, missing, k)
    s, i = torch.tensor(scores, device=DEV), torch.tensor(idx, device=DEV)
    kw = dict(weights=w, mode=mode, rrf_c=60.0, normalize=normalize, missing=missing)
    _same(ops.fuse_lists(s, i, k, return_count=True, **kw), want, "with the counts")
    got = ops.fuse_lists(s, i, k, **kw)
    assert len(got) == 2
    _same(got, want[:2], "without the counts")
    if Bq >= 2:
        assert (want[1][Bq - 1] == -1).all() and np.isneginf(want[0][Bq - 1]).all() and (want[2][Bq - 1] == -1).all()
    if P * kin > 3:
        assert (want[1][0, 0] >= 0) and not np.isnan(want[0]).any()    # (the draw is not vacuous)


@pytest.mark.parametrize("rrf_c,w", [(0.0, [1.0, 1.0, 1.0]), (1.5, [2.0, -1.0, 0.5]), (60.0, [0.0, 0.0, 0.0])])
def test_rrf_constants_and_weights(rrf_c, w):
    from cor_amd import ops
    scores, idx, _ = hostile_lists(3, 4, 7)
    want = ref_fuse(scores, idx, w, "rrf", rrf_c, "none", "zero", 9)
    _same(ops.fuse_lists(torch.tensor(scores, device=DEV), torch.tensor(idx, device=DEV), 9, weights=w, rrf_c=rrf_c, return_count=True), want)


@pytest.fixture(scope="module")
def gallery():
    """3 000 unit rows per width on the host and 3 noisy views of 24 requests; never modified."""
    out = {}
    for C in (64, 256):
        g = torch.Generator().manual_seed(70 + C)
        G = torch.nn.functional.normalize(torch.randn((3000, C), generator=g), dim=-1)
        t = torch.randperm(3000, generator=g)[:24]
        views = torch.stack([torch.nn.functional.normalize(G[t] + 1.5 * torch.randn((24, C), generator=g) / C ** 0.5, dim=-1) for _ in range(3)])
        out[C] = (G, views)
    return out


def test_one_list_comes_back_and_copies_keep_the_order(gallery):
    from cor_amd import ops
    from cor_amd.retrieval import GalleryShard
    G, views = gallery[64]
    for shard, kin in ((GalleryShard(G.to(DEV), offset=2 ** 33), 100), (GalleryShard(G[:40].to(DEV), offset=5), 64)):   # the second: a (-inf, -1) tail
        s, i = shard.search(views[0].to(DEV), kin)
        # P = 1, SUM, weight 1, none, zero: the list itself, a -0.0 score as +0.0
        got = ops.fuse_lists(s[None], i[None], kin, weights=[1.0], mode="sum", return_count=True)
        present = (i >= 0).to(torch.int32)
        _same(got, (torch.where(s == 0, torch.zeros_like(s), s), i, present * 2 - 1), f"one list, kin={kin}")
        # RRF of P copies of one list keeps its order
        for P in (2, 5):
            fs, fi, fc = ops.fuse_lists(s[None].expand(P, -1, -1), i[None].expand(P, -1, -1), kin, return_count=True)
            assert torch.equal(fi, i) and torch.equal(fc, torch.where(i >= 0, P, -1).to(torch.int32))
            assert (fs[:, :-1] >= fs[:, 1:]).all()


def test_fuse_lists_device_pads_unequal_lists(gallery):
    from cor_amd import ops, retrieval
    from cor_amd.retrieval import GalleryShard
    G, views = gallery[256]
    shard = GalleryShard(G.to(DEV, torch.bfloat16), offset=1000)
    res = [shard.search(views[p].to(DEV), kk) for p, kk in enumerate((50, 7, 128))]
    s = torch.full((3, 24, 128), float("-inf"), device=DEV)
    i = torch.full((3, 24, 128), -1, dtype=torch.int64, device=DEV)
    for p, (sp, ip) in enumerate(res):
        s[p, :, :sp.shape[1]], i[p, :, :ip.shape[1]] = sp, ip
    for kw in (dict(), dict(mode="sum", normalize="minmax", missing="floor", weights=[1.0, 0.5, 2.0]), dict(mode="max", weights=[1.0, 1.1, 0.9])):
        got = retrieval.fuse_lists_device([r[0] for r in res], [r[1] for r in res], 60, return_count=True, **kw)
        _same(got, ops.fuse_lists(s, i, 60, return_count=True, **kw), str(kw))
        want = ref_fuse(s.cpu().numpy(), i.cpu().numpy(), kw.get("weights", [1, 1, 1]), kw.get("mode", "rrf"), 60.0, kw.get("normalize", "none"),
                        kw.get("missing", "zero"), 60)
        _same(got, want, f"{kw} against the restatement")
    same = retrieval.fuse_lists_device([res[0][0], res[0][0]], [res[0][1], res[0][1]], 50)      # equal k_i: no padding
    assert torch.equal(same[1], res[0][1])


def _restated(res, k, weights=None, mode="rrf", rrf_c=60.0, normalize="none", missing="zero"):
    """The restatement applied to CPU copies of the individual search results."""
    s = np.stack([r[0].cpu().numpy() for r in res])
    i = np.stack([r[1].cpu().numpy() for r in res])
    return ref_fuse(s, i, [1.0] * len(res) if weights is None else weights, mode, rrf_c, normalize, missing, k)[:2]


def test_fused_search_three_views_over_one_shard(gallery):
    from cor_amd import retrieval
    from cor_amd.retrieval import GalleryShard
    for C in (64, 256):
        G, views = gallery[C]
        shard = GalleryShard(G.to(DEV), offset=2 ** 32)
        q = views.to(DEV)
        res = [shard.search(q[p], 50) for p in range(3)]
        _same(retrieval.fused_search(q, shard, 20, 50), _restated(res, 20), f"C={C} rrf, stacked views")
        kw = dict(weights=[1.0, 0.5, 0.25], mode="sum", normalize="minmax", missing="floor")
        _same(retrieval.fused_search(list(q), shard, 256, 50, **kw), _restated(res, 256, **kw), f"C={C} sum")
        kw = dict(mode="max", rrf_c=1.0)
        _same(retrieval.fused_search(list(q), [shard] * 3, 10, 50, **kw), _restated(res, 10, **kw), f"C={C} max")


def test_fused_search_two_galleries_over_one_id_space(gallery):
    from cor_amd import retrieval
    from cor_amd.retrieval import GalleryShard, QuantizedGallery
    G, views = gallery[256]
    fp32 = GalleryShard(G.to(DEV), offset=77)
    i8 = fp32.quantized().gallery()
    assert isinstance(i8, QuantizedGallery)
    q = views[:2].to(DEV)
    res = [fp32.search(q[0], 100), i8.search(q[1], 100)]
    for kw in (dict(), dict(mode="sum", weights=[1.0, 0.5]), dict(mode="sum", normalize="minmax", missing="floor"), dict(mode="max", normalize="minmax")):
        _same(retrieval.fused_search(q, [fp32, i8], 30, 100, **kw), _restated(res, 30, **kw), str(kw))


def test_fused_search_over_a_gallery_set_with_labels(gallery):
    from cor_amd import retrieval
    from cor_amd.retrieval import GallerySet, GalleryShard
    G, views = gallery[64]
    lab = (torch.arange(3000) % 5).to(torch.int32)
    both = GallerySet([GalleryShard(G[:1700].to(DEV), offset=0, labels=lab[:1700]),
                       GalleryShard(G[1700:].to(DEV, torch.float16), offset=1700, labels=lab[1700:])])
    q = views.to(DEV)
    ql = (torch.arange(24) % 5).to(torch.int32)
    for skw, mkw in ((dict(query_labels=ql), dict(query_labels=ql)), (dict(query_labels=ql, filter_mode="ne"), dict(query_labels=ql, mode="ne"))):
        res = [both.search(q[p], 40, **mkw) for p in range(3)]
        _same(retrieval.fused_search(q, both, 40, 40, **skw), _restated(res, 40), str(skw))
        keep = (lab[res[0][1].cpu().clamp(min=0)] == ql[:, None]) == ("filter_mode" not in skw)
        assert keep[res[0][1].cpu() >= 0].all()                        # the filter reached the searches
        kw = dict(mode="sum", normalize="minmax", weights=[0.2, 0.3, 0.5])
        _same(retrieval.fused_search(q, both, 10, 40, **kw, **skw), _restated(res, 10, **kw), f"{skw} {kw}")


def test_side_stream_and_captured_graph():
    """A side stream, and a capture on a single stream that is replayed twice with the same bits and once more with new lists: the weights
    travel in the kernel arguments, nothing is allocated or copied at launch."""
    from cor_amd import ops
    sa, ia, w = hostile_lists(5, 3, 100)
    sb, ib, _ = hostile_lists(5, 3, 100)
    sb, ib = np.ascontiguousarray(sb[::-1]), np.ascontiguousarray(ib[::-1])      # the lists in the opposite order
    kw = dict(weights=w, mode="sum", normalize="minmax", missing="floor", return_count=True)
    want_a = ref_fuse(sa, ia, w, "sum", 60.0, "minmax", "floor", 64)
    want_b = ref_fuse(sb, ib, w, "sum", 60.0, "minmax", "floor", 64)
    dsa, dia = torch.tensor(sa, device=DEV), torch.tensor(ia, device=DEV)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = ops.fuse_lists(dsa, dia, 64, **kw)
    side.synchronize()
    _same(got, want_a, "side stream")
    sin, iin = dsa.clone(), dia.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                      # one capture stream
        out = ops.fuse_lists(sin, iin, 64, **kw)
    for n in (1, 2):
        graph.replay()
        torch.cuda.synchronize()
        _same(out, want_a, f"replay {n}")
    sin.copy_(torch.from_numpy(sb))
    iin.copy_(torch.from_numpy(ib))
    graph.replay()
    torch.cuda.synchronize()
    _same(out, want_b, "replay with new lists")

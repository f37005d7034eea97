"""GPU tests of the list stages over int8 galleries: cor_dequantize_rows_i8, cor_rescore_topk_i8, cor_expand_queries_sq, their fronts in
cor_amd/ops.py and the QuantizedGallery / GallerySet methods built on them. Every comparison is bitwise, on score bits, ids and positions.
The references are the NumPy restatements of tests/i8_list_refs.py, which never call the code under test; the compositions of the Python
layer are compared with the calls they are made of."""
import numpy as np
import pytest
import torch

from tests.i8_list_refs import RefRescore, ref_dequantize, ref_expand_sq
from tests.i8_refs import F, ref_quantize, ref_search

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
INT64_MIN, INT64_MAX = -2 ** 63, 2 ** 63 - 1
BIG = 2 ** 33 + 5


def _unit(n, C, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn((n, C), generator=g), dim=-1)


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({4: torch.int32, 2: torch.int16, 1: torch.int8, 8: torch.int64}[t.element_size()])


def _eq(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _same_lists(got, want, what=""):
    assert torch.equal(got[1].cpu(), want[1].cpu()), f"indices differ {what}"
    assert torch.equal(_bits(got[0]), _bits(want[0])), f"score bits differ {what}"
    if len(got) > 2:
        assert got[2].dtype == torch.int32 and torch.equal(got[2].cpu(), want[2].cpu()), f"positions differ {what}"


@pytest.fixture(scope="module")
def gal():
    """Per width: 5 000 unit rows quantised on the host by the restatement, 130 unit queries; never modified."""
    out = {}
    for C in (16, 64, 128, 256):
        G, Q = _unit(5000, C, 21 + C), _unit(130, C, 22 + C)
        gq, gs = ref_quantize(G)
        out[C] = (torch.from_numpy(gq), torch.from_numpy(gs), Q)
    return out


# ---- dequantise --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", [16, 48, 128, 256])
@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 4097])
def test_dequantize_bitwise(n, C):
    from cor_amd import ops
    rng = np.random.default_rng(n * 1000 + C)
    q = rng.integers(-127, 128, (n, C)).astype(np.int8)
    scale = rng.uniform(1e-4, 0.05, n).astype(F)
    if n:
        q[n - 1] = np.where(np.arange(C) % 3 == 0, -127, 127)                                  # the all-+-127 row
        scale[0] = 0.0                                                                          # a zero-scale row
    qd, sd = torch.from_numpy(q).to(DEV), torch.from_numpy(scale).to(DEV)
    for dt in DTYPES:
        got = ops.dequantize_rows_i8(qd, sd, out_dtype=dt)
        assert _eq(got.cpu(), ref_dequantize(q, scale, dt)), f"{dt}"
        out = torch.full((n, C), 7.0, dtype=dt, device=DEV)
        assert ops.dequantize_rows_i8(qd, sd, out_dtype=dt, out=out) is out and _eq(out, got)
    if n > 1:
        assert (ops.dequantize_rows_i8(qd, sd)[0] == 0).all()


def test_dequantize_fp16_rounds_the_rounded_product():
    """q * s lies just above the midpoint of two fp16 values and rounds (fp32) onto it: rounding that again gives the even neighbour,
    1.0; one rounding of the exact product (a fused multiply-convert) would give 1 + 2^-10."""
    from cor_amd import ops
    H = 1.0 + 2.0 ** -11
    qv, s = next((v, np.float32(H / v)) for v in range(3, 128, 2)
                 if v * float(np.float32(H / v)) > H and np.float32(v * float(np.float32(H / v))) == np.float32(H))
    exact = qv * float(s)                                                                       # exact in float64 (7 + 24 bits)
    assert np.float16(exact).view(np.int16) == 0x3C01 and np.float16(np.float32(exact)).view(np.int16) == 0x3C00   # the two disagree here
    q = np.zeros((2, 16), np.int8)
    q[0, 0], q[0, 5], q[1, 15] = qv, -qv, qv
    scale = np.array([s, s], F)
    got = ops.dequantize_rows_i8(torch.from_numpy(q).to(DEV), torch.from_numpy(scale).to(DEV), out_dtype=torch.float16).cpu()
    assert _eq(got, ref_dequantize(q, scale, torch.float16))
    b = got.view(torch.int16)
    assert b[0, 0].item() == 0x3C00 and b[0, 5].item() == 0x3C00 - 0x8000 and b[1, 15].item() == 0x3C00


# ---- rescore -----------------------------------------------------------------------------------------------------------------------

RESCORE_CASES = [  # kin, C, Bq, offset: every kin, C, Bq and offset of the issue's list occurs
    (1, 16, 5, 0), (3, 64, 1, BIG), (64, 128, 130, 0), (65, 256, 5, BIG), (100, 256, 130, 0), (256, 64, 5, 0), (257, 16, 130, BIG),
    (1024, 256, 5, 0), (4096, 128, 5, BIG), (4096, 256, 1, 0)]


@pytest.mark.parametrize("kin,C,Bq,offset", RESCORE_CASES)
def test_rescore_bitwise(gal, kin, C, Bq, offset):
    from cor_amd import ops
    gq, gs, Q = gal[C]
    Q, Ng = Q[:Bq], gq.shape[0]
    rng = np.random.default_rng(kin + C)
    cand = rng.integers(offset - 40, offset + Ng + 40, (Bq, kin)).astype(np.int64)             # repeats and ids of no row among them
    cand[0, : kin // 2] = cand[0, kin - kin // 2:]                                              # ... and many repeats in one list
    ref = RefRescore(Q, gq, gs, cand, offset)
    qd, gd, sd, cd = Q.to(DEV), gq.to(DEV), gs.to(DEV), torch.from_numpy(cand).to(DEV)
    for k in (1, 10, 256):                                                                      # k above the number of present entries too
        _same_lists(ops.rescore_topk_i8(qd, gd, sd, cd, k, g_offset=offset, return_pos=True), ref.top(k), f"k={k}")
    assert len(ops.rescore_topk_i8(qd, gd, sd, cd, 10, g_offset=offset)) == 2


@pytest.mark.parametrize("C", [16, 64, 128, 256])
def test_rescore_returns_a_search_list_unchanged(gal, C):
    from cor_amd.retrieval import QuantizedGallery
    gq, gs, Q = gal[C]
    qs = QuantizedGallery(gq.to(DEV), gs.to(DEV), offset=1000)
    q = Q.to(DEV)
    gen = torch.Generator().manual_seed(C)
    for k in (1, 10, 256):
        s, i = qs.search(q, k)
        _same_lists((s, i), [torch.from_numpy(x) for x in ref_search(Q, gq.numpy(), gs.numpy(), k, 1000)], f"search k={k}")
        want = (s, i, torch.arange(k, dtype=torch.int32).expand(130, k))
        _same_lists(qs.rescore(q, i, k, return_pos=True), want, f"k={k}")
        assert qs.rescore(q, i)[1].shape == (130, k)                                            # k defaults to min(kin, 256)
        perm = torch.stack([torch.randperm(k, generator=gen) for _ in range(130)])
        got = qs.rescore(q, torch.gather(i, 1, perm.to(DEV)), k, return_pos=True)
        _same_lists(got, (s, i, torch.argsort(perm, dim=1).to(torch.int32)), f"shuffled, k={k}")


@pytest.mark.parametrize("offset", [0, BIG])
def test_rescore_hostile_lists_one_row_shard_and_zero_query(gal, offset):
    from cor_amd import ops
    gq, gs, Q = gal[64]
    gq, gs, Ng, o = gq[:50], gs[:50], 50, offset
    cand = torch.tensor([
        [o + 3, o + 4, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1],
        [o + Ng, o - 1, o + 7, o + 10 ** 12, 5 - o, o + 8, INT64_MIN, INT64_MAX, o + 9, -2, o + Ng - 1, o],
        [INT64_MIN, INT64_MAX, INT64_MIN + 1, INT64_MAX - 1, o + 2 ** 31, o + 2 ** 32, o - 2 ** 32, -1, -1, -1, -1, o + 1],
        [o + 5, o + 5, o + 6, o + 5, o + 6, o + 5, o + 5, o + 5, o + 5, o + 5, o + 5, o + 5],
        [-1] * 12,
        [o + Ng, o + Ng + 1, o - 1, o - 2, INT64_MAX, INT64_MIN, -1, -1, -1, -1, -1, -1],
        [o + 11, o + 10, o + 9, o + 8, o + 7, o + 6, o + 5, o + 4, o + 3, o + 2, o + 1, o]], dtype=torch.int64)
    Qh = Q[:7].clone()
    Qh[6] = 0                                                                                   # a zero query: every score +0.0, the id decides
    ref = RefRescore(Qh, gq, gs, cand, o)
    for k in (1, 5, 12, 20):
        _same_lists(ops.rescore_topk_i8(Qh.to(DEV), gq.to(DEV), gs.to(DEV), cand.to(DEV), k, g_offset=o, return_pos=True), ref.top(k), f"k={k}")
    got = ops.rescore_topk_i8(Qh.to(DEV), gq.to(DEV), gs.to(DEV), cand.to(DEV), 12, g_offset=o)
    assert got[1][6].cpu().tolist() == list(range(o, o + 12)) and (got[0][6] == 0).all() and (got[1][4] == -1).all()
    # a shard of ONE row; an empty one
    one = ops.rescore_topk_i8(Qh.to(DEV), gq[:1].to(DEV), gs[:1].to(DEV), cand.to(DEV), 3, g_offset=o, return_pos=True)
    _same_lists(one, RefRescore(Qh, gq[:1], gs[:1], cand, o).top(3), "Ng=1")
    assert one[1][1, 0].item() == o and one[2][1, 0].item() == 11
    none = ops.rescore_topk_i8(Qh.to(DEV), gq[:0].to(DEV), gs[:0].to(DEV), cand.to(DEV), 3, g_offset=o, return_pos=True)
    assert (none[1] == -1).all() and torch.isinf(none[0]).all() and (none[2] == -1).all()


def test_rescore_plus_and_minus_zero_scores_tie_and_the_id_decides():
    """Hand-made scales of zero: (float)d * qscale keeps d's sign, times 0.0 gives +0.0 or -0.0. The list kernels compare them as equal
    floats and the id decides (the search would rank every +0.0 first); the score bits go out as computed."""
    from cor_amd import ops
    rng = np.random.default_rng(5)
    gq = rng.integers(-127, 128, (40, 64)).astype(np.int8)
    gs = np.where(np.arange(40) % 4 == 0, 0.01, 0.0).astype(F)
    Q = _unit(6, 64, 9)
    cand = np.stack([rng.permutation(40) for _ in range(6)]).astype(np.int64)
    ref = RefRescore(Q, gq, gs, cand, 0)
    got = ops.rescore_topk_i8(Q.to(DEV), torch.from_numpy(gq).to(DEV), torch.from_numpy(gs).to(DEV), torch.from_numpy(cand).to(DEV), 40, return_pos=True)
    _same_lists(got, ref.top(40))
    b = _bits(got[0])
    zeros = [r for r in range(40) if r % 4]
    for row in range(6):
        assert (b[row] == 0).any() and (b[row] == -2 ** 31).any()                              # both zeros occur ...
        mid = got[1][row].cpu()[torch.isin(b[row], torch.tensor([0, -2 ** 31], dtype=torch.int32))]
        assert mid.tolist() == zeros                                                            # ... in id order, whatever their sign


# ---- expand ------------------------------------------------------------------------------------------------------------------------

def _lists(Bq, kin, lo, hi, seed):
    rng = np.random.default_rng(seed)
    return (torch.from_numpy(rng.uniform(0.1, 1.0, (Bq, kin)).astype(F)), torch.from_numpy(rng.integers(lo, hi, (Bq, kin)).astype(np.int64)))


def _dev_table(segments):
    return [tuple(t.to(DEV) for t in seg[:-1]) + (seg[-1],) for seg in segments]


@pytest.mark.parametrize("n,m", enumerate([1, 7, 8, 9, 63, 64, 65, 256]))
def test_expand_int8_bitwise_and_equal_to_the_float_kernel(gal, n, m):
    from cor_amd import ops
    C, alpha, odt = (16, 64, 256)[n % 3], (0, 3, 8)[(n + n // 3) % 3], DTYPES[(n // 2) % 3]           # every C meets two alphas
    normalize, qw, Bq, kin = n % 4 != 3, (1.0, 0.0, 0.5)[(n + n // 3) % 3], (1, 5, 130)[(n + 1) % 3], m + (n % 2) * 5
    gq, gs, Q = gal[C]
    gq, gs, Q = gq[:700], gs[:700], Q[:Bq]
    s, i = _lists(Bq, kin, -20, 720, 100 + m)                                                   # some ids of no row
    Qd = None if qw == 0.0 else Q.to(DEV)
    got = ops.expand_queries(Qd, [(gq.to(DEV), gs.to(DEV), 0)], s.to(DEV), i.to(DEV), m, alpha=alpha, query_weight=qw, normalize=normalize,
                             out_dtype=odt)
    want = ref_expand_sq(None if qw == 0.0 else Q, qw, [(gq, gs, 0)], s, i, m, alpha, normalize)
    assert _eq(got.cpu(), torch.from_numpy(want).to(odt))
    # the EXISTING kernel over the dequantised fp32 rows gives the same bits
    deq = ops.dequantize_rows_i8(gq.to(DEV), gs.to(DEV))
    flt = ops.expand_queries(Qd, [(deq, 0)], s.to(DEV), i.to(DEV), m, alpha=alpha, query_weight=qw, normalize=normalize, out_dtype=odt)
    assert _eq(got, flt)
    out = torch.empty((Bq, C), dtype=odt, device=DEV)
    assert ops.expand_queries(Qd, [(gq.to(DEV), gs.to(DEV), 0)], s.to(DEV), i.to(DEV), m, alpha=alpha, query_weight=qw, normalize=normalize,
                              out_dtype=odt, out=out) is out and _eq(out, got)


@pytest.mark.parametrize("C", [16, 64, 256])
@pytest.mark.parametrize("nseg", [0, 1, 2, 3, 5, 16])
def test_expand_segment_tables_int8_only_and_mixed(gal, nseg, C):
    """300 rows cut into nseg segments with an empty segment and a gap in the id space: int8 alone, and fp32 / bf16 / int8 / fp16 mixed.
    The int8-only table gives the bits of ONE int8 segment whose ids skip the gap the same way."""
    from cor_amd import ops
    gq, gs, Q = gal[C]
    Bq, m, kin = 9, 20, 24
    s, i = _lists(Bq, kin, -10, 330, nseg * 7 + C)
    cuts = np.linspace(0, 300, nseg + 1).astype(int) if nseg else np.zeros(1, int)
    if nseg >= 3:
        cuts[2] = cuts[1]                                                                       # segment 1 is empty
    off = lambda lo: int(lo) + (17 if lo >= 150 else 0)                                         # a gap of 17 ids at row 150
    int8, mixed = [], []
    for n in range(nseg):
        lo, hi = cuts[n], cuts[n + 1]
        if lo < 150 < hi:                                                                       # no segment spans the gap
            hi = 150
        int8.append((gq[lo:hi], gs[lo:hi], off(lo)))
        kind = n % 4
        deq = ref_dequantize(gq[lo:hi], gs[lo:hi])
        mixed.append(int8[-1] if kind == 2 else (deq.to((torch.float32, torch.bfloat16, None, torch.float16)[kind]), off(lo)))
    for table in (int8, mixed):
        for odt, alpha, qw, normalize in ((torch.float32, 3, 1.0, True), (torch.bfloat16, 0, 0.5, False)):
            got = ops.expand_queries(Q[:Bq].to(DEV), _dev_table(table), s.to(DEV), i.to(DEV), m, alpha=alpha, query_weight=qw, normalize=normalize,
                                     out_dtype=odt)
            want = ref_expand_sq(Q[:Bq], qw, table, s, i, m, alpha, normalize)
            assert _eq(got.cpu(), torch.from_numpy(want).to(odt)), f"{len(table)} segments"
    if nseg:                                                                                    # Q = None with query_weight = 0
        got = ops.expand_queries(None, _dev_table(mixed), s.to(DEV), i.to(DEV), m, query_weight=0.0)
        assert _eq(got.cpu(), torch.from_numpy(ref_expand_sq(None, 0.0, mixed, s, i, m, 3, True)))


# ---- the Python layer --------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def shards(gal):
    """One QuantizedGallery of 4097 rows at offset 1000 with labels and groups, and the same rows cut into a three-segment set of plain
    QuantizedShard segments (the set carries their list stages) given out of
    order with an empty segment (a set names its segments by offset, so the empty one has an offset of its own)."""
    from cor_amd.retrieval import GallerySet, QuantizedGallery, QuantizedShard
    gq, gs, Q = gal[256]
    n = 4097
    gq, gs = gq[:n].to(DEV), gs[:n].to(DEV)
    lab, grp = torch.arange(n, dtype=torch.int32) % 7, torch.arange(n, dtype=torch.int32) // 3
    one = QuantizedGallery(gq, gs, offset=1000, labels=lab, groups=grp)
    cut = lambda lo, hi: QuantizedShard(gq[lo:hi], gs[lo:hi], offset=1000 + lo, labels=lab[lo:hi], groups=grp[lo:hi])
    empty = QuantizedShard(gq[:0], gs[:0], offset=900, labels=lab[:0], groups=grp[:0])
    parts = GallerySet([cut(3000, n), cut(0, 1234), empty, cut(1234, 3000)])
    return one, parts, Q.to(DEV)


def test_quantized_shard_methods_against_their_compositions(shards, gal):
    from cor_amd import ops
    from cor_amd.retrieval import GalleryShard, QuantizedGallery, QuantizedShard
    one, _, q = shards
    gq, gs, Q = gal[256]
    plain = QuantizedShard(one.rows, one.scales, offset=1000, labels=one.labels, groups=one.groups)
    assert not hasattr(plain, "rescore") and not hasattr(plain, "expand") and not hasattr(plain, "rerank")   # the coarse copy only searches
    same = plain.gallery()
    assert type(same) is QuantizedGallery and same.rows is plain.rows and same.scales is plain.scales and same.labels is plain.labels
    assert same.offset == 1000 and QuantizedGallery.of(one) is one and type(QuantizedGallery.from_rows(gq[:16].float().to(DEV))) is QuantizedGallery
    for dt in DTYPES:
        d = one.dequantized(dt)
        assert isinstance(d, GalleryShard) and d.offset == 1000 and d.labels is one.labels and d.groups is one.groups
        assert _eq(d.rows.cpu(), ref_dequantize(gq[:4097], gs[:4097], dt))
    deq = one.dequantized()
    s, i = one.search(q, 20)
    # rescore and expand are the ops over the shard's tensors; expand equals the float shard's expand
    _same_lists(one.rescore(q, i, 10, return_pos=True), ops.rescore_topk_i8(q, one.rows, one.scales, i, 10, g_offset=1000, return_pos=True))
    e = one.expand(q, s, i, 20)
    assert _eq(e, deq.expand(q, s, i, 20)) and _eq(e.cpu(), torch.from_numpy(ref_expand_sq(Q, 1.0, [(gq[:4097], gs[:4097], 1000)], s.cpu(), i.cpu(), 20, 3, True)))
    # neighbour_graph: the dequantised rows as queries, in batches
    g8 = one.neighbour_graph(8, batch=1500)
    ks, ki = one.search(deq.rows, 8)
    assert g8.width == 8 and g8.offsets == (1000,) and g8.lengths == (4097,)
    assert _eq(g8.kth[0], ks[:, 7].contiguous()) and _eq(g8.rnbr[0], ops.knn_reciprocal([(ki, 1000)], 0))
    assert (g8.rnbr[0][:, 0].cpu() == torch.arange(1000, 5097)).all()                            # a row finds itself first
    # rerank: the lists and the graph are all it reads
    rs, ri = one.rerank(s, i, g8, lam=0.3, k=10)
    _same_lists((rs, ri), ops.rerank_reciprocal(s, i, g8.segments, 8, 0.3, 10))
    with pytest.raises(ValueError, match="build a new graph"):
        QuantizedGallery(one.rows[:100], one.scales[:100], offset=1000).rerank(s, i, g8)        # a stale graph
    # augmented: search the dequantised rows, expand with weight 0, quantise; batches do not matter
    aug = one.augmented(3, batch=2000)
    assert type(aug) is QuantizedGallery and aug.offset == 1000 and aug.labels is one.labels and aug.groups is one.groups
    s3, i3 = one.search(deq.rows, 3)
    wq, wsc = ops.quantize_rows_i8(one.expand(None, s3, i3, 3, query_weight=0.0))
    assert _eq(aug.rows, wq) and _eq(aug.scales, wsc)
    x = ref_expand_sq(None, 0.0, [(gq[:4097], gs[:4097], 1000)], s3[:50].cpu(), i3[:50].cpu(), 3, 3, True)
    rq, rsc = ref_quantize(x)
    assert _eq(aug.rows[:50].cpu(), torch.from_numpy(rq)) and _eq(aug.scales[:50].cpu(), torch.from_numpy(rsc))
    # a float shard with a search-only int8 neighbour still expands over its OWN rows; with an int8 gallery, over the gallery's
    fine = GalleryShard(_unit(4097, 256, 77).to(DEV), offset=1000)
    fa = fine.augmented(3, batch=2000, neighbours=plain)
    f3 = one.search(fine.rows[:2000], 3)
    assert _eq(fa.rows[:2000], fine.expand(None, f3[0], f3[1], 3, query_weight=0.0))
    fg = fine.augmented(3, batch=2000, neighbours=one)
    assert _eq(fg.rows[:2000], one.expand(None, f3[0], f3[1], 3, query_weight=0.0))


def test_gallery_set_of_int8_segments_equals_one_shard(shards):
    one, parts, q = shards
    assert [len(sh) for sh in parts.segments] == [0, 1234, 1766, 1097]
    s, i = one.search(q, 50)
    _same_lists(parts.search(q, 50), (s, i))
    _same_lists(parts.rescore(q, i, 10), one.rescore(q, i, 10))
    for kw in (dict(), dict(alpha=0, query_weight=0.5, normalize=False, out_dtype=torch.float16)):
        assert _eq(parts.expand(q, s, i, 50, **kw), one.expand(q, s, i, 50, **kw))
    g1, gp = one.neighbour_graph(6, batch=3000), parts.neighbour_graph(6, batch=700)
    assert gp.offsets == (1000, 2234, 4000) and gp.lengths == (1234, 1766, 1097)
    assert _eq(torch.cat(gp.rnbr), g1.rnbr[0]) and _eq(torch.cat(gp.kth), g1.kth[0])
    _same_lists(parts.rerank(s, i, gp, lam=0.4, k=20), one.rerank(s, i, g1, lam=0.4, k=20))
    with pytest.raises(ValueError, match="build a new graph"):
        parts.rerank(s, i, g1)
    a1, ap = one.augmented(4, batch=4097), parts.augmented(4, batch=500)
    live = [sh for sh in ap.segments if len(sh)]
    assert [type(sh).__name__ for sh in ap.segments] == ["QuantizedGallery"] * 4 and [sh.offset for sh in ap.segments] == [900, 1000, 2234, 4000]
    assert _eq(torch.cat([sh.rows for sh in live]), a1.rows) and _eq(torch.cat([sh.scales for sh in live]), a1.scales)


def test_mixed_gallery_set_and_the_search_compositions(shards, gal):
    from cor_amd import retrieval
    from cor_amd.retrieval import GallerySet, GalleryShard, QuantizedShard
    one, _, q = shards
    gq, gs, Q = gal[256]
    deq = one.dequantized()
    # mixed: int8 | (empty int8) | fp32 of the dequantised rows | bf16 copy of them, given out of order
    cutq = lambda lo, hi: QuantizedShard(one.rows[lo:hi], one.scales[lo:hi], offset=1000 + lo)
    f32 = GalleryShard(deq.rows[1500:3000], offset=2500)
    b16 = GalleryShard(deq.rows[3000:], offset=4000, dtype=torch.bfloat16)
    mixed = GallerySet([b16, cutq(0, 1500), f32, QuantizedShard(one.rows[:0], one.scales[:0], offset=500)])
    s, i = mixed.search(q, 30)
    table = [(gq[:1500], gs[:1500], 1000), (f32.rows.cpu(), 2500), (b16.rows.cpu(), 4000)]
    assert _eq(mixed.expand(q, s, i, 30).cpu(), torch.from_numpy(ref_expand_sq(Q, 1.0, table, s.cpu(), i.cpu(), 30, 3, True)))
    rs, ri = mixed.rescore(q, i, 10)
    parts = [sh.rescore(q, i, 10) for sh in (cutq(0, 1500).gallery(), f32, b16)]
    _same_lists((rs, ri), retrieval.merge_topk_device([p[0] for p in parts], [p[1] for p in parts], 10))
    g = mixed.neighbour_graph(5, batch=1000)
    assert g.offsets == (1000, 2500, 4000) and g.lengths == (1500, 1500, 1097)
    assert mixed.rerank(s, i, g, k=10)[1].shape == (130, 10)
    am = mixed.augmented(3, batch=1000)
    assert [type(sh).__name__ for sh in am.segments] == ["QuantizedGallery", "QuantizedGallery", "GalleryShard", "GalleryShard"]
    s3, i3 = mixed.search(deq.rows[:200], 3)
    wq, wsc = retrieval.ops.quantize_rows_i8(mixed.expand(None, s3, i3, 3, query_weight=0.0))
    assert am.segments[1].offset == 1000 and _eq(am.segments[1].rows[:200], wq) and _eq(am.segments[1].scales[:200], wsc)
    # two_stage_search(coarse = bf16 shard, fine = int8 gallery); expanded_search and reranked_search on the int8-only gallery
    coarse = GalleryShard(deq.rows, offset=1000, dtype=torch.bfloat16)
    _same_lists(retrieval.two_stage_search(q, coarse, one, 10, 50), one.rescore(q, coarse.search(q, 50)[1], 10))
    _same_lists(retrieval.two_stage_search(q, one, one, 10, 50), one.search(q, 10))
    es, ei, eq = retrieval.expanded_search(q, one, 10, 5, alpha=2, query_weight=0.5)
    s5, i5 = one.search(q, 5)
    want_q = one.expand(q, s5, i5, 5, alpha=2, query_weight=0.5)
    assert _eq(eq, want_q)
    _same_lists((es, ei), one.search(want_q, 10))
    g7 = one.neighbour_graph(7)
    s50, i50 = one.search(q, 50)
    _same_lists(retrieval.reranked_search(q, one, g7, 10, 50), one.rerank(s50, i50, g7, k=10))


def test_side_stream_and_captured_graph(shards):
    """Re-scoring and then expanding on a side stream, and the two captured in ONE single-stream graph that is replayed with new queries."""
    from cor_amd import ops
    one, _, q = shards
    Bq, kin, k = 64, 100, 20
    qa, qb = q[:Bq].contiguous(), q[Bq:2 * Bq].contiguous()
    ca, cb = one.search(qa, kin)[1], one.search(qb, kin)[1]

    def both(qq, cc):
        s, i = ops.rescore_topk_i8(qq, one.rows, one.scales, cc, k, g_offset=1000)
        return s, i, ops.expand_queries(qq, [(one.rows, one.scales, 1000)], s, i, k)

    want_a, want_b = both(qa, ca), both(qb, cb)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = both(qa, ca)
    side.synchronize()
    assert all(_eq(g, w) for g, w in zip(got, want_a))
    qin, cin = qa.clone(), ca.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                                               # one capture stream
        out = both(qin, cin)
    graph.replay()
    torch.cuda.synchronize()
    assert all(_eq(g, w) for g, w in zip(out, want_a))
    qin.copy_(qb)
    cin.copy_(cb)
    graph.replay()
    torch.cuda.synchronize()
    assert all(_eq(g, w) for g, w in zip(out, want_b))

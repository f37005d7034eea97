"""GPU tests of the filtered int8 gallery search (cor_similarity_topk_i8_filtered, ops.similarity_topk_i8_filtered, QuantizedShard with
labels, GalleryShard.quantized, load_gallery_shard). Every comparison is bitwise, on score bits (.view(int32)) and indices, against
tests/i8_filtered_refs.py, the CPU restatement of the definition in include/cor_amd.h, with no excused position."""
import numpy as np
import pytest
import torch

from tests import i8_filtered_refs as FR
from tests import i8_refs as R
from tests.test_gpu_topk_i8 import _gallery, _np, _same            # the seeded galleries are computed once for both files

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F = np.float32
BIG = 2 ** 33 + 5


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _search(Q, gq, gs, k, rl, ql, mode, offset=0, flags=0):
    from cor_amd import ops
    return ops.similarity_topk_i8_filtered(_dev(Q), _dev(gq), _dev(gs), k, _dev(rl), _dev(ql), mode=mode, g_offset=offset, flags=flags)


# ------------------------------------------------------------------------------------------------------------------ label layouts

def _row_labels(layout, Ng, seed):
    rng = np.random.default_rng(seed)
    if layout == "uniform4":
        rl = rng.integers(0, 4, Ng)
    elif layout == "uniform64":
        rl = rng.integers(0, 64, Ng)
    elif layout == "blocks16":                                                     # class-sorted: one label's rows in one block
        rl = (np.arange(Ng) * 16) // Ng
    elif layout == "skew":                                                         # one class holds 90 %
        rl = np.where(rng.random(Ng) < 0.9, 0, rng.integers(1, 4, Ng))
    elif layout == "runs":                                                         # image ids in runs of 1-8 rows
        rl = np.repeat(np.arange(Ng), rng.integers(1, 9, Ng))[:Ng]
    else:
        raise KeyError(layout)
    return rl.astype(np.int32)


def _queries(G, rl, Bq, seed):
    """Bq noisy copies of gallery rows; each query carries its source row's label (mode "ne": its own image is excluded, "eq": its
    class), every 7th is unrestricted"""
    rng = np.random.default_rng(seed)
    src = rng.integers(0, G.shape[0], Bq)
    Q = G[src] + F(0.3) * rng.standard_normal((Bq, G.shape[1])).astype(F)
    ql = rl[src].copy()
    ql[3::7] = -1
    return Q, ql.astype(np.int32)


# ------------------------------------------------------------------------------------------------------------------ shapes

BQS, NGS, CS, KS = (1, 7, 65, 257, 513), (15, 200, 4096, 4097, 40000, 70001), (16, 48, 64, 128, 256), (1, 10, 33, 100, 256)
LAYOUTS = (("eq", "uniform4"), ("eq", "uniform64"), ("eq", "blocks16"), ("eq", "skew"), ("ne", "runs"), ("ne", "uniform4"))
# 42 of the 4500 combinations: round a = 0 .. 6 pairs row count b with layout (a + b) % 6, C (b + 3 a) % 5, k (b + 2 a) % 5 and Bq (4 a + b) % 5:
# seven rounds reach every residue, so every (Ng, layout), (Ng, C), (Ng, k) and (Ng, Bq) pair occurs
SHAPES = [(BQS[(4 * a + b) % 5], NGS[b], CS[(b + 3 * a) % 5], KS[(b + 2 * a) % 5]) + LAYOUTS[(a + b) % 6] + (a,)
          for a in range(7) for b in range(6)]


def _offset(n):
    return BIG if n == 5 else (1000 if n % 2 else 0)


def test_shape_cases_cover_every_axis_value():
    assert len(SHAPES) == 42 and len(set(s[:6] for s in SHAPES)) == 42
    assert {(s[1], s[4], s[5]) for s in SHAPES} == {(Ng,) + m for Ng in NGS for m in LAYOUTS}
    assert {(s[1], s[2]) for s in SHAPES} == {(Ng, C) for Ng in NGS for C in CS}
    assert {(s[1], s[3]) for s in SHAPES} == {(Ng, k) for Ng in NGS for k in KS}
    assert {(s[1], s[0]) for s in SHAPES} == {(Ng, Bq) for Ng in NGS for Bq in BQS}
    offs = [_offset(n) for n in range(len(SHAPES))]
    assert offs.count(1000) == 20 and offs.count(BIG) == 1


@pytest.mark.parametrize("n", range(len(SHAPES)))
def test_search_is_bitwise_on_labelled_galleries(n):
    from cor_amd import _native
    Bq, Ng, C, k, mode, layout, a = SHAPES[n]
    G, gq, gs = _gallery(Ng, C)
    rl = _row_labels(layout, Ng, Ng + a)
    Q, ql = _queries(G, rl, Bq, Bq + k + a)
    off = _offset(n)
    want = FR.ref_search_filtered(Q, gq, gs, k, rl, ql, mode, off)
    _same(_search(Q, gq, gs, k, rl, ql, mode, off), want, "default")
    if Ng >= 40000:                                                                # these layouts stay off the brute force
        got = _search(Q, gq, gs, k, rl, ql, mode, off, flags=_native.TOPK_NO_FALLBACK)
        assert (_np(got[1]) != -2).all(), f"{int((_np(got[1])[:, 0] == -2).sum())} of {Bq} queries overflowed"
        _same(got, want, "no fallback")


@pytest.mark.parametrize("Bq,Ng,C,k", [(65, 40000, 256, 10), (7, 4097, 48, 100)])
def test_all_unrestricted_equals_the_unfiltered_search(Bq, Ng, C, k):
    from cor_amd import ops
    G, gq, gs = _gallery(Ng, C)
    rl = _row_labels("uniform4", Ng, 1)
    Q, _ = _queries(G, rl, Bq, 2)
    ql = np.full(Bq, -1, np.int32)
    for mode in ("eq", "ne"):
        got = _search(Q, gq, gs, k, rl, ql, mode, 1000)
        plain = ops.similarity_topk_i8(_dev(Q), _dev(gq), _dev(gs), k, g_offset=1000)
        assert torch.equal(got[1], plain[1]) and torch.equal(got[0].view(torch.int32), plain[0].view(torch.int32)), mode
    _same(got, R.ref_search(Q, gq, gs, k, 1000))


# ------------------------------------------------------------------------------------------------------------------ tails

def test_tails():
    Ng, C, k = 4097, 64, 50
    G, gq, gs = _gallery(Ng, C)
    rng = np.random.default_rng(11)
    rl = rng.integers(0, 5, Ng).astype(np.int32)
    rl[[100, 2047, 4096]] = 77                                                     # exactly three rows, one of them the last
    Q = G[rng.integers(0, Ng, 9)] * F(1.5)
    ql = np.array([0, 99, 77, 1, -1, 2, 99, 3, 77], np.int32)                      # 99: no row carries it
    counts = [int(FR.allowed_rows(rl, int(q), "eq").sum()) for q in ql]
    assert counts[1] == 0 and counts[6] == 0 and counts[2] == 3 and counts[8] == 3 and counts[4] == Ng and min(counts[0], counts[3]) > k
    want = FR.ref_search_filtered(Q, gq, gs, k, rl, ql, "eq", 1000)
    assert (want[1][1] == -1).all() and (want[1][2, :3] >= 1000).all() and (want[1][2, 3:] == -1).all()
    assert sorted(want[1][2, :3].tolist()) == [1100, 3047, 5096]
    got = _search(Q, gq, gs, k, rl, ql, "eq", 1000)
    _same(got, want, "eq")
    assert np.isneginf(_np(got[0])[1]).all() and np.isneginf(_np(got[0])[2, 3:]).all()
    # ne on a single-label gallery: a query with that label has no allowed row
    one = np.full(Ng, 6, np.int32)
    ql2 = np.array([6, 5, 6, -1, 6, 6, 0, 6, 6], np.int32)
    assert [int(FR.allowed_rows(one, int(q), "ne").sum()) for q in ql2] == [0, Ng, 0, Ng, 0, 0, Ng, 0, 0]
    want = FR.ref_search_filtered(Q, gq, gs, k, one, ql2, "ne")
    assert (want[1][0] == -1).all() and (want[1][1] >= 0).all()
    _same(_search(Q, gq, gs, k, one, ql2, "ne"), want, "ne, one label")
    # a shard smaller than k
    G2, gq2, gs2 = _gallery(15, 64)
    rl3 = np.array([1, 1, 2, 1, 2, 2, 1, 1, 1, 2, 1, 1, 2, 1, 1], np.int32)
    for mode in ("eq", "ne"):
        want = FR.ref_search_filtered(Q[:, :64], gq2, gs2, k, rl3, np.array([1, 2, -1, 3, 1, 2, 2, 1, -1], np.int32), mode, 7)
        assert (want[1][:, 15:] == -1).all()
        _same(_search(Q[:, :64], gq2, gs2, k, rl3, np.array([1, 2, -1, 3, 1, 2, 2, 1, -1], np.int32), mode, 7), want, f"Ng < k, {mode}")


# ------------------------------------------------------------------------------------------------------------------ ties across the filter

@pytest.mark.parametrize("mode", ["ne", "eq"])
def test_ties_across_the_filter(mode):
    """The duplicated rows, zero scales and zero query of test_gpu_topk_i8.test_ties_zero_scales_and_a_zero_query; one copy of every
    duplicate pair is disallowed, and so are rows Ng - 1 and Ng - 3 of the ragged last tile."""
    Ng, C = 70001, 64
    G, gq, gs = _gallery(Ng, C)
    gq, gs = gq.copy(), gs.copy()
    Q = G[[5, 20000, Ng - 3, 11]] * F(2.0)
    for a, b in ((5, 9), (5, 14), (5, 66), (20000, 45000), (20000, 69999), (Ng - 3, Ng - 1), (Ng - 3, 4)):
        gq[b], gs[b] = gq[a], gs[a]
    gs[[11, 12, 30000]] = 0.0
    gq[12] = -gq[11]
    Q = np.concatenate([Q, np.zeros((1, C), F)])
    off_rows = [9, 66, 20000, 69999, Ng - 1, Ng - 3, 2, 30000]                     # 5 / 14, 45000 and 4 stay allowed
    rl = np.full(Ng, 1, np.int32)
    rl[off_rows] = 7
    ql = np.full(5, 7 if mode == "ne" else 1, np.int32)                            # the same allowed set in either mode
    S = R.ref_scores(Q, gq, gs)[0]
    assert np.signbit(S[3, 11]) != np.signbit(S[3, 12]) and (S[4] == 0).all()
    for k in (10, 100):
        want = FR.ref_topk_filtered(S, k, rl, ql, mode, 1000)
        assert want[1][0, :2].tolist() == [1005, 1014] and want[1][1, 0] == 46000 and want[1][2, 0] == 1004
        assert not np.isin(want[1], np.array(off_rows) + 1000).any()
        assert want[1][4].tolist() == [1000 + g for g in range(k + 4) if g not in (2, 9, 66)][:k]
        plain = R.ref_topk(S, k, 1000)
        assert plain[1][0, :4].tolist() == [1005, 1009, 1014, 1066]                # what the filter removed
        _same(_search(Q, gq, gs, k, rl, ql, mode, 1000), want, f"k={k}")


# ------------------------------------------------------------------------------------------------------------------ overflow

def test_overflow_ranks_only_allowed_rows():
    from cor_amd import _native
    Ng, C, k = 20000, 256, 100
    G, gq0, gs0 = _gallery(70001, C)
    gq, gs = np.repeat(gq0[:1], Ng, axis=0), np.repeat(gs0[:1], Ng)                # 20000 identical rows
    rl = np.where(np.arange(Ng) % 3 == 0, 1, 0).astype(np.int32)                   # every third row is allowed for query 0
    five = [17, 4000, 5000, 6000, 19999]
    rl[five] = 9                                                                   # and five rows for query 1
    Q = np.stack([G[0], G[1], G[0]])
    ql = np.array([1, 9, -1], np.int32)
    want = FR.ref_search_filtered(Q, gq, gs, k, rl, ql, "eq")
    allowed0 = [g for g in range(400) if g % 3 == 0 and g not in five]
    assert want[1][0].tolist() == allowed0[:k] and want[1][1, :5].tolist() == five and (want[1][1, 5:] == -1).all()
    assert want[1][2].tolist() == list(range(k))
    _same(_search(Q, gq, gs, k, rl, ql, "eq"), want, "fallback")
    marked = _search(Q, gq, gs, k, rl, ql, "eq", flags=_native.TOPK_NO_FALLBACK)
    mi, ms = _np(marked[1]), _np(marked[0])
    assert (mi[[0, 2]] == -2).all() and np.isneginf(ms[[0, 2]]).all()
    assert np.array_equal(mi[1], want[1][1]) and np.array_equal(ms[1].view(np.int32), want[0][1].view(np.int32))


# ------------------------------------------------------------------------------------------------------------------ labels as the caller has them

def test_labels_through_a_view_and_as_int64():
    from cor_amd import ops
    Ng, C, k = 4097, 128, 33
    G, gq, gs = _gallery(Ng, C)
    rl = _row_labels("uniform4", Ng, 5)
    Q, ql = _queries(G, rl, 7, 6)
    want = FR.ref_search_filtered(Q, gq, gs, k, rl, ql, "ne")
    dq, dg, ds = _dev(Q), _dev(gq), _dev(gs)
    big = _dev(np.concatenate([np.array([123], np.int32), rl]))
    view = big[1:]                                                                 # 4 bytes into its buffer
    assert view.data_ptr() % 16 == 4
    _same(ops.similarity_topk_i8_filtered(dq, dg, ds, k, view, _dev(ql), mode="ne"), want, "view")
    _same(ops.similarity_topk_i8_filtered(dq, dg, ds, k, _dev(rl.astype(np.int64)), _dev(ql.astype(np.int64)), mode="ne"), want, "int64")
    _same(ops.similarity_topk_i8_filtered(dq, dg, ds, k, torch.from_numpy(rl), ql.tolist(), mode="ne"), want, "host labels")
    assert big[0].item() == 123 and torch.equal(view.cpu(), torch.from_numpy(rl))


# ------------------------------------------------------------------------------------------------------------------ the Python layers

def _eq(a, b):
    return torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))


def test_python_layers(tmp_path):
    from cor_amd import ops, retrieval
    Ng, C = 4097, 64
    G = torch.from_numpy(_gallery(Ng, C)[0])
    rl = _row_labels("runs", Ng, 9)
    src = [3, 900, 4096, 2000, 1999]
    Q = (G[src] + 0.01).to(DEV)
    ql = torch.from_numpy(rl[src].copy())
    ql[3] = -1
    shard = retrieval.GalleryShard(G.to(DEV), offset=1000, labels=rl)
    qs = shard.quantized()
    assert isinstance(qs, retrieval.QuantizedShard) and qs.labels is shard.labels and qs.groups is None and qs.offset == 1000
    wq, ws = R.ref_quantize(G)
    for m in ("eq", "ne"):
        got = qs.search(Q, 20, query_labels=ql, mode=m)
        assert _eq(got, ops.similarity_topk_i8_filtered(Q, qs.rows, qs.scales, 20, qs.labels, ql.to(DEV), mode=m, g_offset=1000))
        _same(got, FR.ref_search_filtered(_np(Q), wq, ws, 20, rl, ql.numpy(), m, 1000), m)
    assert _eq(qs.search(Q, 20), ops.similarity_topk_i8(Q, qs.rows, qs.scales, 20, g_offset=1000))       # unfiltered as before
    with pytest.raises(ValueError):
        qs.search(Q, 5, query_labels=ql, distinct=True)
    with pytest.raises(ValueError):
        retrieval.QuantizedShard.from_rows(G.to(DEV)).search(Q, 5, query_labels=ql)
    with pytest.raises(ValueError):
        retrieval.QuantizedShard(qs.rows, qs.scales, labels=rl[:-1])
    # coarse stage of a filtered two-stage search = the composition of the two calls, and the query's own image is gone
    fine = retrieval.GalleryShard(G.to(DEV), offset=1000)
    ts, ti = retrieval.two_stage_search(Q, qs, fine, 10, 50, query_labels=ql, mode="ne")
    assert _eq((ts, ti), fine.rescore(Q, qs.search(Q, 50, query_labels=ql, mode="ne")[1], 10))
    lab = torch.from_numpy(rl)[(ti.cpu() - 1000).clamp(min=0)]
    assert (ti >= 1000).all() and not ((lab == ql[:, None]) & (ql[:, None] >= 0)).any() and ti[3, 0].item() == 3000
    # two labelled int8 segments = the single shard
    a = retrieval.QuantizedShard(qs.rows[:2000], qs.scales[:2000], offset=1000, labels=rl[:2000])
    b = retrieval.QuantizedShard(qs.rows[2000:], qs.scales[2000:], offset=3000, labels=rl[2000:])
    gset = retrieval.GallerySet([a, b])
    for m in ("eq", "ne"):
        assert _eq(gset.search(Q, 30, query_labels=ql, mode=m), qs.search(Q, 30, query_labels=ql, mode=m)), m
    # disk round trip
    path = str(tmp_path / "gal")
    retrieval.save_gallery(path, qs.rows, world=2, scales=qs.scales, labels=rl)
    lo, hi = retrieval.shard_bounds(Ng, 2, 1)
    back = retrieval.load_gallery_shard(path, 1, DEV)
    assert isinstance(back, retrieval.QuantizedShard) and back.offset == lo and len(back) == hi - lo and back.groups is None
    assert back.labels.dtype == torch.int32 and back.labels.device == back.rows.device and torch.equal(back.labels.cpu(), torch.from_numpy(rl[lo:hi]))
    _same(back.search(Q, 5, query_labels=ql, mode="ne"), FR.ref_search_filtered(_np(Q), wq[lo:hi], ws[lo:hi], 5, rl[lo:hi], ql.numpy(), "ne", lo))
    # an empty labelled shard
    empty = retrieval.QuantizedShard.from_rows(shard.rows[:0], offset=7, labels=rl[:0])
    es, ei = empty.search(Q, 4, query_labels=ql, mode="ne")
    assert len(empty) == 0 and (ei == -1).all() and torch.isneginf(es).all() and tuple(ei.shape) == (5, 4)


# ------------------------------------------------------------------------------------------------------------------ streams

def test_side_stream_and_graph_replay():
    from cor_amd import ops
    G, gq, gs = _gallery(40000, 256)
    rl = _row_labels("runs", 40000, 4)
    (Qa, qla), (Qb, qlb) = _queries(G, rl, 33, 3), _queries(G, rl, 33, 8)
    q, sc, drl = _dev(gq), _dev(gs), _dev(rl)
    Q, dql = _dev(Qa), _dev(qla)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = ops.similarity_topk_i8_filtered(Q, q, sc, 100, drl, dql, mode="ne")   # (also sets the kernels' one-time attributes before the capture)
    side.synchronize()
    _same(got, FR.ref_search_filtered(Qa, gq, gs, 100, rl, qla, "ne"), "side stream")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cs, ci = ops.similarity_topk_i8_filtered(Q, q, sc, 100, drl, dql, mode="ne")
    Q.copy_(_dev(Qb))
    dql.copy_(_dev(qlb))
    graph.replay()
    torch.cuda.synchronize()
    assert not np.array_equal(qla, qlb)
    _same((cs, ci), FR.ref_search_filtered(Qb, gq, gs, 100, rl, qlb, "ne"), "graph replay")


def test_labelled_quantized_shard_in_a_one_rank_distributed_search():
    """distributed_search takes a labelled QuantizedShard and a filter unchanged (one-rank nccl group, gather and deferred forms)."""
    import socket
    import torch.distributed as dist
    from cor_amd import retrieval
    if dist.is_initialized():
        pytest.skip("a process group already exists in this process")
    G = torch.from_numpy(_gallery(4097, 128)[0])
    rl = _row_labels("runs", 4097, 2)
    src = [7, 4000, 12]
    Q = (G[src] * 0.9).to(DEV)
    ql = torch.from_numpy(rl[src].copy())
    shard = retrieval.QuantizedShard.from_rows(G.to(DEV), offset=100, labels=rl)
    s0, i0 = shard.search(Q, 50, query_labels=ql, mode="ne")
    assert not torch.isin(i0.cpu(), torch.tensor(src) + 100).any()
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=torch.device(DEV))
    try:
        s1, i1 = retrieval.distributed_search(Q, shard, 50, max_local=8, always_collective=True, query_labels=ql, filter_mode="ne")
        s2, i2 = retrieval.distributed_search(Q, shard, 50, max_local=8, always_collective=True, defer=True, query_labels=ql,
                                              filter_mode="ne").result()
        torch.cuda.synchronize()
        for s_, i_ in ((s1, i1), (s2, i2)):
            assert torch.equal(i_, i0.cpu()) and torch.equal(s_.view(torch.int32), s0.cpu().view(torch.int32))
    finally:
        dist.destroy_process_group()

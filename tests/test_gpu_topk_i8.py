"""GPU tests of the int8 gallery search (cor_quantize_rows_i8, cor_similarity_topk_i8, ops.quantize_rows_i8 / similarity_topk_i8,
retrieval.QuantizedShard, GalleryShard.quantized, save_gallery(scales=)). Every comparison is bitwise, on score bits (.view(int32)) and
indices, against tests/i8_refs.py, the CPU restatement of the definition in include/cor_amd.h, with no excused position."""
import numpy as np
import pytest
import torch

from tests import i8_refs as R
from tests.test_cpu_topk_i8 import edge_rows

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F = np.float32
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
BIG = 2 ** 33 + 5


def _np(t):
    return t.detach().cpu().numpy()


def _same(got, want, what=""):
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.int64 and tuple(got[0].shape) == want[0].shape, what
    gi, gs = _np(got[1]), _np(got[0]).view(np.int32)
    bad = np.flatnonzero((gi != want[1]).any(axis=1) | (gs != want[0].view(np.int32)).any(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} queries differ, first {bad[0]}: got {gi[bad[0]][:8]} {_np(got[0])[bad[0]][:8]} want {want[1][bad[0]][:8]} {want[0][bad[0]][:8]}"


def _search(Q, gq, gs, k, offset=0, flags=0):
    from cor_amd import ops
    return ops.similarity_topk_i8(torch.from_numpy(Q).to(DEV), torch.from_numpy(gq).to(DEV), torch.from_numpy(gs).to(DEV), k, g_offset=offset,
                                  flags=flags)


# ------------------------------------------------------------------------------------------------------------------ the quantiser

@pytest.mark.parametrize("n", [1, 63, 257])
@pytest.mark.parametrize("C", [16, 48, 64, 128, 256])
def test_quantiser_is_bitwise_for_every_source_dtype(n, C):
    from cor_amd import ops
    X = torch.randn((n, C), generator=torch.Generator().manual_seed(n * 1000 + C)) * 3.0
    X[n // 2] = 0.0                                                                # a zero row
    for dt in DTYPES:
        src = X.to(dt)
        dev = src.to(DEV)
        q, sc = ops.quantize_rows_i8(dev)
        assert torch.equal(dev.cpu(), src)                                         # the source is untouched
        wq, ws = R.ref_quantize(src)
        assert q.dtype == torch.int8 and sc.dtype == torch.float32 and tuple(q.shape) == (n, C) and tuple(sc.shape) == (n,)
        assert np.array_equal(_np(q), wq), f"{dt}: q differs"
        assert np.array_equal(_np(sc).view(np.int32), ws.view(np.int32)), f"{dt}: scale bits differ"
        assert (_np(q)[n // 2] == 0).all() and _np(sc)[n // 2] == 0


@pytest.mark.parametrize("C", [16, 64, 256])
def test_quantiser_edge_rows(C):
    from cor_amd import ops
    X, why = edge_rows(C)
    q, sc = ops.quantize_rows_i8(torch.from_numpy(X).to(DEV))
    wq, ws = R.ref_quantize(X)
    for g in range(X.shape[0]):
        assert np.array_equal(_np(q)[g], wq[g]) and _np(sc)[g].view(np.int32) == ws[g].view(np.int32), why[g]
    view = torch.from_numpy(np.concatenate([np.ones((1, C), F), X])).to(DEV)[1:]   # rows that start 4 C bytes into their buffer
    q2, sc2 = ops.quantize_rows_i8(view)
    assert torch.equal(q2, q) and torch.equal(sc2, sc)


# ------------------------------------------------------------------------------------------------------------------ layout

def _pattern_rows(n, C, step, shift):
    """int8 rows with entries in {-127, 0, 127}: row g is +127 at (g * step + shift) % C and -127 at its right neighbour"""
    X = np.zeros((n, C), np.int8)
    g = np.arange(n)
    X[g, (g * step + shift) % C] = 127
    X[g, (g * step + shift + 1) % C] = -127
    return X


@pytest.mark.parametrize("C", [16, 48, 64, 128, 256])
def test_layout_on_exact_integer_patterns(C):
    """Gallery row g is non-zero at positions g mod C and its neighbour, the queries carry another asymmetric pattern (steps 3 and 1): a
    swapped row / column write, a wrong K chunk or a dropped K tail changes the integer scores. Scales are 1 (amax = 127)."""
    Ng, Bq = 4 * C + 37, 70
    gq = _pattern_rows(Ng, C, 1, 0)
    Q = _pattern_rows(Bq, C, 3, 2).astype(F)
    Q[np.arange(Bq), (np.arange(Bq) * 3 + 7) % C] += 64.0                          # a third entry: the three weights differ
    gs = np.ones(Ng, F)
    S, qq, qs = R.ref_scores(Q, gq, gs)
    assert len(np.unique(R.int_dots(qq, gq))) >= 5
    for k in (1, 10, 100):
        _same(_search(Q, gq, gs, k), R.ref_topk(S, k), f"C={C} k={k}")


def test_largest_dot_product():
    gq = np.full((300, 256), 127, np.int8)
    gq[::3] = -127
    Q = np.full((5, 256), -2.0, F)
    Q[1] = 2.0
    gs = np.full(300, F(1.0) / F(127.0), F)
    S = R.ref_scores(Q, gq, gs)[0]
    assert np.abs(R.int_dots(R.ref_quantize(Q)[0], gq)).max() == 127 * 127 * 256
    _same(_search(Q, gq, gs, 40), R.ref_topk(S, 40), "largest |d|")


# ------------------------------------------------------------------------------------------------------------------ shapes

BQS, NGS, CS, KS = (1, 7, 65, 257), (1, 15, 17, 200, 4097, 40000, 70001), (16, 48, 64, 128, 256), (1, 10, 32, 33, 100, 256)
# 42 of the 840 combinations: round a = 0 .. 5 pairs row count b with k (a + b) % 6, C (b + 2 a) % 5 and Bq (3 a + b) % 4: every (Ng, k) pair,
# every (Ng, C) pair and every (Ng, Bq) pair occurs
SHAPES = [(BQS[(3 * a + b) % 4], NGS[b], CS[(b + 2 * a) % 5], KS[(a + b) % 6]) for a in range(6) for b in range(7)]


def test_shape_cases_cover_every_axis_value():
    assert len(SHAPES) == 42 and len(set(SHAPES)) == 42
    assert {(s[1], s[3]) for s in SHAPES} == {(Ng, k) for Ng in NGS for k in KS}        # k > Ng and both sample-stride sizes at every k
    assert {(s[1], s[2]) for s in SHAPES} == {(Ng, C) for Ng in NGS for C in CS}
    assert {(s[1], s[0]) for s in SHAPES} == {(Ng, Bq) for Ng in NGS for Bq in BQS}


_GALLERIES = {}


def _gallery(Ng, C):
    """(rows f32, q int8, scale f32) of a seeded unit-norm gallery; computed once per (Ng, C), never modified"""
    if (Ng, C) not in _GALLERIES:
        rng = np.random.default_rng(Ng * 7 + C)
        G = rng.standard_normal((Ng, C)).astype(F)
        G /= np.linalg.norm(G, axis=1, keepdims=True).astype(F)
        _GALLERIES[(Ng, C)] = (G,) + R.ref_quantize(G)
    return _GALLERIES[(Ng, C)]


@pytest.mark.parametrize("Bq,Ng,C,k", SHAPES)
def test_search_is_bitwise_on_random_galleries(Bq, Ng, C, k):
    from cor_amd import _native
    G, gq, gs = _gallery(Ng, C)
    rng = np.random.default_rng(Bq + k)
    Q = G[rng.integers(0, Ng, Bq)] + F(0.3) * rng.standard_normal((Bq, C)).astype(F)
    want = R.ref_search(Q, gq, gs, k)
    _same(_search(Q, gq, gs, k), want, "default")
    got = _search(Q, gq, gs, k, flags=_native.TOPK_NO_FALLBACK)                    # random data never overflows
    assert (_np(got[1]) != -2).all()
    _same(got, want, "no fallback")
    if k > Ng:
        assert (_np(got[1])[:, Ng:] == -1).all() and np.isneginf(_np(got[0])[:, Ng:]).all()


def test_the_device_quantiser_feeds_the_search():
    """ops.quantize_rows_i8 -> ops.similarity_topk_i8 end to end, fp16 source rows"""
    from cor_amd import ops
    G = torch.from_numpy(_gallery(4097, 128)[0]).to(torch.float16)
    Q = G[:9].float() * 1.5
    q, sc = ops.quantize_rows_i8(G.to(DEV))
    wq, ws = R.ref_quantize(G)
    _same(ops.similarity_topk_i8(Q.to(DEV), q, sc, 50), R.ref_search(Q.numpy(), wq, ws, 50))


# ------------------------------------------------------------------------------------------------------------------ ties and edge values

@pytest.mark.parametrize("offset", [0, BIG])
def test_ties_zero_scales_and_a_zero_query(offset):
    Ng, C = 70001, 64
    G, gq, gs = _gallery(Ng, C)
    gq, gs = gq.copy(), gs.copy()
    Q = G[[5, 20000, Ng - 3, 11]] * F(2.0)
    for a, b in ((5, 9), (5, 14), (5, 66), (20000, 45000), (20000, 69999), (Ng - 3, Ng - 1), (Ng - 3, 4)):   # inside a tile, across
        gq[b], gs[b] = gq[a], gs[a]                                                # tiles and slices, in the ragged last tile
    gs[[11, 12, 30000]] = 0.0                                                      # zero-scale rows: +0.0 or -0.0 by the sign of d
    gq[12] = -gq[11]
    Q = np.concatenate([Q, np.zeros((1, C), F)])                                   # a zero query: every score is 0.0, the index decides
    S = R.ref_scores(Q, gq, gs)[0]
    assert np.signbit(S[3, 11]) != np.signbit(S[3, 12]) and (S[4] == 0).all() and not np.signbit(S[4]).any()
    for k in (10, 100):
        want = R.ref_topk(S, k, offset)
        assert want[1][0, :4].tolist() == [offset + 5, offset + 9, offset + 14, offset + 66]
        assert want[1][4].tolist() == list(range(offset, offset + k))
        _same(_search(Q, gq, gs, k, offset), want, f"k={k}")


# ------------------------------------------------------------------------------------------------------------------ overflow

def test_overflow_takes_the_device_fallback():
    from cor_amd import _native
    Ng, C, k = 20000, 256, 100
    G, gq0, gs0 = _gallery(70001, C)
    gq, gs = np.repeat(gq0[:1], Ng, axis=0), np.repeat(gs0[:1], Ng)                # 20000 identical rows
    gq[[17, 4000]], gs[[17, 4000]] = gq0[[1, 2]], gs0[[1, 2]]
    Q = np.stack([G[0], G[1], -G[0]])
    want = R.ref_search(Q, gq, gs, k)
    assert want[1][1, 0] == 17 and want[1][0].tolist() == [i for i in range(102) if i != 17][:100]
    _same(_search(Q, gq, gs, k), want, "fallback")
    marked = _search(Q, gq, gs, k, flags=_native.TOPK_NO_FALLBACK)
    assert (_np(marked[1]) == -2).all() and np.isneginf(_np(marked[0])).all()


# ------------------------------------------------------------------------------------------------------------------ the Python API

def test_quantized_shard_api(tmp_path):
    from cor_amd import ops, retrieval
    G = torch.from_numpy(_gallery(4097, 64)[0])
    Q = (G[[3, 900, 4096]] + 0.01).to(DEV)
    shard = retrieval.GalleryShard(G.to(DEV), offset=1000, dtype=torch.bfloat16)
    before = shard.rows.clone()
    qs = shard.quantized()
    q, sc = ops.quantize_rows_i8(shard.rows)
    assert torch.equal(shard.rows, before) and isinstance(qs, retrieval.QuantizedShard)
    assert torch.equal(qs.rows, q) and torch.equal(qs.scales, sc) and qs.offset == 1000 and len(qs) == 4097
    assert qs.labels is None and qs.groups is None
    fr = retrieval.QuantizedShard.from_rows(shard.rows, offset=1000)
    assert torch.equal(fr.rows, q) and torch.equal(fr.scales, sc)
    s, i = qs.search(Q, 20)
    s2, i2 = ops.similarity_topk_i8(Q, q, sc, 20, g_offset=1000)
    assert torch.equal(i, i2) and torch.equal(s.view(torch.int32), s2.view(torch.int32))
    _same((s, i), R.ref_search(_np(Q), *R.ref_quantize(shard.rows), 20, 1000))
    with pytest.raises(ValueError):
        qs.search(Q, 5, query_labels=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError):
        qs.search(Q, 5, distinct=True)
    empty = retrieval.QuantizedShard.from_rows(shard.rows[:0], offset=7)
    es, ei = empty.search(Q, 4)
    assert len(empty) == 0 and (ei == -1).all() and torch.isneginf(es).all() and tuple(ei.shape) == (3, 4)
    # coarse stage of a two-stage search = the composition of the two calls
    fine = retrieval.GalleryShard(G.to(DEV), offset=1000)
    ts, ti = retrieval.two_stage_search(Q, qs, fine, 10, 50)
    _, ci = qs.search(Q, 50)
    fs, fi = fine.rescore(Q, ci, 10)
    assert torch.equal(ti, fi) and torch.equal(ts.view(torch.int32), fs.view(torch.int32)) and (ti[:, 0].cpu() == torch.tensor([1003, 1900, 5096])).all()
    # neighbours of a graph build and of an augmentation
    g8 = fine.neighbour_graph(8, batch=1500, neighbours=qs)
    assert g8.width == 8 and g8.lengths == (4097,)
    assert torch.equal(g8.kth[0][:1500].view(torch.int32), qs.search(fine.rows[:1500], 8)[0][:, 7].contiguous().view(torch.int32))
    aug = fine.augmented(3, batch=2000, neighbours=qs)
    s3, i3 = qs.search(fine.rows[:2000], 3)
    assert torch.equal(aug.rows[:2000], fine.expand(None, s3, i3, 3, query_weight=0.0))
    # disk round trip
    path = str(tmp_path / "gal")
    retrieval.save_gallery(path, qs.rows, world=2, scales=qs.scales)
    lo, hi = retrieval.shard_bounds(4097, 2, 1)
    back = retrieval.load_gallery_shard(path, 1, DEV)
    assert isinstance(back, retrieval.QuantizedShard) and back.offset == lo and len(back) == hi - lo
    assert torch.equal(back.rows, q[lo:hi]) and torch.equal(back.scales, sc[lo:hi])
    bs, bi = back.search(Q, 5)
    _same((bs, bi), R.ref_search(_np(Q), _np(q[lo:hi]), _np(sc[lo:hi]), 5, lo))


# ------------------------------------------------------------------------------------------------------------------ streams

def test_side_stream_and_graph_replay():
    from cor_amd import ops
    G, gq, gs = _gallery(40000, 256)
    rng = np.random.default_rng(3)
    Qa, Qb = (G[rng.integers(0, 40000, 33)] + F(0.2) * rng.standard_normal((33, 256)).astype(F) for _ in range(2))
    q, sc = torch.from_numpy(gq).to(DEV), torch.from_numpy(gs).to(DEV)
    Q = torch.from_numpy(Qa).to(DEV)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = ops.similarity_topk_i8(Q, q, sc, 100)                                # (also sets the kernels' one-time attributes before the capture)
    side.synchronize()
    _same(got, R.ref_search(Qa, gq, gs, 100), "side stream")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cs, ci = ops.similarity_topk_i8(Q, q, sc, 100)
    Q.copy_(torch.from_numpy(Qb).to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    _same((cs, ci), R.ref_search(Qb, gq, gs, 100), "graph replay")


def test_quantized_shard_in_a_one_rank_distributed_search():
    """distributed_search takes a QuantizedShard as its shard unchanged (one-rank nccl group, gather and deferred forms)."""
    import socket
    import torch.distributed as dist
    from cor_amd import retrieval
    if dist.is_initialized():
        pytest.skip("a process group already exists in this process")
    G = torch.from_numpy(_gallery(4097, 128)[0])
    Q = (G[[7, 4000, 12]] * 0.9).to(DEV)
    shard = retrieval.QuantizedShard.from_rows(G.to(DEV), offset=100)
    s0, i0 = shard.search(Q, 50)
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=torch.device(DEV))
    try:
        s1, i1 = retrieval.distributed_search(Q, shard, 50, max_local=8, always_collective=True)
        s2, i2 = retrieval.distributed_search(Q, shard, 50, max_local=8, always_collective=True, defer=True).result()
        torch.cuda.synchronize()
        for s_, i_ in ((s1, i1), (s2, i2)):
            assert torch.equal(i_, i0.cpu()) and torch.equal(s_.view(torch.int32), s0.cpu().view(torch.int32))
    finally:
        dist.destroy_process_group()

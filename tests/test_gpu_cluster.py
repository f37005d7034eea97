"""GPU tests of the clustering (cor_kmeans_seed, cor_kmeans_update, ops.kmeans_seed / kmeans_update, GalleryShard / QuantizedGallery /
GallerySet .cluster, Clustering). Every comparison is bitwise: centres, counts, score sums, ids and assignments. The reference is the CPU
restatement of the definitions, tests/cluster_refs.py, over the row values the kernels read (16-bit rows widened, int8 rows
float(q) * scale). The member-list build works in tiles of 2 048 rows and the sums in chunks of 256 members: the sizes below cross both."""
import numpy as np
import pytest
import torch

from tests.cluster_refs import planted, purity, ref_cluster, ref_seed, ref_update
from tests.i8_list_refs import widened

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KINDS = ["fp32", "bf16", "fp16", "int8"]
BIG = 2 ** 33 + 5
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def _bits(x):
    x = torch.as_tensor(x).cpu()
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def _same(got, want, what=""):
    """Two tuples of tensors / arrays (None allowed on both sides), compared bit for bit."""
    assert len(got) == len(want)
    for n, (g, w) in enumerate(zip(got, want)):
        assert (g is None) == (w is None), f"output {n} {what}"
        if g is not None:
            g, w = _bits(g), _bits(w)
            assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(g, w), f"output {n} differs {what}"


def _stored(G):
    """fp32 rows on the host -> per storage kind the segment as the ops take it (on the GPU, offset left out) and the fp32 values it stands for."""
    from cor_amd import ops
    q8, s8 = ops.quantize_rows_i8(G.to(DEV))
    stored = {"fp32": (G.to(DEV),), "bf16": (G.to(DEV, torch.bfloat16),), "fp16": (G.to(DEV, torch.float16),), "int8": (q8, s8)}
    values = {kind: widened([tuple(t.cpu() for t in seg) + (0,)])[0][0] for kind, seg in stored.items()}
    return stored, values


@pytest.fixture(scope="module")
def gallery():
    """5 000 unit rows per width: 40 loose modes, shuffled. Never modified."""
    out = {}
    for C in (64, 128, 256):
        g = torch.Generator().manual_seed(90 + C)
        centres = torch.nn.functional.normalize(torch.randn((40, C), generator=g), dim=-1)
        G = torch.nn.functional.normalize(centres[torch.randint(0, 40, (5000,), generator=g)] + 0.6 * torch.randn((5000, C), generator=g) / C ** 0.5, dim=-1)
        out[C] = (G.contiguous(),) + _stored(G.contiguous())
    return out


def _update(seg, off, a, K, sc=None, prev=None):
    from cor_amd import ops
    return ops.kmeans_update([seg + (off,)], [a.to(DEV)], K, scores=None if sc is None else [sc.to(DEV)], prev=None if prev is None else prev.to(DEV))


# ------------------------------------------------------------------------------------------------------------------ the centre step

@pytest.mark.parametrize("K", [1, 2, 33, 300])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000, 5000])
def test_update_sizes_widths_and_dtypes(gallery, n, K):
    """Random assignments that include -1 and K (no cluster); prev and scores given or not, by turns."""
    for nc, C in enumerate((64, 128, 256)):
        _, stored, values = gallery[C]
        for nk, kind in enumerate(KINDS):
            g = torch.Generator().manual_seed(n * 1000 + K + nc)
            a = torch.randint(-1, K + 1, (n,), generator=g, dtype=torch.int32)
            sc = torch.rand((n,), generator=g) if (nc + nk) % 2 == 0 else None
            prev = torch.randn((K, C), generator=g) if (nc + nk) % 3 != 0 else None
            off = BIG if nk % 2 else 0
            want = ref_update([(values[kind][:n], off)], [a.numpy()], K, scores=None if sc is None else [sc.numpy()],
                              prev=None if prev is None else prev.numpy())
            got = _update(tuple(t[:n] for t in stored[kind]), off, a, K, sc, prev)
            _same(got, want, f"n={n} K={K} C={C} {kind}")


@pytest.mark.parametrize("kind", KINDS)
def test_update_cluster_sizes_around_the_chunk(gallery, kind):
    """Clusters of exactly 0, 1, 255, 256, 257 and 513 members, interleaved, among rows that belong to no cluster."""
    _, stored, values = gallery[128]
    sizes = [0, 1, 255, 256, 257, 513]
    g = torch.Generator().manual_seed(4)
    a = torch.cat([torch.full((s,), c, dtype=torch.int32) for c, s in enumerate(sizes)] + [torch.tensor([-1, 6, INT_MIN, INT_MAX] * 50, dtype=torch.int32)])
    a = a[torch.randperm(a.shape[0], generator=g)]
    n = a.shape[0]
    sc = torch.rand((n,), generator=g)
    prev = torch.randn((6, 128), generator=g)
    want = ref_update([(values[kind][:n], 7)], [a.numpy()], 6, scores=[sc.numpy()], prev=prev.numpy())
    assert want[1].tolist() == sizes
    _same(_update(tuple(t[:n] for t in stored[kind]), 7, a, 6, sc, prev), want, kind)
    _same(_update(tuple(t[:n] for t in stored[kind]), 7, a, 6), ref_update([(values[kind][:n], 7)], [a.numpy()], 6), f"{kind}, no prev, no scores")


def test_update_one_cluster_holds_everything_and_values_out_of_range(gallery):
    _, stored, values = gallery[256]
    g = torch.Generator().manual_seed(6)
    sc = torch.rand((5000,), generator=g)
    prev = torch.randn((3, 256), generator=g)
    for kind in KINDS:
        a = torch.full((5000,), 1, dtype=torch.int32)
        want = ref_update([(values[kind], 0)], [a.numpy()], 3, scores=[sc.numpy()], prev=prev.numpy())
        assert want[1].tolist() == [0, 5000, 0]
        got = _update(stored[kind], 0, a, 3, sc, prev)
        _same(got, want, kind)
        assert torch.equal(_bits(got[0][[0, 2]]), _bits(prev[[0, 2]]))                       # the empty clusters: prev bit for bit
    hostile = torch.tensor([-1, 3, INT_MIN, INT_MAX, -2, 4, 2 ** 14, 2 ** 20, -2 ** 20], dtype=torch.int32)
    a = hostile[torch.randint(0, len(hostile), (5000,), generator=g)]
    got = _update(stored["bf16"], 0, a, 3, sc, None)
    assert got[1].tolist() == [0, 0, 0] and not got[0].any() and not got[2].any()            # nobody belongs anywhere: +0 rows, +0 sums
    assert not torch.signbit(got[0]).any() and not torch.signbit(got[2]).any()
    a[::7] = 2
    _same(_update(stored["bf16"], 0, a, 3, sc, None), ref_update([(values["bf16"], 0)], [a.numpy()], 3, scores=[sc.numpy()]), "a few members")


def test_update_segments_out_of_order_with_a_gap_and_mixed_dtypes(gallery):
    """Three segments (int8, fp32, bf16) given out of order, a gap in the ids and an empty segment, against the restatement, against one
    fp32 segment over the same values, and values exact in every dtype stored four ways."""
    from cor_amd import ops
    _, stored, values = gallery[64]
    g = torch.Generator().manual_seed(8)
    K = 9
    a = torch.randint(-1, K, (5000,), generator=g, dtype=torch.int32).to(DEV)
    sc = torch.rand((5000,), generator=g).to(DEV)
    cuts = (("bf16", 3100, 5000, BIG + 4000), ("int8", 0, 1300, BIG), ("fp16", 0, 0, 17), ("fp32", 1300, 3100, BIG + 1300))
    table = [tuple(t[lo:hi] for t in stored[kind]) + (off,) for kind, lo, hi, off in cuts]
    aa, ss = [a[lo:hi] for _, lo, hi, _ in cuts], [sc[lo:hi] for _, lo, hi, _ in cuts]
    vals = [(values[kind][lo:hi], off) for kind, lo, hi, off in cuts]
    want = ref_update(vals, [x.cpu().numpy() for x in aa], K, scores=[x.cpu().numpy() for x in ss])
    got = ops.kmeans_update(table, aa, K, scores=ss)
    _same(got, want, "three segments")
    order = [1, 3, 0]                                                                        # ascending id
    one = torch.from_numpy(np.concatenate([vals[n][0] for n in order])).to(DEV)
    _same(got, ops.kmeans_update([(one, 0)], [torch.cat([aa[n] for n in order])], K, scores=[torch.cat([ss[n] for n in order])]), "one fp32 segment")
    q = torch.randint(-64, 65, (3000, 64), generator=g)
    v = (q.float() / 64).contiguous()
    a3 = a[:3000]
    ways = {"fp32": (v.to(DEV),), "bf16": (v.to(DEV, torch.bfloat16),), "fp16": (v.to(DEV, torch.float16),),
            "int8": (q.to(DEV, torch.int8), torch.full((3000,), 1 / 64, device=DEV))}
    want = ref_update([(v.numpy(), 5)], [a3.cpu().numpy()], K)
    for kind, seg in ways.items():
        _same(ops.kmeans_update([seg + (5,)], [a3], K), want, f"exact values as {kind}")
    parts = [tuple(t[lo:hi] for t in ways[kind]) + (5 + lo,) for kind, (lo, hi) in zip(KINDS, ((0, 10), (10, 2048), (2048, 2049), (2049, 3000)))]
    _same(ops.kmeans_update(parts[::-1], [a3[2049:], a3[2048:2049], a3[10:2048], a3[:10]], K), want, "one kind per segment")


@pytest.mark.parametrize("kind", ["bf16", "fp32"])
def test_update_spans_several_tiles(kind):
    """20 000 x 256 rows, K = 512: ten tiles of the member-list build, clusters whose members lie in every tile, and one skewed cluster."""
    g = torch.Generator().manual_seed(11)
    G = torch.nn.functional.normalize(torch.randn((20000, 256), generator=g), dim=-1)
    rows = G.to(DEV, torch.bfloat16 if kind == "bf16" else torch.float32)
    a = torch.randint(0, 512, (20000,), generator=g, dtype=torch.int32)
    a[torch.rand((20000,), generator=g) < 0.3] = 77                                          # ~6 000 members: 24 chunks
    a[2040:2060] = 511                                                                       # a run across the first tile boundary
    sc = torch.rand((20000,), generator=g)
    want = ref_update([(rows.cpu().float().numpy(), BIG)], [a.numpy()], 512, scores=[sc.numpy()])
    assert want[1][77] > 5000 and want[1].min() > 0
    _same(_update((rows,), BIG, a, 512, sc), want, kind)


def test_update_on_a_side_stream_and_in_a_replayed_graph(gallery):
    from cor_amd import ops
    _, stored, values = gallery[128]
    seg = stored["fp16"] + (0,)
    g = torch.Generator().manual_seed(13)
    assigns = [torch.randint(-1, 20, (5000,), generator=g, dtype=torch.int32).to(DEV) for _ in range(3)]
    sc = torch.rand((5000,), generator=g).to(DEV)
    prev = torch.randn((20, 128), generator=g).to(DEV)
    wants = [ref_update([(values["fp16"], 0)], [a.cpu().numpy()], 20, scores=[sc.cpu().numpy()], prev=prev.cpu().numpy()) for a in assigns]
    run = lambda a: ops.kmeans_update([seg], [a], 20, scores=[sc], prev=prev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = run(assigns[0])
    side.synchronize()
    _same(got, wants[0], "side stream")
    ain = assigns[0].clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                                            # one capture stream
        out = run(ain)
    for n in (1, 2, 0):                                                                      # replayed with new assignments
        ain.copy_(assigns[n])
        graph.replay()
        torch.cuda.synchronize()
        _same(out, wants[n], f"replay with assignment {n}")
    assert not torch.equal(torch.as_tensor(wants[0][1]), torch.as_tensor(wants[1][1]))


# ------------------------------------------------------------------------------------------------------------------ the seeding

@pytest.mark.parametrize("n,K", [(1, 1), (2, 1), (2, 2), (1000, 1), (1000, 2), (1000, 33), (5000, 1), (5000, 2), (5000, 33)])
def test_seed_sizes_and_dtypes(gallery, n, K):
    from cor_amd import ops
    for nc, C in enumerate((64, 128, 256)):
        _, stored, values = gallery[C]
        for nk, kind in enumerate(KINDS):
            off = BIG if (nc + nk) % 2 else 0
            first = None if nk % 2 else off + (n * 3) // 7                                    # a first id that is not the smallest
            want = ref_seed([(values[kind][:n], off)], K, first)
            assert want[0][0] == (off if first is None else first) and len(set(want[0].tolist())) == K
            _same(ops.kmeans_seed([tuple(t[:n] for t in stored[kind]) + (off,)], K, first_id=first), want, f"n={n} K={K} C={C} {kind}")


def test_seed_every_row_and_identical_rows(gallery):
    from cor_amd import ops
    _, stored, values = gallery[64]
    for kind in KINDS:                                                                       # K = n: every row once, the twin of nobody
        ids, cent = ops.kmeans_seed([tuple(t[:300] for t in stored[kind]) + (50,)], 300)
        _same((ids, cent), ref_seed([(values[kind][:300], 50)], 300), f"K = n, {kind}")
        assert sorted(ids.tolist()) == list(range(50, 350))
    same = stored["fp32"][0][7:8].expand(64, 64).contiguous()                                # 64 identical rows: every best ties
    ids, cent = ops.kmeans_seed([(same, 100)], 64)
    assert ids.tolist() == list(range(100, 164)) and torch.equal(cent, same)                 # the smallest id, a chosen row never again
    ids, _ = ops.kmeans_seed([(same, 100)], 64, first_id=130)
    assert ids.tolist() == [130] + list(range(100, 130)) + list(range(131, 164))
    twins = torch.cat([stored["fp32"][0][:40], stored["fp32"][0][:40]])                      # every row twice: the twins come last
    ids, _ = ops.kmeans_seed([(twins, 0)], 80)
    _same((ids,), (ref_seed([(twins.cpu().numpy(), 0)], 80)[0],), "twins")
    assert sorted(i % 40 for i in ids[:40].tolist()) == list(range(40))


def test_seed_segments_out_of_order_with_a_gap_and_mixed_dtypes(gallery):
    from cor_amd import ops
    _, stored, values = gallery[256]
    cuts = (("bf16", 3100, 5000, BIG + 4000), ("int8", 0, 1300, BIG), ("fp16", 0, 0, 17), ("fp32", 1300, 3100, BIG + 1300))
    table = [tuple(t[lo:hi] for t in stored[kind]) + (off,) for kind, lo, hi, off in cuts]
    vals = [(values[kind][lo:hi], off) for kind, lo, hi, off in cuts]
    for first in (None, BIG + 4000 + 1899, BIG + 1300):
        want = ref_seed(vals, 25, first)
        got = ops.kmeans_seed(table, 25, first_id=first)
        _same(got, want, f"three segments, first_id={first}")
        _same(ops.kmeans_seed(table[::-1], 25, first_id=first), want, "the table reversed")
    one = torch.from_numpy(np.concatenate([vals[n][0] for n in (1, 3, 0)])).to(DEV)          # the same rows as one fp32 segment, ids 0 ..
    ids1, cent1 = ops.kmeans_seed([(one, 0)], 25)
    ids0, cent0 = ops.kmeans_seed(table, 25)
    back = torch.where(ids0 >= BIG + 4000, ids0 - BIG - 4000 + 3100, ids0 - BIG)
    assert torch.equal(back, ids1) and torch.equal(_bits(cent0), _bits(cent1))
    g = torch.Generator().manual_seed(3)
    q = torch.randint(-64, 65, (500, 64), generator=g)
    v = (q.float() / 64).contiguous()
    want = ref_seed([(v.numpy(), 9)], 30)
    for kind, seg in {"fp32": (v.to(DEV),), "bf16": (v.to(DEV, torch.bfloat16),), "fp16": (v.to(DEV, torch.float16),),
                      "int8": (q.to(DEV, torch.int8), torch.full((500,), 1 / 64, device=DEV))}.items():
        _same(ops.kmeans_seed([seg + (9,)], 30), want, f"exact values as {kind}")


def test_seed_on_a_side_stream_and_in_a_replayed_graph(gallery):
    from cor_amd import ops
    _, stored, values = gallery[64]
    rows = [stored["bf16"][0][lo:lo + 1000].clone() for lo in (0, 1000, 2000)]
    wants = [ref_seed([(values["bf16"][lo:lo + 1000], 0)], 12) for lo in (0, 1000, 2000)]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = ops.kmeans_seed([(rows[0], 0)], 12)
    side.synchronize()
    _same(got, wants[0], "side stream")
    rin = rows[0].clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.kmeans_seed([(rin, 0)], 12)
    for n in (1, 2, 0):
        rin.copy_(rows[n])
        graph.replay()
        torch.cuda.synchronize()
        _same(out, wants[n], f"replay with rows {n}")


# ------------------------------------------------------------------------------------------------------------------ the loop

def _galleries(G, off=0):
    """The same rows as a bf16 shard, an int8-only gallery and a mixed set (fp32 / int8 / fp16 segments given out of order) -> [(name,
    gallery, the widened segments in offset order)]"""
    from cor_amd.retrieval import GallerySet, GalleryShard, QuantizedGallery, QuantizedShard
    stored, values = _stored(G)
    n = G.shape[0]
    a, b = n // 3, (2 * n) // 3
    shard = GalleryShard(stored["bf16"][0], offset=off)
    i8 = QuantizedGallery(*stored["int8"], offset=off)
    mixed = GallerySet([GalleryShard(stored["fp16"][0][b:], offset=off + b), GalleryShard(stored["fp32"][0][:a], offset=off),
                        QuantizedShard(stored["int8"][0][a:b], stored["int8"][1][a:b], offset=off + a)])
    return [("shard", shard, [(values["bf16"], off)]), ("int8", i8, [(values["int8"], off)]),
            ("set", mixed, [(values["fp32"][:a], off), (values["int8"][a:b], off + a), (values["fp16"][b:], off + b)])]


def _same_clustering(got, want, what):
    assign = got.assign if isinstance(got.assign, list) else [got.assign]
    assert all(a.dtype == torch.int32 for a in assign)
    _same((got.centroids.rows, got.counts) + tuple(assign), (want["centroids"], want["counts"]) + tuple(want["assign"]), what)
    assert got.objective == want["objective"] and got.iters == want["iters"] and got.converged == want["converged"], what
    assert got.centroids.offset == 0 and got.centroids.rows.dtype == torch.float32


@pytest.fixture(scope="module")
def fixture_rows():
    X, mode, d = planted()
    return torch.from_numpy(X), mode, d


def test_cluster_the_planted_fixture(fixture_rows):
    """The purpose fixture through .cluster of a shard, an int8 gallery and a mixed set: bitwise the restatement's loop, and the planted
    modes come back (the bf16 / int8 roundings move no row to another mode)."""
    G, mode, _ = fixture_rows
    for name, gal, segs in _galleries(G, off=1000):
        want = ref_cluster(segs, 30)
        got = gal.cluster(30)
        _same_clustering(got, want, name)
        assign = torch.cat(got.assign) if isinstance(got.assign, list) else got.assign
        assert got.converged and got.iters <= 20 and purity(assign.cpu().numpy(), mode, 30) == 1.0 and (got.counts == 100).all()
        assert all(b - a >= -1e-6 for a, b in zip(got.objective, got.objective[1:]))


def test_cluster_a_random_gallery_and_a_given_start(gallery):
    """5 000 x 256 rows at K = 45, a few passes (the restatement walks 5 000 x 45 chains per pass); first_id, batch sizes that do not divide
    the rows, and init as a tensor."""
    G = gallery[256][0]
    for name, gal, segs in _galleries(G):
        want = ref_cluster(segs, 45, iters=3, first_id=4321)
        _same_clustering(gal.cluster(45, iters=3, first_id=4321, batch=1777), want, name)
        assert not want["converged"] and want["iters"] == 3
    name, gal, segs = _galleries(G[:1500])[2]
    g = torch.Generator().manual_seed(2)
    init = torch.nn.functional.normalize(torch.randn((7, 256), generator=g), dim=-1)
    want = ref_cluster(segs, 7, iters=25, init=init.numpy())
    got = gal.cluster(7, iters=25, init=init.to(DEV), batch=4096)
    _same_clustering(got, want, "init as a tensor")
    got_cpu_init = gal.cluster(7, iters=25, init=init)                                       # a host tensor is moved
    _same_clustering(got_cpu_init, want, "init as a host tensor")
    one = gal.cluster(7, iters=1, init=init.to(DEV))
    assert one.iters == 1 and not one.converged and len(one.objective) == 1 and one.objective[0] == want["objective"][0]


# ------------------------------------------------------------------------------------------------------------------ the uses

def test_cluster_ids_as_groups_and_labels(fixture_rows):
    """With the cluster ids as `groups`, a distinct search returns rows of 10 different planted directions where the plain top-10 returns
    10 of one; as `labels` with mode "eq" and the query's own cell, only rows of that cell come back."""
    from cor_amd.retrieval import GalleryShard
    G, mode, d = fixture_rows
    rows = G.to(DEV)
    cl = GalleryShard(rows).cluster(30)
    assert cl.assign.shape == (3000,) and cl.assign.dtype == torch.int32
    q = torch.from_numpy(d[:8]).to(DEV)
    plain = GalleryShard(rows).search(q, 10)[1].cpu().numpy()
    diverse = GalleryShard(rows, groups=cl.assign).search(q, 10, distinct=True)[1].cpu().numpy()
    for b in range(8):
        assert len(set(mode[plain[b]].tolist())) == 1 and mode[plain[b, 0]] == b
        assert len(set(mode[diverse[b]].tolist())) == 10 and mode[diverse[b, 0]] == b
    cs, cell = cl.assign_queries(q)
    assert cell.shape == (8, 1) and cell.dtype == torch.int64 and len(set(cell[:, 0].tolist())) == 8
    labelled = GalleryShard(rows, labels=cl.assign)
    s, i = labelled.search(q, 100, query_labels=cell[:, 0].to(torch.int32), mode="eq")
    assert (i >= 0).all() and torch.equal(cl.assign[i.reshape(-1)].reshape(8, 100).long(), cell.expand(8, 100))
    s, i = labelled.search(q, 100, query_labels=cell[:, 0].to(torch.int32), mode="ne")
    assert (cl.assign[i.reshape(-1)].reshape(8, 100).long() != cell).all()
    assert torch.equal(cl.assign[labelled.search(q, 1)[1][:, 0]].long(), cell[:, 0])      # the nearest row lies in the query's own cell

"""GPU tests of the cell-probing search (cor_ivf_build, cor_ivf_search, ops.ivf_build / ivf_search, retrieval.IVFIndex and .ivf). Every
comparison is bitwise: stored rows, scales, ids, cell starts, score bits, result ids and the scanned counts. The reference is the CPU
restatement tests/ivf_refs.py, which gathers a query's candidate rows in ascending id and runs the dtype's own exact-search restatement.
The scan works in tiles of 512 slots and keeps 2 048 keys in LDS: the cell sizes below sit one below, at and one above both."""
import numpy as np
import pytest
import torch

from tests.i8_refs import ref_quantize
from tests.ivf_refs import ref_exact, ref_ivf_build, ref_ivf_search

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KINDS = ["fp32", "bf16", "fp16", "int8"]
BIG = 2 ** 33 + 5
INT_MIN, INT64_MIN = -2 ** 31, -2 ** 63
SIZES = [0, 1, 511, 512, 513, 2047, 2048, 2049, 255, 256, 257, 3, 700, 0, 40, 100, 100, 100, 100, 100]     # cells of the main index
K0 = len(SIZES)


def _raw(t):
    return torch.as_tensor(t).cpu().contiguous().view(torch.uint8)


def _bits(x):
    x = torch.as_tensor(x).cpu()
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def _same(got, want, what=""):
    assert len(got) == len(want)
    for n, (g, w) in enumerate(zip(got, want)):
        g, w = _bits(g), _bits(w)
        assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(g, w), f"output {n} differs {what}"


def _unit(n, C, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn((n, C), generator=g), dim=-1).contiguous()


def _store(X, kind):
    """fp32 rows on the host -> the host segment payload of that kind: (rows,) or (rows int8, scales ndarray)"""
    if kind == "int8":
        q, sc = ref_quantize(X)
        return (torch.from_numpy(q), sc)
    return (X.to({"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}[kind]),)


def _dev_seg(seg):
    return tuple(torch.as_tensor(t).to(DEV) for t in seg[:-1]) + (seg[-1],)


class Index:
    """An index built on the GPU from host segments, checked bit for bit against the restatement, with both copies kept."""

    def __init__(self, segs, assigns, K):
        from cor_amd import ops
        self.K = K
        self.host = ref_ivf_build(segs, assigns, K)
        self.dev = ops.ivf_build([_dev_seg(s) for s in segs], [torch.as_tensor(a).to(DEV) for a in assigns], K)
        rows, scales, ids, cs = self.host
        m = int(cs[K])
        n = sum(s[0].shape[0] for s in segs)
        assert self.dev[0].shape == (n, segs[0][0].shape[1]) and self.dev[0].dtype == segs[0][0].dtype and self.dev[2].shape == (n,)
        assert torch.equal(self.dev[3].cpu(), torch.from_numpy(cs)), "cell_start"
        assert torch.equal(_raw(self.dev[0][:m]), _raw(rows)), "stored rows"
        assert torch.equal(self.dev[2][:m].cpu(), torch.from_numpy(ids)), "ids"
        assert (self.dev[1] is None) == (scales is None)
        if scales is not None:
            assert torch.equal(_bits(self.dev[1][:m]), _bits(torch.from_numpy(scales))), "scales"
        self.max_cell = max(int(np.diff(cs).max()), 1)

    def check(self, Q, probes, k, max_cell=None, split=0, what="", want=None):
        from cor_amd import ops
        probes = torch.as_tensor(probes, dtype=torch.int64)
        want = ref_ivf_search(Q.numpy(), *self.host, probes.numpy(), k) if want is None else want
        got = ops.ivf_search(Q.to(DEV), *self.dev, probes.to(DEV), k, self.max_cell if max_cell is None else max_cell, split=split, return_scanned=True)
        _same(got, want, what)
        return want


def _main_assign(n_extra=50, seed=5):
    a = np.concatenate([np.full(s, c, np.int32) for c, s in enumerate(SIZES)] + [np.array([-1, K0, INT_MIN, K0 + 7, -5] * (n_extra // 5), np.int32)])
    return a[np.random.default_rng(seed).permutation(a.shape[0])]


_CACHE = {}


def main_index(kind, C):
    """The main index of a kind and width: the cell sizes SIZES, 50 rows in no cell, one segment at a large offset. Built once."""
    if (kind, C) not in _CACHE:
        a = _main_assign()
        _CACHE[kind, C] = Index([_store(_unit(a.shape[0], C, 100 + C), kind) + (BIG,)], [a], K0)
    return _CACHE[kind, C]


def _probes_of(Q, C, K, nprobe, seed=17):
    """What a search of the queries over K centres returns for k = nprobe: with nprobe > K the list carries a -1 tail"""
    from cor_amd import ops
    return ops.similarity_topk(Q.to(DEV), _unit(K, C, seed).to(DEV), nprobe)[1].cpu()


# ------------------------------------------------------------------------------------------------------------------ the build

@pytest.mark.parametrize("C", [16, 64, 256])
@pytest.mark.parametrize("kind", KINDS)
def test_build_widths_and_dtypes(kind, C):
    main_index(kind, C)                                                                      # the constructor compares every output


@pytest.mark.parametrize("kind", KINDS)
def test_build_does_not_depend_on_the_segmentation(kind):
    """Three segments given out of offset order and an empty one: the index of the same (id, row) pairs in one segment."""
    from cor_amd import ops
    n, C, K = 5000, 64, 37
    X = _unit(n, C, 7)
    a = np.random.default_rng(8).integers(-1, K + 1, n).astype(np.int32)
    a[:5] = [INT_MIN, -1, K, K + 1, 0]
    cuts = [(3001, n, 1000), (0, 3000, BIG), (3000, 3001, 5)]                                # (lo, hi, offset)
    full = _store(X, kind)
    segs = [tuple(t[lo:hi] for t in full) + (off,) for lo, hi, off in cuts] + [tuple(t[:0] for t in full) + (77,)]
    cut = Index(segs, [a[lo:hi] for lo, hi, _ in cuts] + [a[:0]], K)
    # the same pairs as ONE segment: ids are offset + local, so lay the rows out by ascending id with the gaps left to rows in no cell
    ids = np.zeros(n, np.int64)
    for lo, hi, off in cuts:
        ids[lo:hi] = np.arange(hi - lo) + off                                                # the global id of every original row
    order = np.argsort(ids)
    dense = {int(g): n_ for n_, g in enumerate(ids[order])}
    rows1 = tuple(torch.as_tensor(t)[torch.from_numpy(order)] for t in full)
    one = ref_ivf_build([rows1 + (0,)], [a[order]], K)
    assert torch.equal(_raw(one[0]), _raw(cut.host[0])) and np.array_equal(one[3], cut.host[3])
    assert np.array_equal(np.array([dense[int(g)] for g in cut.host[2]]), one[2])            # the same rows in the same slots, ids renamed


@pytest.mark.parametrize("kind", ["bf16", "int8"])
def test_build_and_search_of_no_rows(kind):
    from cor_amd import ops
    full = _store(_unit(4, 64, 1), kind)
    idx = Index([tuple(t[:0] for t in full) + (0,)], [np.zeros(0, np.int32)], 6)
    assert idx.dev[0].shape == (0, 64) and torch.equal(idx.dev[3].cpu(), torch.zeros(7, dtype=torch.int32))
    s, i, sc = idx.check(_unit(3, 64, 2), np.tile(np.arange(6), (3, 1)), 4, what="an empty index")
    assert np.all(i == -1) and np.all(sc == 0)
    rest = Index([full + (10,)], [np.full(4, -1, np.int32)], 6)                              # rows, none of them in a cell
    assert int(rest.dev[3][-1]) == 0
    rest.check(_unit(3, 64, 2), np.tile(np.arange(6), (3, 1)), 4, what="no row indexed")


# ------------------------------------------------------------------------------------------------------------------ the search

@pytest.mark.parametrize("C", [16, 64, 256])
@pytest.mark.parametrize("kind", KINDS)
def test_search_k_and_nprobe(kind, C):
    idx = main_index(kind, C)
    Q = _unit(5, C, 300 + C)
    for k, nprobe in ((1, 1), (10, 2), (32, K0), (33, 256), (256, 2), (256, 256), (10, 8)):
        idx.check(Q, _probes_of(Q, C, K0, nprobe), k, what=f"k={k} nprobe={nprobe} {kind} C={C}")
    # k above the candidate count: the cell of one row, the empty cells, both
    for cells in ([1], [0], [13, 0], [1, 0, 11], [1, 1, 1]):
        s, i, sc = idx.check(Q, np.tile(np.array(cells), (5, 1)), 10, what=f"cells {cells} {kind} C={C}")
        m = sum(SIZES[c] for c in set(cells))
        assert np.all(sc == m) and np.all(i[:, m:] == -1) and np.all(i[:, :m] >= BIG)
    # every cell of every size on its own
    for c in range(K0):
        idx.check(Q, np.full((5, 1), c), 33, what=f"cell {c} of {SIZES[c]} rows {kind} C={C}")


@pytest.mark.parametrize("kind", KINDS)
def test_split_and_max_cell_change_no_bit(kind):
    """One block walks a cell of 2 049 rows to its end (split = 1, max_cell = 1), or the cell is cut into slices; 1 .. 4 096 partial lists."""
    idx = main_index(kind, 64)
    Q = _unit(3, 64, 41)
    probes = np.stack([np.arange(K0), np.array([7, 6, 5] + [7] * (K0 - 3)), np.array([12, 2] + [-1] * (K0 - 2))])
    for k in (1, 10, 256):
        want = None
        for split in (1, 3, 4096 // k, 0):
            for max_cell in (1, 300, idx.max_cell, 2 ** 31 - 1):
                want = idx.check(Q, probes, k, max_cell=max_cell, split=split, what=f"k={k} split={split} max_cell={max_cell} {kind}", want=want)


@pytest.mark.parametrize("kind", ["fp32", "bf16", "int8"])
def test_hostile_probes_are_ignored(kind):
    idx = main_index(kind, 64)
    Q = _unit(6, 64, 43)
    bad = [INT64_MIN, -1, K0, 2 ** 40, 2 ** 63 - 1, K0 + 2 ** 32, -K0]
    rows = [bad + [4, 9],                                     # at the head
            [4] + bad + [9],                                  # in the middle
            [4, 9] + bad,                                     # at the tail
            bad + [-1, -1],                                   # nothing else
            [9, 9, 4, 9, 4, 4, 9, 2, 2],                      # repeated cells
            [2 ** 32 + 4, 4, INT64_MIN, 4, 2 ** 32 + 4, -1, 9, K0, 9]]
    want = idx.check(Q, np.array(rows, dtype=np.int64), 40, what=f"hostile probes {kind}")
    assert np.all(want[2] == [SIZES[4] + SIZES[9]] * 3 + [0, SIZES[9] + SIZES[4] + SIZES[2], SIZES[4] + SIZES[9]])
    assert np.all(want[1][3] == -1)


@pytest.mark.parametrize("kind", KINDS)
def test_ties_go_to_the_smaller_id(kind):
    n, C, K = 3000, 64, 7
    X = _unit(n, C, 51)
    X[1::2] = X[0::2]                                                                        # every row twice ...
    a = (np.arange(n) % K).astype(np.int32)                                                  # ... in different cells (K is odd)
    idx = Index([_store(X, kind) + (BIG,)], [a], K)
    Q = _unit(4, C, 52)
    for k in (2, 10, 256):
        want = idx.check(Q, np.tile(np.arange(K), (4, 1)), k, split=3, what=f"twins k={k} {kind}")
        assert np.all(want[1][:, 1:k:2] == want[1][:, 0:k:2] + 1)                            # a twin follows its twin
        idx.check(Q, np.tile(np.array([0, 3, 5]), (4, 1)), k, what=f"twins in three cells k={k} {kind}")
    # all scores equal: 3 000 copies of one row, only the id decides; every append passes the threshold
    same = Index([_store(X[:1].expand(n, C).contiguous(), kind) + (9,)], [a], K)
    for k, split in ((1, 1), (10, 0), (256, 1), (256, 5)):
        want = same.check(Q, np.tile(np.arange(K), (4, 1)), k, max_cell=1, split=split, what=f"equal scores k={k} {kind}")
        assert np.all(want[1] == 9 + np.arange(k))
    # a zero query: every score is a zero
    Z = torch.zeros((2, C))
    want = idx.check(Z, np.tile(np.arange(K), (2, 1)), 256, what=f"zero query {kind}")
    assert np.all(want[0] == 0) and np.all(want[1] == BIG + np.arange(256))


def test_int8_zero_scores_rank_by_their_bits():
    """Hand-made row scales of both signs and a zero query: +0.0 and -0.0 scores, which the int8 order keeps apart (+0.0 first)."""
    n, C, K = 300, 64, 5
    q, sc = ref_quantize(_unit(n, C, 61))
    sc = np.where(np.arange(n) % 3 == 0, -sc, sc).astype(np.float32)
    idx = Index([(torch.from_numpy(q), sc, 100)], [(np.arange(n) % K).astype(np.int32)], K)
    for kw in (dict(split=4), dict(max_cell=1, split=1), dict()):
        want = idx.check(torch.zeros((2, C)), np.tile(np.arange(K), (2, 1)), 256, what=f"signed zeros {kw}", **kw)
        assert np.all(want[0] == 0) and not np.any(np.signbit(want[0][:, :200])) and np.all(np.signbit(want[0][:, 200:]))
        assert np.all(want[1][:, :200] % 3 != 1) and np.all(want[1][:, 200:] == 100 + 3 * np.arange(56))   # ids 100 + 3 j carry -0.0 and come last
    Q = _unit(2, C, 62)
    idx.check(Q, np.tile(np.arange(K), (2, 1)), 256, what="negative scales")


@pytest.mark.parametrize("Bq", [0, 1, 2, 65, 257])
def test_batch_sizes(Bq):
    for kind in ("bf16", "int8"):
        idx = main_index(kind, 64)
        Q = _unit(max(Bq, 1), 64, 70 + Bq)[:Bq]
        probes = torch.from_numpy(np.random.default_rng(Bq).integers(0, K0, (Bq, 3)))
        want = idx.check(Q, probes, 10, what=f"Bq={Bq} {kind}")
        assert want[0].shape == (Bq, 10)


def test_search_on_a_side_stream_and_in_a_replayed_graph():
    from cor_amd import ops
    for kind in ("fp16", "int8"):
        idx = main_index(kind, 64)
        Qs = [_unit(9, 64, 80 + n) for n in range(3)]
        Ps = [torch.from_numpy(np.random.default_rng(n).integers(-1, K0 + 1, (9, 6))) for n in range(3)]
        wants = [ref_ivf_search(Q.numpy(), *idx.host, P.numpy(), 20) for Q, P in zip(Qs, Ps)]
        run = lambda q, p: ops.ivf_search(q, *idx.dev, p, 20, idx.max_cell, return_scanned=True)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            got = run(Qs[0].to(DEV), Ps[0].to(DEV))
        side.synchronize()
        _same(got, wants[0], f"side stream {kind}")
        qin, pin = Qs[0].to(DEV), Ps[0].to(DEV)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = run(qin, pin)
        for n in (1, 2, 0):                                                                  # replayed with new queries and probes
            qin.copy_(Qs[n])
            pin.copy_(Ps[n])
            graph.replay()
            torch.cuda.synchronize()
            _same(out, wants[n], f"replay {n} {kind}")


# ------------------------------------------------------------------------------------------------------------------ the Python layer

def _galleries(X, off):
    """The same rows as a bf16 shard, an int8-only gallery and a set of three fp16 segments given out of order -> [(name, gallery)]"""
    from cor_amd import retrieval as R
    n = X.shape[0]
    cuts = [(2000, n), (0, 1200), (1200, 2000)]
    return [("bf16 shard", R.GalleryShard(X.to(DEV), offset=off, dtype=torch.bfloat16)),
            ("int8 gallery", R.QuantizedGallery.from_rows(X.to(DEV), offset=off)),
            ("fp16 set", R.GallerySet([R.GalleryShard(X[lo:hi].to(DEV), offset=off + lo, dtype=torch.float16) for lo, hi in cuts]))]


def test_ivf_index_against_the_ops_and_the_exact_search():
    from cor_amd import ops
    from cor_amd import retrieval as R
    X, Q = _unit(5000, 256, 91), _unit(33, 256, 92).to(DEV)                                  # C = 256: there the exact search of 16-bit rows is chain-exact at every k
    for name, gal in _galleries(X, BIG):
        index = gal.ivf(24, nprobe=5, iters=2)
        assert isinstance(index, R.IVFIndex) and index.n_cells == 24 and len(index) == 5000 and index.nprobe == 5
        counts = index.counts.cpu()
        assert int(counts.sum()) == 5000 and index.max_cell == int(counts.max()) and torch.equal(index.cell_start.cpu()[1:], counts.cumsum(0).int())
        # the class is the composition it documents
        for nprobe in (None, 1, 24, 300):
            probes = index.centroids.search(Q, min(5 if nprobe is None else nprobe, 24))[1]
            want = ops.ivf_search(Q, index.rows, index.scales, index.ids, index.cell_start, probes, 10, index.max_cell, return_scanned=True)
            _same(index.search(Q, 10, nprobe=nprobe, return_scanned=True), want, f"{name} nprobe={nprobe}")
            _same(index.search(Q, 10, nprobe=nprobe), want[:2], f"{name} nprobe={nprobe}, two outputs")
        # every cell probed: the gallery's own exact search
        for k in (1, 10, 256):
            _same(index.search(Q, k, nprobe=24), gal.search(Q, k), f"{name} k={k} against the exact search")
        s, i, sc = index.search(Q[:0], 7, return_scanned=True)
        assert s.shape == (0, 7) and i.shape == (0, 7) and sc.shape == (0,)
        with pytest.raises(ValueError):
            index.search(Q, 0)
        with pytest.raises(ValueError):
            index.search(Q, 10, nprobe=0)
    # the pair of centres and assignment in place of a Clustering; rows with assign -1 are left out
    name, gal = _galleries(X, 0)[0]
    cl = gal.cluster(24, iters=2)
    a = cl.assign.clone()
    a[::10] = -1
    index = R.IVFIndex.build(gal, centroids=cl.centroids.rows, assign=a, nprobe=24)
    keep = torch.ones(5000, dtype=torch.bool)
    keep[::10] = False
    part = R.GalleryShard(gal.rows[keep.to(DEV)], offset=0)
    s, i = part.search(Q, 10)
    kept = torch.arange(5000)[keep].to(DEV)
    _same(index.search(Q, 10), (s, kept[i]), "a tenth of the rows left out")
    with pytest.raises(ValueError):
        R.IVFIndex.build(gal, cl, nprobe=0)
    with pytest.raises(ValueError):
        R.IVFIndex.build(gal, centroids=cl.centroids, assign=a[:-1])


def test_two_stage_search_takes_an_ivf_index_as_coarse():
    from cor_amd import retrieval as R
    X, Q = _unit(5000, 64, 93), _unit(17, 64, 94).to(DEV)
    fine = R.GalleryShard(X.to(DEV), offset=BIG)
    index = fine.ivf(16, nprobe=4, iters=2)
    got = R.two_stage_search(Q, index, fine, 10, 50)
    _, cand = index.search(Q, 50)
    _same(got, fine.rescore(Q, cand, 10), "two-stage over an IVF coarse stage")
    assert torch.all(got[1] >= BIG)
    _same(R.two_stage_search(Q, index, fine, 10, 50, nprobe=16), R.two_stage_search(Q, fine, fine, 10, 50), "all cells probed, fp32 master rows")


def test_purpose_the_index_reproduces_the_reference_lists():
    """The purpose fixture of tests/test_cpu_ivf.py on the GPU: the same planted rows, clustering and queries; the lists the index returns
    at every nprobe are the reference's, bit for bit (so are its recall and its share of rows scanned)."""
    from cor_amd import retrieval as R
    from tests.test_cpu_ivf import purpose_fixture
    x, cl, Q, order = purpose_fixture()
    gal = R.GalleryShard(torch.from_numpy(x).to(DEV), offset=0)
    index = R.IVFIndex.build(gal, centroids=torch.from_numpy(cl["centroids"]).to(DEV), assign=torch.from_numpy(cl["assign"][0]).to(DEV))
    host = ref_ivf_build([(torch.from_numpy(x), 0)], cl["assign"], 64)
    assert torch.equal(index.cell_start.cpu(), torch.from_numpy(host[3])) and torch.equal(index.ids.cpu(), torch.from_numpy(host[2]))
    for nprobe in (1, 2, 4, 8, 16, 64):
        want = ref_ivf_search(Q, *host, order[:, :nprobe], 10)
        _same(index.search(torch.from_numpy(Q).to(DEV), 10, nprobe=nprobe, return_scanned=True), want, f"nprobe={nprobe}")
    _same(index.search(torch.from_numpy(Q).to(DEV), 10, nprobe=64), ref_exact(Q, host[0], None, host[2], 10), "nprobe = K: the exact search")

"""GPU tests of the diffusion re-ranking (cor_rerank_diffusion, ops.rerank_diffusion, GalleryShard / QuantizedGallery / GallerySet .diffuse,
retrieval.diffused_search). Every comparison is bitwise, on score bits, ids and positions. The reference is the CPU restatement of the
definition, tests/diffuse_refs.py, over the row values the kernel sums (16-bit rows widened, int8 rows float(q) * scale)."""
import numpy as np
import pytest
import torch

from tests.diffuse_refs import ref_diffusion
from tests.i8_list_refs import widened

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KINDS = ["fp32", "bf16", "fp16", "int8"]
INT64_MIN, INT64_MAX = -2 ** 63, 2 ** 63 - 1
BIG = 2 ** 33 + 5


def _bits(x):
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def _same(got, want, what=""):
    """got: the GPU's tuple (scores, idx[, pos]); want: ref_diffusion's three arrays (or torch tensors)."""
    want = [torch.as_tensor(w).cpu() for w in want]
    names = ("score bits", "ids", "positions")
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.int64 and (len(got) < 3 or got[2].dtype == torch.int32)
    for n, g in enumerate(got):
        assert torch.equal(_bits(g.cpu()), _bits(want[n])), f"{names[n]} differ {what}"


@pytest.fixture(scope="module")
def gallery():
    """2 000 unit rows per width, 500 groups of 4 look-alikes (every row has close neighbours and far ones), on the host; per storage kind
    the segment as ops.rerank_diffusion takes it (on the GPU, offset left out) and the fp32 values it stands for. Never modified."""
    from cor_amd import ops
    out = {}
    for C in (16, 64, 256):
        g = torch.Generator().manual_seed(70 + C)
        centres = torch.nn.functional.normalize(torch.randn((500, C), generator=g), dim=-1)
        G = torch.nn.functional.normalize(centres.repeat_interleave(4, 0) + 0.3 * torch.randn((2000, C), generator=g) / C ** 0.5, dim=-1)
        G = G[torch.randperm(2000, generator=g)].contiguous()
        q8, s8 = ops.quantize_rows_i8(G.to(DEV))
        stored = {"fp32": (G.to(DEV),), "bf16": (G.to(DEV, torch.bfloat16),), "fp16": (G.to(DEV, torch.float16),), "int8": (q8, s8)}
        values = {kind: widened([tuple(t.cpu() for t in seg) + (0,)])[0][0] for kind, seg in stored.items()}
        out[C] = (G, stored, values)
    return out


KINS = [1, 2, 3, 31, 32, 33, 63, 64, 65, 128, 255, 256]          # around the wave, the 32-row tile and the block sizes 64 / 128 / 256


def _draws():
    """Every kin of KINS four times (48 draws) with seeded (C, kd, kq, gamma, iters, alpha, k, kind, offset); the coverage of every value
    the issue lists is asserted below, so a change of the seed cannot silently lose one. Bq = 3."""
    rng = np.random.default_rng(2025)
    cases = []
    for n in range(4 * len(KINS)):
        kin = KINS[n % len(KINS)]
        C = [16, 64, 256][int(rng.integers(0, 3))]
        kd = [1, 2, 8, 32, "all"][n % 5]
        kd = min(max(kin - 1, 1), 32) if kd == "all" else kd               # kd >= n - 1 wherever n <= 33
        kq = [1, max(1, kin // 2), kin + 3][int(rng.integers(0, 3))]
        gamma = 1 + (n // 2) % 4
        iters = [1, 2, 20, 64][int(rng.integers(0, 4))]
        alpha = [0.0, 0.5, 0.9, 0.99][(n // 3) % 4]
        k = [max(1, kin // 3), kin, min(kin + 7, 256)][int(rng.integers(0, 3))]
        kind = KINDS[n % 4] if n % 8 < 4 else str(rng.choice(KINDS))
        off = [0, BIG][int(rng.integers(0, 2))]
        cases.append((kin, C, kd, kq, gamma, iters, alpha, k, kind, off))
    cover = lambda col: {c[col] for c in cases}
    assert cover(1) == {16, 64, 256} and {1, 2, 8, 32} <= cover(2) and cover(4) == {1, 2, 3, 4} and cover(5) == {1, 2, 20, 64}
    assert cover(6) == {0.0, 0.5, 0.9, 0.99} and cover(8) == set(KINDS)
    assert any(c[3] == 1 for c in cases) and any(1 < c[3] < c[0] for c in cases) and any(c[3] > c[0] for c in cases)
    assert any(c[7] < c[0] for c in cases) and any(c[7] == c[0] for c in cases) and any(c[7] > c[0] for c in cases)
    assert any(c[2] >= c[0] - 1 and c[0] > 3 for c in cases)
    return cases


@pytest.mark.parametrize("kin,C,kd,kq,gamma,iters,alpha,k,kind,off", _draws())
def test_drawn_combinations(gallery, kin, C, kd, kq, gamma, iters, alpha, k, kind, off):
    """Random candidate lists (not search results): ids a little outside the segment (missing entries anywhere in the list), repeats by
    chance, scores of both signs. k > the number of present entries checks the tail."""
    from cor_amd import ops
    _, stored, values = gallery[C]
    Bq = 3
    g = torch.Generator().manual_seed(kin * 1000 + k + kd)
    idx = torch.randint(-40, 2040, (Bq, kin), generator=g) + off
    sc = torch.rand((Bq, kin), generator=g) * 2 - 0.5
    want = ref_diffusion(sc.numpy(), idx.numpy(), [(values[kind], off)], k, kd=kd, kq=kq, gamma=gamma, alpha=alpha, iters=iters)
    got = ops.rerank_diffusion([stored[kind] + (off,)], sc.to(DEV), idx.to(DEV), k, kd=kd, kq=kq, gamma=gamma, alpha=alpha, iters=iters, return_pos=True)
    _same(got, want)
    assert (want[1][:, 0] >= 0).any() or kin < 32                      # (the draw is not vacuous: something is present)


MIXED = (("fp32", 0, 500), ("int8", 500, 1000), ("bf16", 1000, 1500), ("fp16", 1500, 2000))


@pytest.mark.parametrize("Bq,kin,C,kd,gamma,alpha,iters,k,off", [
    (5, 1, 16, 1, 1, 0.5, 1, 1, 0), (5, 33, 64, 8, 3, 0.9, 20, 40, BIG), (3, 65, 256, 2, 2, 0.99, 64, 65, 0), (3, 128, 16, 32, 4, 0.5, 2, 100, BIG),
    (2, 255, 64, 8, 3, 0.9, 20, 256, 0), (2, 256, 256, 8, 3, 0.9, 20, 256, BIG)])
def test_a_mixed_table(gallery, Bq, kin, C, kd, gamma, alpha, iters, k, off):
    """A table of four segments, one per storage kind: the kernel that reads the dtype per candidate, at every block size."""
    from cor_amd import ops
    _, stored, values = gallery[C]
    g = torch.Generator().manual_seed(kin * 1000 + k + Bq + 1)
    idx = torch.randint(-40, 2040, (Bq, kin), generator=g) + off
    sc = torch.rand((Bq, kin), generator=g) * 2 - 0.5
    table = [tuple(t[lo:hi] for t in stored[kind]) + (off + lo,) for kind, lo, hi in MIXED]
    vals = np.concatenate([values[kind][lo:hi] for kind, lo, hi in MIXED])
    want = ref_diffusion(sc.numpy(), idx.numpy(), [(vals, off)], k, kd=kd, gamma=gamma, alpha=alpha, iters=iters)
    _same(ops.rerank_diffusion(table, sc.to(DEV), idx.to(DEV), k, kd=kd, gamma=gamma, alpha=alpha, iters=iters, return_pos=True), want)


def test_equal_values_in_four_dtypes_and_any_segmentation():
    """Values k / 64 (|k| <= 64) are exact in fp32, bf16, fp16 and as int8 q = k with scale 1 / 64: the four tables give the same bits. The
    same rows as one segment, cut into 3 and into 16 segments (given out of order, one of them empty), give the same bits again."""
    from cor_amd import ops
    g = torch.Generator().manual_seed(5)
    q = torch.randint(-64, 65, (400, 64), generator=g)
    q[200:300] = q[:100]                                               # twins
    vals = (q.float() / 64).contiguous()
    off = BIG
    idx = (torch.randint(-10, 410, (4, 100), generator=g) + off)
    sc = torch.rand((4, 100), generator=g)
    want = ref_diffusion(sc.numpy(), idx.numpy(), [(vals.numpy(), off)], 100, kd=8, gamma=3, alpha=0.9, iters=20)
    tables = {"fp32": (vals.to(DEV),), "bf16": (vals.to(DEV, torch.bfloat16),), "fp16": (vals.to(DEV, torch.float16),),
              "int8": (q.to(DEV, torch.int8), torch.full((400,), 1 / 64, device=DEV))}
    run = lambda table: ops.rerank_diffusion(table, sc.to(DEV), idx.to(DEV), 100, kd=8, gamma=3, alpha=0.9, iters=20, return_pos=True)
    for kind, seg in tables.items():
        _same(run([seg + (off,)]), want, kind)
    for kind in ("fp32", "int8"):
        for cuts in ([0, 130, 130, 400], [0] + sorted(torch.randperm(399, generator=g)[:14].add(1).tolist()) + [400, 400]):
            parts = [tuple(t[lo:hi] for t in tables[kind]) + (off + lo,) for lo, hi in zip(cuts, cuts[1:])]
            assert any(p[0].shape[0] == 0 for p in parts) and len(parts) in (3, 16)
            _same(run(parts[::-1]), want, f"{kind} in {len(parts)} segments")
    kinds = ["fp32", "bf16", "fp16", "int8"]
    cuts = [0, 100, 200, 300, 400]
    _same(run([tuple(t[lo:hi] for t in tables[kinds[n]]) + (off + lo,) for n, (lo, hi) in enumerate(zip(cuts, cuts[1:]))]), want, "one kind per segment")


@pytest.mark.parametrize("kind", KINDS)
def test_lists_straight_from_search(gallery, kind):
    """alpha = 0 with gamma = 1 returns a searched list with positive scores bitwise; the same lists against the restatement."""
    G, stored, values = gallery[256]
    shard = _shard(stored, kind, 1000)
    q = torch.nn.functional.normalize(G[:12] + G[100:112] + 0.5 * G[200:212], dim=-1).to(DEV)
    for kin in (10, 100, 256):
        s, i = shard.search(q, kin)
        assert (s > 0).all()
        pos = torch.arange(kin, dtype=torch.int32).expand(12, kin)
        _same(shard.diffuse(s, i, kin, gamma=1, alpha=0.0, return_pos=True), (s.cpu(), i.cpu(), pos), f"kin={kin}")
        assert shard.diffuse(s, i)[1].shape == (12, kin)               # k defaults to min(kin, 256)
    s, i = s[:4], i[:4]
    for kw in (dict(), dict(kd=4, kq=10, gamma=2, alpha=0.5, iters=5)):
        want = ref_diffusion(s.cpu().numpy(), i.cpu().numpy(), [(values[kind], 1000)], 50, **kw)
        _same(shard.diffuse(s, i, 50, return_pos=True, **kw), want, str(kw))


def _shard(stored, kind, offset, lo=0, hi=None, plain=False):
    from cor_amd.retrieval import GalleryShard, QuantizedGallery, QuantizedShard
    if kind == "int8":
        return (QuantizedShard if plain else QuantizedGallery)(stored[kind][0][lo:hi], stored[kind][1][lo:hi], offset=offset + lo)
    return GalleryShard(stored[kind][0][lo:hi], offset=offset + lo)


def test_hostile_lists(gallery):
    """-1, INT64_MIN / MAX, another shard's ids, 64-bit garbage at the head, in the middle and at the tail of a list, NaN scores on the missing
    entries; a list with no present entry; no segment at all; no queries; out_pos left out."""
    from cor_amd import ops
    _, stored, values = gallery[64]
    off, Bq, kin = 5000, 6, 70
    g = torch.Generator().manual_seed(9)
    idx = torch.randint(0, 2000, (Bq, kin), generator=g) + off
    sc = torch.rand((Bq, kin), generator=g)
    hostile = torch.tensor([-1, INT64_MIN, INT64_MAX, off - 1, off + 2000, 17, off + 2 ** 32, -off, INT64_MIN + off, INT64_MAX - 3])
    where = torch.rand((Bq, kin), generator=g) < 0.3
    where[0, :9] = True                                                # the head
    where[1, 30:41] = True                                             # the middle
    idx = torch.where(where, hostile[torch.randint(0, len(hostile), (Bq, kin), generator=g)], idx)
    idx[:, 50:] = -1                                                   # a search's tail
    idx[5] = hostile[torch.arange(kin) % len(hostile)]                 # a query with nothing present
    sc = torch.where(where | (idx == -1), torch.full_like(sc, float("nan")), sc)
    sc[5] = float("nan")
    seg = stored["fp32"] + (off,)
    for kw, k in ((dict(), 70), (dict(kd=32, gamma=1, alpha=0.5, iters=2), 256), (dict(kd=1, kq=3, gamma=4, alpha=0.99, iters=64), 5)):
        want = ref_diffusion(sc.numpy(), idx.numpy(), [(values["fp32"], off)], k, **kw)
        assert (want[1][5] == -1).all() and not np.isnan(want[0]).any()
        _same(ops.rerank_diffusion([seg], sc.to(DEV), idx.to(DEV), k, return_pos=True, **kw), want, str(kw))
        _same(ops.rerank_diffusion([seg], sc.to(DEV), idx.to(DEV), k, **kw), want[:2], f"{kw} without positions")
    tail = ref_diffusion(sc.numpy(), idx.numpy(), [], 7)
    assert (tail[1] == -1).all() and (tail[2] == -1).all()
    _same(ops.rerank_diffusion([], sc.to(DEV), idx.to(DEV), 7, return_pos=True), tail, "nseg == 0")
    empty = (stored["fp32"][0][:0], off)
    _same(ops.rerank_diffusion([empty], sc.to(DEV), idx.to(DEV), 7, return_pos=True), tail, "an empty segment")
    s0, i0, p0 = ops.rerank_diffusion([seg], sc[:0].to(DEV), idx[:0].to(DEV), 3, return_pos=True)
    assert s0.shape == (0, 3) and i0.shape == (0, 3) and p0.shape == (0, 3)    # no queries


def test_ties_isolated_rows_and_edge_scores(gallery):
    from cor_amd import ops
    G, _, _ = gallery[64]
    rows = G[:300].clone()
    rows[100:200] = rows[:100]                                         # duplicated gallery rows: ids g and g + 100 hold the same values
    rows[200:205] = rows[0]                                            # a block of six identical rows (0, 100, 200 .. 204)
    e = torch.eye(64)
    rows[250:258] = e[:8]                                              # orthogonal rows
    rows[258:262] = -e[:4]                                             # and opposite ones: no positive similarity to any other of these
    seg, vals, off = (rows.to(DEV), 70), rows.numpy(), 70
    g = torch.Generator().manual_seed(3)

    def check(sc, idx, k, what, **kw):
        want = ref_diffusion(sc.numpy(), idx.numpy(), [(vals, off)], k, **kw)
        _same(ops.rerank_diffusion([seg], sc.to(DEV), idx.to(DEV), k, return_pos=True, **kw), want, what)
        return want

    # identical rows tie in the neighbour selection (decided by position): twins and the block of six, in a random order
    base = torch.stack([torch.randperm(100, generator=g)[:37] for _ in range(4)])
    idx = torch.cat([base + 100, base, torch.arange(200, 205).expand(4, 5), torch.zeros((4, 1), dtype=torch.int64)], 1) + off
    idx = torch.gather(idx, 1, torch.stack([torch.randperm(80, generator=g) for _ in range(4)]))
    sc = (((idx - off) % 100).float() / 128 + 0.125)                   # a twin has its twin's score
    for kw in (dict(), dict(kd=1, gamma=1, alpha=0.5, iters=1), dict(kd=3, gamma=2, alpha=0.99, iters=64), dict(kd=32, kq=7, alpha=0.5, iters=2)):
        check(sc, idx, 80, f"twins {kw}", **kw)
    # equal f ties in the final rank (decided by the id, then the position): alpha = 0 and equal scores, repeated ids among them
    rep = torch.tensor([[5, 9, 5, 250, 9, 5, 3, 104]]) + off
    want = check(torch.full((1, 8), 0.5), rep, 8, "equal f", kd=2, gamma=2, alpha=0.0, iters=3)
    assert want[1][0].tolist() == [73, 75, 75, 75, 79, 79, 174, 320] and want[2][0].tolist() == [6, 0, 2, 5, 1, 4, 7, 3]
    check(torch.tensor([[0.9, 0.8, 0.9, 0.7, 0.8, 0.2, 0.6, 0.5]]), rep, 8, "repeated ids", kd=2, gamma=1, alpha=0.9, iters=20)
    # isolated nodes: d = 0, f = (alpha * 0) + (1 - alpha) y; mixed with rows that do have neighbours
    iso = (torch.tensor([[250, 258, 251, 259, 252, 253, 260, 0, 100, 1]]) + off)
    check(torch.tensor([[0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3, 0.2, 0.1, 0.05]]), iso, 10, "isolated rows among others", kd=4, gamma=1, alpha=0.9, iters=20)
    isc = torch.rand((3, 12), generator=g)
    want = check(isc, (torch.arange(250, 262).expand(3, 12) + off).contiguous(), 12, "only isolated rows", kd=8, gamma=2, alpha=0.5, iters=3)
    y = isc.numpy() * isc.numpy()
    alone = (np.float32(0.5) * np.float32(0)) + ((np.float32(1) - np.float32(0.5)) * y)
    assert np.array_equal(np.take_along_axis(alone, want[2].astype(np.int64), 1), want[0])
    # non-positive and -0.0 scores inject nothing; all scores non-positive: every f is +0 and the ids decide
    z = torch.tensor([[0.5, -0.0, 0.0, -0.3, 0.25, -0.0, 0.0, 0.125]])
    zi = torch.tensor([[7, 6, 5, 4, 3, 2, 1, 0]]) + off
    for kw in (dict(gamma=1, alpha=0.5, iters=2), dict(gamma=3, alpha=0.0, iters=1), dict(kd=32, gamma=2, alpha=0.99, iters=64)):
        check(z, zi, 8, f"signed zeros {kw}", **kw)
    want = check(-z.abs(), zi, 8, "no positive score", kd=8, gamma=3, alpha=0.9, iters=20)
    assert want[1][0].tolist() == sorted(zi[0].tolist()) and (want[0] == 0).all() and not np.signbit(want[0]).any()


@pytest.mark.parametrize("Bq", [1, 2, 257, 513])
def test_many_queries(gallery, Bq):
    """More blocks than CUs, odd counts; short lists keep the CPU restatement at about a second."""
    from cor_amd import ops
    _, stored, values = gallery[16]
    g = torch.Generator().manual_seed(Bq)
    idx = torch.randint(-5, 2005, (Bq, 20), generator=g)
    sc = torch.rand((Bq, 20), generator=g) * 2 - 0.5
    want = ref_diffusion(sc.numpy(), idx.numpy(), [(values["bf16"], 0)], 12, kd=4, gamma=2, alpha=0.9, iters=5)
    _same(ops.rerank_diffusion([stored["bf16"] + (0,)], sc.to(DEV), idx.to(DEV), 12, kd=4, gamma=2, alpha=0.9, iters=5, return_pos=True), want)


def test_segmentation_and_storage_through_the_gallery_classes(gallery):
    """diffuse of a GalleryShard, a QuantizedGallery and a GallerySet (segments out of order, a gap, an empty one, a plain QuantizedShard)
    against ops.rerank_diffusion over the same table, and the set against one fp32 shard over the concatenated values."""
    from cor_amd import ops
    from cor_amd.retrieval import GallerySet, GalleryShard
    G, stored, values = gallery[256]
    off = BIG
    g = torch.Generator().manual_seed(21)
    q = torch.nn.functional.normalize(G[500:510] + G[900:910], dim=-1).to(DEV)
    kw = dict(kd=6, kq=40, gamma=2, alpha=0.8, iters=10)
    for kinds in (("fp32", "fp32", "fp32"), ("int8", "int8", "int8"), ("fp32", "bf16", "int8"), ("int8", "fp16", "bf16")):
        segs = [_shard(stored, kinds[2], off, 1300, 2000, plain=True), _shard(stored, kinds[0], off, 0, 700),
                _shard(stored, kinds[1], off - 50, 0, 0), _shard(stored, kinds[1], off, 800, 1300)]
        parts = GallerySet(segs)
        vals = np.concatenate([values[kinds[0]][:700], np.zeros((100, 256), np.float32), values[kinds[1]][800:1300], values[kinds[2]][1300:]])
        one = GalleryShard(torch.from_numpy(vals).to(DEV), offset=off)
        idx = torch.randint(-30, 2030, (10, 120), generator=g) + off
        sc = torch.rand((10, 120), generator=g)
        gap = (idx >= off + 700) & (idx < off + 800)
        idx = torch.where(gap, torch.full_like(idx, -1), idx).to(DEV)  # (the single shard holds zero rows there: keep them out of the lists)
        sc = sc.to(DEV)
        table = [(sh.rows, sh.scales, sh.offset) if hasattr(sh, "scales") else (sh.rows, sh.offset) for sh in segs if len(sh)]
        got = parts.diffuse(sc, idx, 50, return_pos=True, **kw)
        _same(got, ops.rerank_diffusion(table, sc, idx, 50, return_pos=True, **kw), f"{kinds} set against ops")
        _same(got, one.diffuse(sc, idx, 50, return_pos=True, **kw), f"{kinds} set against one shard")
        _same(segs[1].diffuse(sc, idx, 50, return_pos=True, **kw), ops.rerank_diffusion(table[1:2], sc, idx, 50, return_pos=True, **kw),
              f"{kinds[0]} shard against ops")
        s, i = parts.search(q, 100)                                    # the set's own lists
        _same(parts.diffuse(s, i, 20), one.diffuse(s, i, 20), f"{kinds} searched lists")
    want = ref_diffusion(sc.cpu().numpy(), idx.cpu().numpy(), [(vals, off)], 50, **kw)
    _same(got, want, "the last set against the restatement")
    qg = _shard(stored, "int8", 1000)
    s, i = qg.search(q, 128)
    _same(qg.diffuse(s, i, 30, return_pos=True), ops.rerank_diffusion([(qg.rows, qg.scales, 1000)], s, i, 30, return_pos=True), "quantized gallery against ops")
    _same(qg.diffuse(s, i, 30, return_pos=True), qg.dequantized().diffuse(s, i, 30, return_pos=True), "quantized gallery against its fp32 rows")


def test_diffused_search_is_the_composition(gallery):
    from cor_amd import retrieval
    from cor_amd.retrieval import GallerySet, GalleryShard, QuantizedGallery
    G, stored, _ = gallery[256]
    lab = (torch.arange(2000) % 7).to(torch.int32)
    grp = (torch.arange(2000) // 3).to(torch.int32)
    q = torch.nn.functional.normalize(G[40:56] + G[1040:1056], dim=-1).to(DEV)
    ql = (torch.arange(16) % 7).to(torch.int32)
    f32 = GalleryShard(stored["fp32"][0], offset=300, labels=lab, groups=grp)
    i8 = QuantizedGallery(*stored["int8"], offset=300, labels=lab, groups=grp)
    both = GallerySet([GalleryShard(stored["bf16"][0][:900], offset=300, labels=lab[:900], groups=grp[:900]),
                       QuantizedGallery(stored["int8"][0][900:], stored["int8"][1][900:], offset=1200, labels=lab[900:], groups=grp[900:])])
    for gal in (f32, i8, both):
        for kw in (dict(), dict(query_labels=ql, mode="ne"), dict(distinct=True)):
            s, i = gal.search(q, 100, **kw)
            _same(retrieval.diffused_search(q, gal, 10, 100, kd=6, kq=50, gamma=2, alpha=0.8, iters=10, **kw),
                  gal.diffuse(s, i, k=10, kd=6, kq=50, gamma=2, alpha=0.8, iters=10), str(kw))


def test_side_stream_and_captured_graph(gallery):
    """A side stream, and a capture on a single stream that is replayed three times, each time with new lists."""
    G, stored, _ = gallery[64]
    shard = _shard(stored, "bf16", 0)
    q = torch.nn.functional.normalize(G[:48] + G[300:348], dim=-1).to(DEV)
    lists = [shard.search(q[16 * n:16 * n + 16], 100) for n in range(3)]
    run = lambda s, i: shard.diffuse(s, i, 20, return_pos=True)
    wants = [run(s, i) for s, i in lists]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = run(*lists[0])
    side.synchronize()
    _same(got, [w.cpu() for w in wants[0]], "side stream")
    sin, iin = lists[0][0].clone(), lists[0][1].clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                      # one capture stream
        out = run(sin, iin)
    for n in (1, 2, 0):                                                # replayed three times with new lists
        sin.copy_(lists[n][0])
        iin.copy_(lists[n][1])
        graph.replay()
        torch.cuda.synchronize()
        _same(out, [w.cpu() for w in wants[n]], f"replay with lists {n}")
    assert not torch.equal(wants[0][1], wants[1][1])

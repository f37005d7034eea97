"""GPU tests of the result diversification (cor_diversify_mmr, ops.diversify_mmr, GalleryShard / QuantizedGallery / GallerySet .diversify,
retrieval.diversified_search). Every comparison is bitwise, on score bits, ids, positions and values. The reference is the CPU restatement
of the definition, tests/diversify_refs.py, over the row values the kernel sums (16-bit rows widened, int8 rows float(q) * scale)."""
import numpy as np
import pytest
import torch

from tests.diversify_refs import ref_diversify
from tests.i8_list_refs import widened

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KINDS = ["fp32", "bf16", "fp16", "int8"]
INT64_MIN, INT64_MAX = -2 ** 63, 2 ** 63 - 1
BIG = 2 ** 33 + 5


def _bits(x):
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def _same(got, want, what=""):
    """got: the GPU's tuple (scores, idx[, pos][, value]); want: ref_diversify's four arrays (or torch tensors)."""
    want = [torch.as_tensor(w).cpu() for w in want]
    names = ("score bits", "ids", "positions", "values")
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.int64
    for n, g in enumerate(got):
        assert torch.equal(_bits(g.cpu()), _bits(want[n])), f"{names[n]} differ {what}"


@pytest.fixture(scope="module")
def gallery():
    """2 000 unit rows per width, 500 groups of 4 look-alikes (so that max_sim = 0.5 / 0.9 both bite), on the host; per storage kind
    the segment as ops.diversify_mmr takes it (on the GPU, offset left out) and the fp32 values it stands for. Never modified."""
    from cor_amd import ops
    out = {}
    for C in (16, 64, 128, 256):
        g = torch.Generator().manual_seed(40 + C)
        centres = torch.nn.functional.normalize(torch.randn((500, C), generator=g), dim=-1)
        G = torch.nn.functional.normalize(centres.repeat_interleave(4, 0) + 0.3 * torch.randn((2000, C), generator=g) / C ** 0.5, dim=-1)
        G = G[torch.randperm(2000, generator=g)].contiguous()
        q8, s8 = ops.quantize_rows_i8(G.to(DEV))
        stored = {"fp32": (G.to(DEV),), "bf16": (G.to(DEV, torch.bfloat16),), "fp16": (G.to(DEV, torch.float16),), "int8": (q8, s8)}
        values = {kind: widened([tuple(t.cpu() for t in seg) + (0,)])[0][0] for kind, seg in stored.items()}
        out[C] = (G, stored, values)
    return out


def _draws():
    """40 seeded draws of (Bq, kin, k, C, kind, lam, max_sim, offset), then the sizes at which the launch changes. Bq <= 5 when
    kin >= 1024, and Bq = 130 is cut to 5 (or 1) where the CPU restatement would cost more than 6e8 chain steps, a step of its Python
    loop counted as 300 (a test takes a few seconds); one draw is the largest shape, kin = 4096 with k = 256 at Bq = 1."""
    rng = np.random.default_rng(2024)
    cases = [(1, 4096, 256, 64, "bf16", 0.5, 0.9, BIG)]
    kins = [1, 2, 63, 64, 65, 255, 256, 257, 1000, 4096]
    while len(cases) < 40:
        n = len(cases)
        kin = kins[n % len(kins)]                                      # every kin four times
        Bq = int(rng.choice([1, 5, 130]))
        k = int(rng.choice([1, 2, 10, 100, 256]))
        C = int(rng.choice([16, 64, 256]))
        kind = KINDS[n % 4] if n % 8 < 4 else str(rng.choice(KINDS))
        lam = float(rng.choice([0, 0.3, 0.5, 1]))
        ms = [None, 0.5, 0.9][int(rng.integers(0, 3))]
        off = [0, BIG][int(rng.integers(0, 2))]
        if kin >= 1024:
            Bq = min(Bq, 5)
        if Bq * min(k, kin) * kin * (C + 300) > 6e8:
            Bq = 5 if 5 * min(k, kin) * kin * (C + 300) <= 6e8 else 1
        cases.append((Bq, kin, k, C, kind, lam, ms, off))
    # A block has one thread per candidate up to kin = 256 (64, 128, 256 threads: 64 / 65, 128 / 129 change the count), then 256 threads
    # with two (kin <= 512) or four candidates each, 512 threads from kin = 1025 and 1024 from 2049. A single-dtype table stages its rows
    # through LDS 128 bytes at a time: rows shorter than, as long as and longer than 128 bytes, for every storage kind
    for kin in (512, 513):
        cases += [(5, kin, 10, 16, "fp32", 0.5, 0.9, 0), (3, kin, 20, 256, "fp32", 0.3, None, BIG), (5, kin, 10, 64, "bf16", 0.5, None, BIG),
                  (5, kin, 10, 16, "fp16", 1.0, 0.5, 0), (3, kin, 20, 256, "fp16", 0.5, 0.9, 0), (5, kin, 10, 16, "int8", 0.5, 0.9, BIG),
                  (5, kin, 10, 128, "int8", 0.3, None, 0), (3, kin, 20, 256, "int8", 0.0, 0.5, 0)]
    for kin in (128, 129, 1024, 1025, 2048, 2049):
        cases += [(3, kin, 10, 64, "fp32", 0.5, 0.9, BIG), (3, kin, 10, 256, "bf16", 0.3, None, 0), (3, kin, 10, 128, "fp16", 0.5, 0.5, 0),
                  (3, kin, 10, 64, "int8", 1.0, 0.9, BIG)]
    return cases


@pytest.mark.parametrize("Bq,kin,k,C,kind,lam,max_sim,off", _draws())
def test_drawn_combinations(gallery, Bq, kin, k, C, kind, lam, max_sim, off):
    """Random candidate lists (not search results): ids a little outside the segment, repeats by chance (kin > 2 000: by necessity),
    scores of both signs. k > kin and k > the number of present entries check the tail."""
    from cor_amd import ops
    _, stored, values = gallery[C]
    g = torch.Generator().manual_seed(kin * 1000 + k + Bq)
    idx = torch.randint(-40, 2040, (Bq, kin), generator=g) + off
    sc = torch.rand((Bq, kin), generator=g) * 2 - 0.5
    want = ref_diversify(sc.numpy(), idx.numpy(), [(values[kind], off)], k, lam, max_sim)
    got = ops.diversify_mmr([stored[kind] + (off,)], sc.to(DEV), idx.to(DEV), k, lam=lam, max_sim=max_sim, return_pos=True, return_value=True)
    _same(got, want)
    assert (want[1][:, 0] >= 0).all() or kin < 64                      # (the draw is not vacuous: something is present)


MIXED = (("fp32", 0, 500), ("int8", 500, 1000), ("bf16", 1000, 1500), ("fp16", 1500, 2000))


@pytest.mark.parametrize("Bq,kin,k,C,lam,max_sim,off", [
    (5, 1, 1, 16, 0.5, None, 0), (130, 63, 10, 64, 0.3, 0.9, BIG), (5, 64, 100, 256, 0.5, 0.5, 0), (5, 65, 10, 128, 1.0, 0.9, 0),
    (5, 128, 256, 16, 0.0, None, BIG), (5, 129, 10, 64, 0.5, 0.9, 0), (5, 256, 100, 256, 0.3, None, BIG), (5, 257, 10, 64, 0.5, 0.5, 0),
    (3, 512, 20, 256, 0.5, 0.9, 0), (3, 513, 20, 16, 0.3, None, BIG), (3, 1000, 100, 64, 0.5, 0.9, 0), (3, 1025, 10, 128, 1.0, 0.5, 0),
    (3, 2049, 10, 64, 0.5, None, BIG), (1, 4096, 256, 256, 0.5, 0.9, BIG)])
def test_drawn_combinations_over_a_mixed_table(gallery, Bq, kin, k, C, lam, max_sim, off):
    """A table of four segments, one per storage kind: the kernel that reads the dtype per candidate and gathers rows straight from global
    memory, at every size at which its launch changes."""
    from cor_amd import ops
    _, stored, values = gallery[C]
    g = torch.Generator().manual_seed(kin * 1000 + k + Bq + 1)
    idx = torch.randint(-40, 2040, (Bq, kin), generator=g) + off
    sc = torch.rand((Bq, kin), generator=g) * 2 - 0.5
    table = [tuple(t[lo:hi] for t in stored[kind]) + (off + lo,) for kind, lo, hi in MIXED]
    vals = np.concatenate([values[kind][lo:hi] for kind, lo, hi in MIXED])
    want = ref_diversify(sc.numpy(), idx.numpy(), [(vals, off)], k, lam, max_sim)
    _same(ops.diversify_mmr(table, sc.to(DEV), idx.to(DEV), k, lam=lam, max_sim=max_sim, return_pos=True, return_value=True), want)


def _shard(stored, kind, offset, lo=0, hi=None, plain=False):
    from cor_amd.retrieval import GalleryShard, QuantizedGallery, QuantizedShard
    if kind == "int8":
        return (QuantizedShard if plain else QuantizedGallery)(stored[kind][0][lo:hi], stored[kind][1][lo:hi], offset=offset + lo)
    return GalleryShard(stored[kind][0][lo:hi], offset=offset + lo)


@pytest.mark.parametrize("kind", KINDS)
def test_lists_straight_from_search(gallery, kind):
    """lam = 1 without max_sim returns a searched list bitwise; the same list at lam = 0.5 and under suppression against the restatement."""
    G, stored, values = gallery[256]
    shard = _shard(stored, kind, 1000)
    q = torch.nn.functional.normalize(G[:24] + G[100:124] + 0.5 * G[200:224], dim=-1).to(DEV)
    for kin in (10, 100, 256):
        s, i = shard.search(q, kin)
        pos = torch.arange(kin, dtype=torch.int32).expand(24, kin)
        _same(shard.diversify(s, i, kin, lam=1.0, return_pos=True), (s.cpu(), i.cpu(), pos), f"kin={kin}")
        assert shard.diversify(s, i)[1].shape == (24, kin)             # k defaults to min(kin, 256)
    for lam, ms in ((0.5, None), (1.0, 0.9), (0.3, 0.5)):
        want = ref_diversify(s.cpu().numpy(), i.cpu().numpy(), [(values[kind], 1000)], 20, lam, ms)
        _same(shard.diversify(s, i, 20, lam=lam, max_sim=ms, return_pos=True), want, f"lam={lam} max_sim={ms}")


def test_hostile_lists(gallery):
    """-1 tails, INT64_MIN / MAX, another shard's ids, NaN scores on the missing entries; all entries missing; no segment at all."""
    from cor_amd import ops
    _, stored, values = gallery[64]
    off, Bq, kin = 5000, 6, 70
    g = torch.Generator().manual_seed(9)
    idx = torch.randint(0, 2000, (Bq, kin), generator=g) + off
    sc = torch.rand((Bq, kin), generator=g)
    hostile = torch.tensor([-1, INT64_MIN, INT64_MAX, off - 1, off + 2000, 17, off + 2 ** 32, -off, INT64_MIN + off, INT64_MAX - 3])
    where = torch.rand((Bq, kin), generator=g) < 0.4
    idx = torch.where(where, hostile[torch.randint(0, len(hostile), (Bq, kin), generator=g)], idx)
    idx[:, 50:] = -1                                                   # a search's tail
    idx[5] = hostile[torch.arange(kin) % len(hostile)]                 # a query with nothing present
    sc = torch.where(where | (idx == -1), torch.full_like(sc, float("nan")), sc)
    seg = stored["fp32"] + (off,)
    for lam, ms, k in ((0.5, None, 70), (1.0, 0.5, 256), (0.0, 0.9, 5)):
        want = ref_diversify(sc.numpy(), idx.numpy(), [(values["fp32"], off)], k, lam, ms)
        assert (want[1][5] == -1).all() and np.isneginf(want[3][5]).all() and not np.isnan(want[0]).any()
        _same(ops.diversify_mmr([seg], sc.to(DEV), idx.to(DEV), k, lam=lam, max_sim=ms, return_pos=True, return_value=True), want, f"lam={lam}")
    tail = ref_diversify(sc.numpy(), idx.numpy(), [], 7, 0.5, None)
    assert (tail[1] == -1).all() and (tail[2] == -1).all()
    _same(ops.diversify_mmr([], sc.to(DEV), idx.to(DEV), 7, return_pos=True, return_value=True), tail, "nseg == 0")
    empty = (stored["fp32"][0][:0], off)
    _same(ops.diversify_mmr([empty], sc.to(DEV), idx.to(DEV), 7, return_pos=True, return_value=True), tail, "an empty segment")
    s0, i0 = ops.diversify_mmr([seg], sc[:0].to(DEV), idx[:0].to(DEV), 3)
    assert s0.shape == (0, 3) and i0.shape == (0, 3)                   # no queries


def test_ties_and_edge_values(gallery):
    from cor_amd import ops
    from tests.diversify_refs import chain_pairs
    G, _, _ = gallery[64]
    rows = G[:300].clone()
    rows[100:200] = rows[:100]                                         # duplicated gallery rows: ids g and g + 100 hold the same values
    seg, vals, off = (rows.to(DEV), 70), rows.numpy(), 70
    g = torch.Generator().manual_seed(3)

    def check(sc, idx, k, lam, ms, what):
        want = ref_diversify(sc.numpy(), idx.numpy(), [(vals, off)], k, lam, ms)
        _same(ops.diversify_mmr([seg], sc.to(DEV), idx.to(DEV), k, lam=lam, max_sim=ms, return_pos=True, return_value=True), want, what)
        return want

    # equal f is decided by the id: twin rows with equal scores, listed in a random order
    base = torch.stack([torch.randperm(100, generator=g)[:40] for _ in range(8)])
    idx = torch.cat([base + 100, base], 1) + off
    idx = torch.gather(idx, 1, torch.stack([torch.randperm(80, generator=g) for _ in range(8)]))
    sc = (((idx - off) % 100).float() / 128 + 0.125)                   # a twin has its twin's score
    for lam, ms in ((1.0, None), (0.5, None), (0.5, 0.99), (0.0, None)):
        want = check(sc, idx, 80, lam, ms, f"twins lam={lam} max_sim={ms}")
    assert (want[1][:, 0] == idx.min(1).values.numpy()).all()          # lam = 0: step 0 is an all-tie won by the lowest id
    # a repeated id: the second copy is penalised by sim(r, r) and suppressed at max_sim <= that value
    rep = torch.tensor([[5, 9, 5, 250, 9, 5]]) + off
    rsc = torch.tensor([[0.9, 0.8, 0.9, 0.7, 0.8, 0.2]])
    self_sim = chain_pairs(vals, [5, 9], [5, 9])                       # sim(r, r) of the two repeated rows: 1 up to rounding
    want = check(rsc, rep, 6, 0.5, None, "a repeated id")
    assert sorted(want[2][0].tolist()) == [0, 1, 2, 3, 4, 5] and want[2][0, 0] == 0
    want = check(rsc, rep, 6, 0.5, float(self_sim.min()), "a repeated id, suppressed")
    assert sorted(p for p in want[2][0].tolist() if p >= 0) == [0, 1, 3]
    above = float(np.nextafter(self_sim.max(), np.float32(2)))
    want = check(rsc, rep, 6, 0.5, above, "a repeated id, max_sim just above sim(r, r)")
    assert sorted(want[2][0].tolist()) == [0, 1, 2, 3, 4, 5]
    # +-0.0 scores tie; the output keeps the input's bits
    z = torch.tensor([[0.0, -0.0, 0.0, -0.0, -0.0, 0.0]])
    zi = torch.tensor([[250, 240, 230, 220, 210, 201]]) + off
    for lam in (0.5, 0.0, 1.0):
        want = check(z, zi, 6, lam, None, f"signed zeros lam={lam}")
    assert want[1][0].tolist() == sorted(zi[0].tolist()) and np.signbit(want[0][0]).tolist() == [False, True, True, False, True, False]
    # max_sim = -inf: exactly one output
    want = check(sc, idx, 5, 0.5, float("-inf"), "max_sim = -inf")
    assert (want[1][:, 0] >= 0).all() and (want[1][:, 1:] == -1).all()


def test_segmentation_and_storage(gallery):
    """A GallerySet of three segments given out of order, with a gap and an empty segment; mixed fp32 / bf16 / int8 segments against one
    fp32 GalleryShard over the concatenated widened / dequantised rows; QuantizedGallery.diversify against dequantized().diversify."""
    from cor_amd.retrieval import GallerySet, GalleryShard
    G, stored, values = gallery[256]
    off = BIG
    g = torch.Generator().manual_seed(21)
    q = torch.nn.functional.normalize(G[500:530] + G[900:930], dim=-1).to(DEV)
    # rows 700 .. 799 are left out (a gap); ids there are missing for both sides
    for kinds in (("fp32", "fp32", "fp32"), ("bf16", "bf16", "bf16"), ("int8", "int8", "int8"), ("fp32", "bf16", "int8"), ("int8", "fp16", "bf16")):
        parts = GallerySet([_shard(stored, kinds[2], off, 1300, 2000, plain=True), _shard(stored, kinds[0], off, 0, 700),
                            _shard(stored, kinds[1], off - 50, 0, 0), _shard(stored, kinds[1], off, 800, 1300)])
        vals = np.concatenate([values[kinds[0]][:700], np.zeros((100, 256), np.float32), values[kinds[1]][800:1300], values[kinds[2]][1300:]])
        one = GalleryShard(torch.from_numpy(vals).to(DEV), offset=off)
        idx = torch.randint(-30, 2030, (30, 200), generator=g) + off
        sc = torch.rand((30, 200), generator=g)
        gap = (idx >= off + 700) & (idx < off + 800)
        idx = torch.where(gap, torch.full_like(idx, -1), idx).to(DEV)  # (the single shard holds zero rows there: keep them out of the lists)
        sc = sc.to(DEV)
        for lam, ms in ((0.5, None), (0.3, 0.9), (1.0, 0.5)):
            _same(parts.diversify(sc, idx, 50, lam=lam, max_sim=ms, return_pos=True), one.diversify(sc, idx, 50, lam=lam, max_sim=ms, return_pos=True),
                  f"{kinds} lam={lam} max_sim={ms}")
        want = ref_diversify(sc.cpu().numpy(), idx.cpu().numpy(), [(vals, off)], 50, 0.5, 0.9)
        _same(parts.diversify(sc, idx, 50, lam=0.5, max_sim=0.9, return_pos=True), want[:3], f"{kinds} against the restatement")
        s, i = parts.search(q, 100)                                    # the set's own lists
        _same(parts.diversify(s, i, 20), one.diversify(s, i, 20), f"{kinds} searched lists")
    qg = _shard(stored, "int8", 1000)
    s, i = qg.search(q, 128)
    for lam, ms in ((0.5, None), (1.0, 0.9)):
        _same(qg.diversify(s, i, 30, lam=lam, max_sim=ms, return_pos=True), qg.dequantized().diversify(s, i, 30, lam=lam, max_sim=ms, return_pos=True))


def test_diversified_search_is_the_composition(gallery):
    from cor_amd import retrieval
    from cor_amd.retrieval import GallerySet, GalleryShard, QuantizedGallery
    G, stored, _ = gallery[256]
    lab = (torch.arange(2000) % 7).to(torch.int32)
    grp = (torch.arange(2000) // 3).to(torch.int32)
    q = torch.nn.functional.normalize(G[40:72] + G[1040:1072], dim=-1).to(DEV)
    ql = (torch.arange(32) % 7).to(torch.int32)
    f32 = GalleryShard(stored["fp32"][0], offset=300, labels=lab, groups=grp)
    i8 = QuantizedGallery(*stored["int8"], offset=300, labels=lab, groups=grp)
    both = GallerySet([GalleryShard(stored["bf16"][0][:900], offset=300, labels=lab[:900], groups=grp[:900]),
                       QuantizedGallery(stored["int8"][0][900:], stored["int8"][1][900:], offset=1200, labels=lab[900:], groups=grp[900:])])
    for gal in (f32, i8, both):
        for kw in (dict(), dict(query_labels=ql, mode="ne"), dict(distinct=True)):
            s, i = gal.search(q, 100, **kw)
            _same(retrieval.diversified_search(q, gal, 10, 100, lam=0.4, max_sim=0.8, **kw), gal.diversify(s, i, k=10, lam=0.4, max_sim=0.8), str(kw))


def test_side_stream_and_captured_graph(gallery):
    """A side stream, and a capture on a single stream that is replayed twice with the same bits and once more with new lists."""
    G, stored, _ = gallery[64]
    shard = _shard(stored, "bf16", 0)
    q = torch.nn.functional.normalize(G[:64] + G[300:364], dim=-1).to(DEV)
    sa, ia = shard.search(q[:32], 100)
    sb, ib = shard.search(q[32:], 100)
    run = lambda s, i: shard.diversify(s, i, 20, lam=0.5, max_sim=0.9, return_pos=True)
    want_a, want_b = run(sa, ia), run(sb, ib)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = run(sa, ia)
    side.synchronize()
    _same(got, [w.cpu() for w in want_a], "side stream")
    sin, iin = sa.clone(), ia.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                      # one capture stream
        out = run(sin, iin)
    for n in (1, 2):                                                   # replayed twice: the same bits
        graph.replay()
        torch.cuda.synchronize()
        _same(out, [w.cpu() for w in want_a], f"replay {n}")
    sin.copy_(sb)
    iin.copy_(ib)
    graph.replay()
    torch.cuda.synchronize()
    _same(out, [w.cpu() for w in want_b], "replay with new lists")

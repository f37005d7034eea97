"""GPU tests of the distinct-group int8 gallery search (cor_similarity_topk_i8_distinct, ops.similarity_topk_i8_distinct, QuantizedShard
with groups, GalleryShard.quantized, load_gallery_shard, GallerySet, two_stage_search, distributed_search). Every comparison is bitwise, on
score bits (.view(int32)) and indices, against tests/i8_distinct_refs.py, the CPU restatement of the definition in include/cor_amd.h,
with no excused position."""
import numpy as np
import pytest
import torch

from tests import i8_distinct_refs as DR
from tests import i8_filtered_refs as FR
from tests import i8_refs as R
from tests.test_gpu_topk_i8 import _gallery, _np, _same            # the seeded galleries are computed once for the three files

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F = np.float32
BIG = 2 ** 33 + 5


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _search(Q, gq, gs, k, groups, rl=None, ql=None, mode="eq", offset=0, flags=0):
    from cor_amd import ops
    return ops.similarity_topk_i8_distinct(_dev(Q), _dev(gq), _dev(gs), k, _dev(groups), None if rl is None else _dev(rl),
                                           None if ql is None else _dev(ql), mode=mode, g_offset=offset, flags=flags)


def _eq(a, b):
    return torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------ group layouts

def _groups(layout, Ng, seed):
    """group ids int32[Ng], the layouts of test_gpu_topk_distinct"""
    rng = np.random.default_rng(seed)
    runs = np.repeat(np.arange(Ng), rng.integers(1, 9, Ng))[:Ng]                   # image ids: runs of 1-8 consecutive rows
    if layout == "runs":
        g = runs
    elif layout == "perm":                                                         # the same ids, regions of one image far apart
        g = runs[rng.permutation(Ng)]
    elif layout == "dup_in":                                                       # every planted duplicate set inside ONE group
        g = runs.copy(); g[5] = g[3]
        if Ng > 300:
            g[Ng - 1] = g[17]; g[Ng - 200] = g[17]
    elif layout == "dup_across":                                                   # ... and spread over different groups
        g = runs + 10; g[3], g[5] = 0, 1
        if Ng > 300:
            g[17], g[Ng - 200], g[Ng - 1] = 2, 3, 4
    elif layout == "own":
        g = np.arange(Ng)
    elif layout == "negative":
        g = -1 - rng.integers(0, 5, Ng)                                            # all negative (values repeat): every row its own group
    else:
        raise KeyError(layout)
    return g.astype(np.int32)


_DUPS = {}


def _dup_gallery(Ng, C):
    """_gallery(Ng, C) with exact duplicates planted, int8 rows AND scales: rows 3 = 5, and for Ng > 300 rows 17 = Ng - 200 = Ng - 1"""
    if (Ng, C) not in _DUPS:
        G, gq, gs = _gallery(Ng, C)
        G, gq, gs = G.copy(), gq.copy(), gs.copy()
        pairs = [(3, 5)] + ([(17, Ng - 200), (17, Ng - 1)] if Ng > 300 else [])
        for a, b in pairs:
            G[b], gq[b], gs[b] = G[a], gq[a], gs[a]
        _DUPS[(Ng, C)] = (G, gq, gs)
    return _DUPS[(Ng, C)]


def _queries(G, Bq, seed):
    """query 0 is row 3 and query 1 row 17 (the planted duplicates lead their lists), the others noisy copies of gallery rows; src: the
    source rows"""
    rng = np.random.default_rng(seed)
    src = rng.integers(0, G.shape[0], Bq)
    Q = G[src] + F(0.3) * rng.standard_normal((Bq, G.shape[1])).astype(F)
    src[0], Q[0] = 3, G[3] * F(2.0)
    if Bq > 1 and G.shape[0] > 17:
        src[1], Q[1] = 17, G[17] * F(2.0)
    return Q, src


def _filter(kind, groups, src, Ng, seed):
    """(row labels, query labels, mode) of a filter kind; every 7th query is unrestricted"""
    if kind is None:
        return None, None, "eq"
    if kind == "ne":                                                               # the query's own image, on the group tensor itself
        rl = groups
    else:                                                                          # "eq" on 16 random classes
        rl = np.random.default_rng(seed).integers(0, 16, Ng).astype(np.int32)
    ql = rl[src].copy()
    ql[3::7] = -1
    return rl, ql.astype(np.int32), kind


# ------------------------------------------------------------------------------------------------------------------ shapes

BQS, NGS, CS, KS = (1, 7, 65, 257, 513), (15, 200, 4096, 4097, 40000, 70001), (16, 48, 64, 128, 256), (1, 10, 33, 100, 256)
LAYOUTS, FILTERS = ("runs", "perm", "dup_in", "dup_across"), (None, "ne", "eq")
# 42 of the 9000 combinations: round a = 0 .. 6 pairs row count b with Bq (4 a + b) % 5, C (b + 3 a) % 5, k (b + 2 a) % 5, layout (a + b) % 4
# and filter (2 a + b) % 3: seven rounds reach every residue, so every (Ng, Bq), (Ng, C), (Ng, k), (Ng, layout) and (Ng, filter) pair occurs
SHAPES = [(BQS[(4 * a + b) % 5], NGS[b], CS[(b + 3 * a) % 5], KS[(b + 2 * a) % 5], LAYOUTS[(a + b) % 4], FILTERS[(2 * a + b) % 3], a)
          for a in range(7) for b in range(6)]


def _offset(n):
    return BIG if n == 5 else (1000 if n % 2 else 0)


def test_shape_cases_cover_every_axis_value():
    assert len(SHAPES) == 42 and len(set(s[:6] for s in SHAPES)) == 42
    assert {(s[1], s[0]) for s in SHAPES} == {(Ng, Bq) for Ng in NGS for Bq in BQS}
    assert {(s[1], s[2]) for s in SHAPES} == {(Ng, C) for Ng in NGS for C in CS}
    assert {(s[1], s[3]) for s in SHAPES} == {(Ng, k) for Ng in NGS for k in KS}
    assert {(s[1], s[4]) for s in SHAPES} == {(Ng, m) for Ng in NGS for m in LAYOUTS}
    assert {(s[1], s[5]) for s in SHAPES} == {(Ng, f) for Ng in NGS for f in FILTERS}
    offs = [_offset(n) for n in range(len(SHAPES))]
    assert offs.count(1000) == 20 and offs.count(BIG) == 1 and offs.count(0) == 21
    assert any(s[1] >= 40000 and s[4] in ("runs", "perm") and s[5] == f for s in SHAPES for f in FILTERS)


@pytest.mark.parametrize("n", range(len(SHAPES)))
def test_search_is_bitwise_on_grouped_galleries(n):
    from cor_amd import _native
    Bq, Ng, C, k, layout, kind, a = SHAPES[n]
    G, gq, gs = _dup_gallery(Ng, C)
    groups = _groups(layout, Ng, Ng + a)
    Q, src = _queries(G, Bq, Bq + k + a)
    rl, ql, mode = _filter(kind, groups, src, Ng, Ng + 3 * a)
    off = _offset(n)
    want = DR.ref_search_distinct(Q, gq, gs, k, groups, rl, ql, mode, off)
    if kind is None:                                                               # the planted duplicates, on the reference first
        lead = (want[1][0] - off).tolist()
        if layout == "dup_in":                                                     # rows 3 = 5 share a group: the lower index, once
            assert lead[0] == 3 and 5 not in lead
        if layout == "dup_across" and k >= 2:                                      # two groups: both, in index order
            assert lead[:2] == [3, 5]
        if Bq > 1 and Ng > 300 and layout == "dup_in":
            assert (want[1][1] - off)[0] == 17 and not np.isin(want[1][1] - off, [Ng - 200, Ng - 1]).any()
        if Bq > 1 and Ng > 300 and layout == "dup_across" and k >= 3:
            assert (want[1][1] - off)[:3].tolist() == [17, Ng - 200, Ng - 1]
    _same(_search(Q, gq, gs, k, groups, rl, ql, mode, off), want, "default")
    if Ng >= 40000 and layout in ("runs", "perm"):                                 # the layouts the capacity plan is derived for
        got = _search(Q, gq, gs, k, groups, rl, ql, mode, off, flags=_native.TOPK_NO_FALLBACK)
        assert (_np(got[1]) != -2).all(), f"{int((_np(got[1])[:, 0] == -2).sum())} of {Bq} queries overflowed"
        _same(got, want, "no fallback")


# ------------------------------------------------------------------------------------------------------------------ one group per row

@pytest.mark.parametrize("layout", ["own", "negative"])
@pytest.mark.parametrize("Bq,Ng,C,k", [(65, 40000, 256, 10), (7, 4097, 48, 100), (9, 200, 64, 256)])
def test_one_group_per_row_equals_the_plain_and_the_filtered_search(Bq, Ng, C, k, layout):
    from cor_amd import ops
    G, gq, gs = _gallery(Ng, C)
    groups = _groups(layout, Ng, 5)
    Q, src = _queries(G, Bq, 2)
    dq, dg, ds, dgr = _dev(Q), _dev(gq), _dev(gs), _dev(groups)
    got = ops.similarity_topk_i8_distinct(dq, dg, ds, k, dgr, g_offset=1000)
    assert _eq(got, ops.similarity_topk_i8(dq, dg, ds, k, g_offset=1000))
    _same(got, R.ref_search(Q, gq, gs, k, 1000))
    rl = np.random.default_rng(8).integers(0, 4, Ng).astype(np.int32)
    ql = rl[src].copy()
    ql[3::7] = -1
    for mode in ("eq", "ne"):
        got = ops.similarity_topk_i8_distinct(dq, dg, ds, k, dgr, _dev(rl), _dev(ql), mode=mode, g_offset=7)
        assert _eq(got, ops.similarity_topk_i8_filtered(dq, dg, ds, k, _dev(rl), _dev(ql), mode=mode, g_offset=7)), mode
        _same(got, FR.ref_search_filtered(Q, gq, gs, k, rl, ql, mode, 7), mode)


# ------------------------------------------------------------------------------------------------------------------ fewer groups than k

@pytest.mark.parametrize("Bq,Ng,k,ngr,on_plan", [(7, 200, 256, 5, True), (16, 2000, 50, 12, True), (8, 30000, 20, 7, False)])
def test_fewer_groups_than_k(Bq, Ng, k, ngr, on_plan):
    from cor_amd import _native
    C = 64
    G, gq, gs = _gallery(70001, C)
    G, gq, gs = G[:Ng], gq[:Ng], gs[:Ng]
    rng = np.random.default_rng(Ng)
    groups = rng.integers(0, ngr, Ng).astype(np.int32)
    Q, _ = _queries(G, Bq, 4)
    want = DR.ref_search_distinct(Q, gq, gs, k, groups, offset=1000)
    assert (want[1][:, :ngr] >= 1000).all() and (want[1][:, ngr:] == -1).all() and np.isneginf(want[0][:, ngr:]).all()
    _same(_search(Q, gq, gs, k, groups, offset=1000), want, "unfiltered")
    marked = _search(Q, gq, gs, k, groups, offset=1000, flags=_native.TOPK_NO_FALLBACK)
    if on_plan:
        _same(marked, want, "no fallback")
    else:                                                                          # no threshold without k sampled groups: every query pages
        assert (_np(marked[1]) == -2).all()
    # a filter on the group ids: "eq" keeps ONE group, a label no row carries keeps nothing, "ne" drops one group
    ql = np.arange(Bq, dtype=np.int32) % ngr
    ql[1] = ngr + 3
    ql[2] = -1
    want = DR.ref_search_distinct(Q, gq, gs, k, groups, groups, ql, "eq", 1000)
    assert (want[1][1] == -1).all() and np.isneginf(want[0][1]).all() and (want[1][0, 1:] == -1).all() and want[1][0, 0] >= 1000
    assert (want[1][2, :ngr] >= 1000).all()
    _same(_search(Q, gq, gs, k, groups, groups, ql, "eq", 1000), want, "eq")
    want = DR.ref_search_distinct(Q, gq, gs, k, groups, groups, ql, "ne", 1000)
    assert (want[1][0, :ngr - 1] >= 1000).all() and (want[1][0, ngr - 1:] == -1).all()
    _same(_search(Q, gq, gs, k, groups, groups, ql, "ne", 1000), want, "ne")


# ------------------------------------------------------------------------------------------------------------------ ties and zeros

def test_ties_zero_scales_and_a_zero_query():
    """The duplicated rows, zero scales, negated row and all-zero query of test_gpu_topk_i8.test_ties_zero_scales_and_a_zero_query, with groups
    laid over them, and a query that turns the signed zeros round."""
    Ng, C = 70001, 64
    G, gq, gs = _gallery(Ng, C)
    gq, gs = gq.copy(), gs.copy()
    Q = G[[5, 20000, Ng - 3, 11]] * F(2.0)
    for a, b in ((5, 9), (5, 14), (5, 66), (20000, 45000), (20000, 69999), (Ng - 3, Ng - 1), (Ng - 3, 4)):
        gq[b], gs[b] = gq[a], gs[a]
    gs[[11, 12, 30000]] = 0.0
    gq[12] = -gq[11]
    Q = np.concatenate([Q, np.zeros((1, C), F), -Q[3:4]])                          # query 4: all zero; query 5: the zeros' signs swapped
    groups = _groups("runs", Ng, 1) + 100
    groups[[5, 9, 14]] = 1                                                         # three equal rows in one group: row 5, once
    groups[66] = 2                                                                 # ... the fourth in another: behind row 5
    groups[[20000, 45000]] = 3
    groups[69999] = 4
    groups[[Ng - 3, Ng - 1]] = 5                                                   # both in the ragged last tile
    groups[4] = 6
    groups[[11, 12]] = 7                                                           # a +0.0 and a -0.0 row of ONE group
    groups[30000] = 8
    S = R.ref_scores(Q, gq, gs)[0]
    assert not np.signbit(S[3, 11]) and np.signbit(S[3, 12]) and np.signbit(S[5, 11]) and not np.signbit(S[5, 12])
    assert (S[4] == 0).all() and not np.signbit(S[4]).any()
    first = np.sort(np.unique(DR.group_keys(groups), return_index=True)[1])        # every group's lowest row, ascending
    for k in (10, 100):
        want = DR.ref_topk_distinct(S, k, groups, offset=1000)
        assert want[1][0, :2].tolist() == [1005, 1066] and want[1][1, :2].tolist() == [21000, 70999]
        assert want[1][2, :2].tolist() == [1004, 1000 + Ng - 3]
        assert not np.isin(want[1], [1009, 1014, 46000, 1000 + Ng - 1]).any()
        assert want[1][4].tolist() == (first[:k] + 1000).tolist()                  # the zero query: each group's lowest index
        _same(_search(Q, gq, gs, k, groups, offset=1000), want, f"k={k}")
    # the zero rows reach a list when a filter leaves little else: group 7 is represented by its +0.0 row, whichever index that is
    rl = np.zeros(Ng, np.int32)
    rl[[11, 12, 30000, 5, 9, 66, Ng - 1]] = 1
    ql = np.ones(6, np.int32)
    want = DR.ref_topk_distinct(S, 10, groups, rl, ql, "eq")
    assert (want[1][:, :5] >= 0).all() and (want[1][:, 5:] == -1).all()            # groups 1, 2, 5, 7, 8
    assert 11 in want[1][3] and 12 not in want[1][3] and 12 in want[1][5] and 11 not in want[1][5]
    assert want[1][4, :5].tolist() == [5, 11, 66, 30000, Ng - 1]
    _same(_search(Q, gq, gs, 10, groups, rl, ql, "eq"), want, "filtered zeros")


# ------------------------------------------------------------------------------------------------------------------ overflow

def _overflow_case(kind):
    """(Q, gq, gs, groups, rl, ql, mode, overflowed queries, final queries). The lists overflow because thousands of rows tie for the top."""
    C = 256
    G, gq0, gs0 = _gallery(70001, C)
    if kind == "single":                                                           # 3000 rows, all of one group
        Ng = 3000
        return np.stack([G[0], G[7]]), gq0[:Ng].copy(), gs0[:Ng].copy(), np.full(Ng, 4, np.int32), None, None, "eq", [0, 1], []
    Ng = 20000
    gq, gs = gq0[:Ng].copy(), gs0[:Ng].copy()
    gq[:5000], gs[:5000] = gq0[0], gs0[0]                                          # 5000 identical rows
    groups = _groups("runs", Ng, 3) + 10
    if kind == "one_group":
        groups[:5000] = 1
    else:
        groups[:5000] = np.arange(5000) + 100000                                   # 5000 groups
    Q = np.stack([G[0], G[12345] - F(0.5) * G[0], G[0] * F(3.0)])                  # query 1 scores the duplicates far down: not overflowed
    if kind == "many_groups_eq":                                                   # every third duplicate is allowed: 1667 tied rows, which
        rl = np.ones(Ng, np.int32)                                                 # the lists may or may not hold (no claim either way)
        rl[:5000] = np.where(np.arange(5000) % 3 == 0, 1, 0)
        return Q, gq, gs, groups.astype(np.int32), rl, np.ones(3, np.int32), "eq", [], [1]
    return Q, gq, gs, groups.astype(np.int32), None, None, "eq", [0, 2], [1]


@pytest.mark.parametrize("k", [10, 256])
@pytest.mark.parametrize("kind", ["one_group", "many_groups", "single", "many_groups_eq"])
def test_overflow_is_ranked_exactly_by_the_fallback(kind, k):
    from cor_amd import _native
    Q, gq, gs, groups, rl, ql, mode, ovf, final = _overflow_case(kind)
    want = DR.ref_search_distinct(Q, gq, gs, k, groups, rl, ql, mode, 1000)
    if kind == "one_group":
        assert want[1][0, 0] == 1000 and (want[1][0, 1:] >= 6000).all()            # the 5000 duplicates: once
    elif kind == "many_groups":
        assert want[1][0].tolist() == list(range(1000, 1000 + k))
    elif kind == "many_groups_eq":
        assert want[1][0].tolist() == [1000 + 3 * j for j in range(k)]
    else:
        assert (want[1][:, 0] >= 1000).all() and (want[1][:, 1:] == -1).all()
    _same(_search(Q, gq, gs, k, groups, rl, ql, mode, 1000), want, "fallback")
    marked = _search(Q, gq, gs, k, groups, rl, ql, mode, 1000, flags=_native.TOPK_NO_FALLBACK)
    mi, ms = _np(marked[1]), _np(marked[0])
    assert (mi[ovf] == -2).all() and np.isneginf(ms[ovf]).all()
    for b in range(Q.shape[0]):                                                    # every query: marked in every slot, or already final
        if not ((mi[b] == -2).all() and np.isneginf(ms[b]).all()):
            assert b not in ovf
            assert np.array_equal(mi[b], want[1][b]) and np.array_equal(ms[b].view(np.int32), want[0][b].view(np.int32)), b
        else:
            assert b not in final                                                  # a query of the same call that did not overflow is final


# ------------------------------------------------------------------------------------------------------------------ the raw ABI

def test_argument_checks_through_the_raw_abi():
    from cor_amd import _native as nat
    lib = nat.load()
    E, N = nat.EINVAL, nat.ENOSUPPORT
    Bq, Ng, C, k = 8, 5000, 64, 10
    G, gq, gs = _gallery(70001, C)
    groups = _groups("runs", Ng, 2)
    Q, src = _queries(G[:Ng], Bq, 1)
    dq, dg, ds, dgr = _dev(Q), _dev(gq[:Ng]), _dev(gs[:Ng]), _dev(groups)
    dql = _dev(groups[src])
    ws = torch.empty((lib.cor_topk_i8_distinct_workspace_bytes(Bq, Ng, k),), dtype=torch.uint8, device=DEV)
    out_s = torch.empty((Bq, k), dtype=torch.float32, device=DEV); out_i = torch.empty((Bq, k), dtype=torch.int64, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    base = dict(Q=dq.data_ptr(), G=dg.data_ptr(), gs=ds.data_ptr(), Bq=Bq, Ng=Ng, C=C, k=k, rg=dgr.data_ptr(), rl=dgr.data_ptr(), ql=dql.data_ptr(),
                mode=nat.FILTER_NE, out_s=out_s.data_ptr(), out_i=out_i.data_ptr(), ws=ws.data_ptr(), flags=0)

    def call(**kw):
        a = dict(base, **kw)
        return lib.cor_similarity_topk_i8_distinct(a["Q"], a["G"], a["gs"], a["Bq"], a["Ng"], a["C"], a["k"], 0, a["rg"], a["rl"], a["ql"], a["mode"],
                                                   a["out_s"], a["out_i"], a["ws"], a["flags"], stream)

    for name in ("Q", "G", "gs", "rg", "out_s", "out_i", "ws"):                    # null pointers
        assert call(**{name: None}) == E, name
    assert call(Bq=0) == E and call(Ng=0) == E and call(k=0) == E and call(Bq=-2) == E
    assert call(rl=None) == E and call(ql=None) == E                               # exactly one label pointer
    assert call(mode=2) == E and call(mode=2, rl=None, ql=None) == E               # the mode, also when unfiltered
    assert call(k=257) == N and call(C=272) == N and call(C=40) == N
    for flag in (nat.TOPK_FORCE_LISTS, nat.TOPK_FORCE_GLOBAL_THRESHOLD, nat.TOPK_WAVE_FINAL, nat.TOPK_NO_FALLBACK | nat.TOPK_WAVE_FINAL):
        assert call(flags=flag) == N, flag
    for name in ("Q", "G", "gs", "rg", "rl"):                                      # 16-byte alignment
        assert call(**{name: base[name] + 4}) == E, name
    assert call(ws=base["ws"] + 16) == E
    assert call(rg=None, k=257) == E and call(mode=2, k=257) == E and call(rg=base["rg"] + 4, k=257) == N and call(rg=base["rg"] + 4, flags=1) == N
    torch.cuda.synchronize()
    # and the valid calls, filtered and not, straight through the ABI
    assert call() == 0
    torch.cuda.synchronize()
    _same((out_s, out_i), DR.ref_search_distinct(Q, gq[:Ng], gs[:Ng], k, groups, groups, groups[src], "ne"), "ne")
    assert call(rl=None, ql=None, flags=nat.TOPK_NO_FALLBACK) == 0
    torch.cuda.synchronize()
    _same((out_s, out_i), DR.ref_search_distinct(Q, gq[:Ng], gs[:Ng], k, groups), "unfiltered")


# ------------------------------------------------------------------------------------------------------------------ ids as the caller has them

def test_ids_through_a_view_and_as_int64():
    from cor_amd import ops
    Ng, C, k = 4097, 128, 33
    G, gq, gs = _gallery(Ng, C)
    groups = _groups("runs", Ng, 5)
    Q, src = _queries(G, 7, 6)
    ql = groups[src]
    want = DR.ref_search_distinct(Q, gq, gs, k, groups, groups, ql, "ne")
    dq, dg, ds = _dev(Q), _dev(gq), _dev(gs)
    big = _dev(np.concatenate([np.array([123], np.int32), groups]))
    view = big[1:]                                                                 # 4 bytes into its buffer
    assert view.data_ptr() % 16 == 4
    _same(ops.similarity_topk_i8_distinct(dq, dg, ds, k, view, view, _dev(ql), mode="ne"), want, "view")
    _same(ops.similarity_topk_i8_distinct(dq, dg, ds, k, _dev(groups.astype(np.int64)), _dev(groups.astype(np.int64)), _dev(ql.astype(np.int64)),
                                          mode="ne"), want, "int64")
    _same(ops.similarity_topk_i8_distinct(dq, dg, ds, k, torch.from_numpy(groups), torch.from_numpy(groups), ql.tolist(), mode="ne"), want, "host ids")
    assert big[0].item() == 123 and torch.equal(view.cpu(), torch.from_numpy(groups))


# ------------------------------------------------------------------------------------------------------------------ streams

def test_side_stream_and_graph_replay():
    from cor_amd import ops
    G, gq, gs = _gallery(40000, 256)
    groups = _groups("runs", 40000, 4)
    (Qa, sa), (Qb, sb) = _queries(G, 33, 3), _queries(G, 33, 8)
    qla, qlb = groups[sa], groups[sb]
    q, sc, dgr = _dev(gq), _dev(gs), _dev(groups)
    Q, dql = _dev(Qa), _dev(qla)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = ops.similarity_topk_i8_distinct(Q, q, sc, 100, dgr, dgr, dql, mode="ne")   # (also sets the kernels' one-time attributes before the capture)
    side.synchronize()
    _same(got, DR.ref_search_distinct(Qa, gq, gs, 100, groups, groups, qla, "ne"), "side stream")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cs, ci = ops.similarity_topk_i8_distinct(Q, q, sc, 100, dgr, dgr, dql, mode="ne")
    Q.copy_(_dev(Qb))
    dql.copy_(_dev(qlb))
    graph.replay()
    torch.cuda.synchronize()
    assert not np.array_equal(qla, qlb)
    eager = ops.similarity_topk_i8_distinct(Q, q, sc, 100, dgr, dgr, dql, mode="ne")
    assert _eq((cs, ci), eager)
    _same((cs, ci), DR.ref_search_distinct(Qb, gq, gs, 100, groups, groups, qlb, "ne"), "graph replay")


# ------------------------------------------------------------------------------------------------------------------ the Python layers

def test_python_layers(tmp_path):
    from cor_amd import ops, retrieval
    Ng, C = 4097, 64
    G = torch.from_numpy(_gallery(Ng, C)[0])
    groups = _groups("runs", Ng, 9)
    src = [3, 900, 4096, 2000, 1999]
    Q = (G[src] + 0.01).to(DEV)
    ql = torch.from_numpy(groups[src].copy())
    ql[3] = -1
    shard = retrieval.GalleryShard(G.to(DEV), offset=1000, labels=groups, groups=groups)
    qs = shard.quantized()
    assert isinstance(qs, retrieval.QuantizedShard) and qs.labels is shard.labels and qs.groups is shard.groups and qs.offset == 1000
    wq, ws = R.ref_quantize(G)
    got = qs.search(Q, 20, distinct=True)
    assert _eq(got, ops.similarity_topk_i8_distinct(Q, qs.rows, qs.scales, 20, qs.groups, g_offset=1000))
    _same(got, DR.ref_search_distinct(_np(Q), wq, ws, 20, groups, offset=1000), "distinct")
    for m in ("eq", "ne"):
        got = qs.search(Q, 20, query_labels=ql, mode=m, distinct=True)
        assert _eq(got, ops.similarity_topk_i8_distinct(Q, qs.rows, qs.scales, 20, qs.groups, qs.labels, ql.to(DEV), mode=m, g_offset=1000))
        _same(got, DR.ref_search_distinct(_np(Q), wq, ws, 20, groups, groups, ql.numpy(), m, 1000), m)
    assert _eq(qs.search(Q, 20), ops.similarity_topk_i8(Q, qs.rows, qs.scales, 20, g_offset=1000))       # not distinct: as before
    plain = retrieval.QuantizedShard.from_rows(G.to(DEV), labels=groups)
    assert plain.groups is None
    with pytest.raises(ValueError, match="no group ids"):
        plain.search(Q, 5, distinct=True)
    with pytest.raises(ValueError):
        retrieval.QuantizedShard(qs.rows, qs.scales, groups=groups[:-1])
    # two int8 segments split INSIDE a run of one image = the single shard
    cut = next(g for g in range(2000, Ng) if groups[g] == groups[g - 1])
    a = retrieval.QuantizedShard(qs.rows[:cut], qs.scales[:cut], offset=1000, labels=groups[:cut], groups=groups[:cut])
    b = retrieval.QuantizedShard(qs.rows[cut:], qs.scales[cut:], offset=1000 + cut, labels=groups[cut:], groups=groups[cut:])
    gset = retrieval.GallerySet([a, b])
    Qc = torch.cat([Q, (G[[cut - 1, cut]] + 0.01).to(DEV)])                         # two queries at the cut image
    qlc = torch.cat([ql, torch.from_numpy(groups[[cut, 5]].copy())])
    assert _eq(gset.search(Qc, 30, distinct=True), qs.search(Qc, 30, distinct=True))
    assert _eq(gset.search(Qc, 30, query_labels=qlc, mode="ne", distinct=True), qs.search(Qc, 30, query_labels=qlc, mode="ne", distinct=True))
    # coarse stage of a distinct two-stage search = the composition of the two calls, one row per image, the query's own image gone
    fine = retrieval.GalleryShard(G.to(DEV), offset=1000, groups=groups)
    ts, ti = retrieval.two_stage_search(Q, qs, fine, 10, 50, query_labels=ql, mode="ne", distinct=True)
    assert _eq((ts, ti), fine.rescore(Q, qs.search(Q, 50, query_labels=ql, mode="ne", distinct=True)[1], 10))
    img = torch.from_numpy(groups)[(ti.cpu() - 1000).clamp(min=0)]
    assert (ti >= 1000).all() and not ((img == ql[:, None]) & (ql[:, None] >= 0)).any()
    assert all(len(set(r.tolist())) == 10 for r in img)
    # disk round trip
    path = str(tmp_path / "gal")
    retrieval.save_gallery(path, qs.rows, world=2, scales=qs.scales, labels=groups, groups=groups)
    lo, hi = retrieval.shard_bounds(Ng, 2, 1)
    back = retrieval.load_gallery_shard(path, 1, DEV)
    assert isinstance(back, retrieval.QuantizedShard) and back.offset == lo and len(back) == hi - lo
    assert back.groups.dtype == torch.int32 and back.groups.device == back.rows.device and torch.equal(back.groups.cpu(), torch.from_numpy(groups[lo:hi]))
    _same(back.search(Q, 5, query_labels=ql, mode="ne", distinct=True),
          DR.ref_search_distinct(_np(Q), wq[lo:hi], ws[lo:hi], 5, groups[lo:hi], groups[lo:hi], ql.numpy(), "ne", lo), "round trip")
    # an empty shard with groups
    empty = retrieval.QuantizedShard.from_rows(shard.rows[:0], offset=7, groups=groups[:0])
    es, ei = empty.search(Q, 4, distinct=True)
    assert len(empty) == 0 and (ei == -1).all() and torch.isneginf(es).all() and tuple(ei.shape) == (5, 4)


def test_grouped_quantized_shard_in_a_one_rank_distributed_search():
    """distributed_search takes a QuantizedShard with groups and distinct=True unchanged (one-rank nccl group, gather and deferred forms)."""
    import socket
    import torch.distributed as dist
    from cor_amd import retrieval
    if dist.is_initialized():
        pytest.skip("a process group already exists in this process")
    G = torch.from_numpy(_gallery(4097, 128)[0])
    groups = _groups("runs", 4097, 2)
    src = [7, 4000, 12]
    Q = (G[src] * 0.9).to(DEV)
    ql = torch.from_numpy(groups[src].copy())
    shard = retrieval.QuantizedShard.from_rows(G.to(DEV), offset=100, labels=groups, groups=groups)
    s0, i0 = shard.search(Q, 50, query_labels=ql, mode="ne", distinct=True)
    assert not torch.isin(i0.cpu(), torch.tensor(src) + 100).any()
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=torch.device(DEV))
    try:
        s1, i1 = retrieval.distributed_search(Q, shard, 50, max_local=8, always_collective=True, query_labels=ql, filter_mode="ne", distinct=True)
        s2, i2 = retrieval.distributed_search(Q, shard, 50, max_local=8, always_collective=True, defer=True, query_labels=ql, filter_mode="ne",
                                              distinct=True).result()
        torch.cuda.synchronize()
        for s_, i_ in ((s1, i1), (s2, i2)):
            assert torch.equal(i_, i0.cpu()) and torch.equal(s_.view(torch.int32), s0.cpu().view(torch.int32))
    finally:
        dist.destroy_process_group()

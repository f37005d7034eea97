"""CPU side of the distinct-group int8 gallery search: the library's exports and argument checks (no device needed), the plan's sample
bound and workspace size, the Python front's validation, the save_gallery manifest of an int8 gallery with group ids, and the restatement
tests/i8_distinct_refs.py against a per-group restatement written out here."""
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import i8_distinct_refs as DR
from tests import i8_filtered_refs as FR
from tests import i8_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _proto_args(hdr, ret, name):
    proto = re.search(r"^" + ret + r"\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr, flags=re.M | re.S)
    assert proto, f"{name} is not declared in include/cor_amd.h"
    return len(proto.group(1).split(","))


def test_header_and_ctypes_table_agree():
    from cor_amd import _native
    lib = _native.load()
    hdr = open(os.path.join(ROOT, "include", "cor_amd.h")).read()
    sig = _native.SIGNATURES
    name = "cor_similarity_topk_i8_distinct"
    assert _proto_args(hdr, "int", name) == 17 == len(sig[name])
    assert _proto_args(hdr, "long", "cor_topk_i8_distinct_workspace_bytes") == 3 == len(sig["cor_topk_i8_distinct_workspace_bytes"])
    assert _proto_args(hdr, "int", "cor_topk_i8_distinct_sample_values") == 3 == len(sig["cor_topk_i8_distinct_sample_values"])
    assert sig[name][7] is _native._ll                                              # g_offset
    assert sig[name][8] is _native._p and sig[name][9] is _native._p and sig[name][10] is _native._p   # groups, row labels, query labels
    assert sig[name][11] is _native._i                                              # filter_mode
    assert lib.cor_similarity_topk_i8_distinct.restype is _native._i
    assert lib.cor_topk_i8_distinct_workspace_bytes.restype is _native._l
    assert "Distinct-group int8 search does not exist" not in hdr


def test_abi_argument_errors_need_no_gpu():
    """Every argument check comes before any HIP call, in the order and with the codes of cor_similarity_topk_i8_filtered, the group pointer
    added and the labels both or neither."""
    from cor_amd import _native
    lib = _native.load()
    E, N = _native.EINVAL, _native.ENOSUPPORT
    buf = torch.zeros(4096, dtype=torch.uint8)
    p = (buf.data_ptr() + 255) & ~255                                              # 256-byte aligned, 3 KiB behind it

    def call(Q=p, G=p, gs=p, Bq=1, Ng=8, C=64, k=4, off=0, rg=p, rl=p, ql=p, mode=_native.FILTER_EQ, out_s=p, out_i=p, ws=p, flags=0):
        return lib.cor_similarity_topk_i8_distinct(Q, G, gs, Bq, Ng, C, k, off, rg, rl, ql, mode, out_s, out_i, ws, flags, None)

    assert call(Q=None) == E and call(G=None) == E and call(gs=None) == E and call(rg=None) == E and call(out_s=None) == E and call(out_i=None) == E
    assert call(ws=None) == E and call(Bq=0) == E and call(Ng=0) == E and call(k=0) == E and call(Bq=-1) == E and call(k=-5) == E
    assert call(rl=None) == E and call(ql=None) == E                               # exactly one label pointer
    assert call(mode=2) == E and call(mode=-1) == E and call(mode=2, rl=None, ql=None) == E       # the mode counts when unfiltered too
    assert call(k=257) == N and call(C=272) == N and call(C=40) == N and call(C=8) == N
    assert call(k=257, rl=None, ql=None) == N
    for flag in (_native.TOPK_FORCE_LISTS, _native.TOPK_FORCE_GLOBAL_THRESHOLD, _native.TOPK_WAVE_FINAL, 4, 1 << 20,
                 _native.TOPK_NO_FALLBACK | _native.TOPK_FORCE_LISTS):
        assert call(flags=flag) == N and call(flags=flag, rl=None, ql=None) == N, flag
    assert call(Q=p + 4) == E and call(G=p + 8) == E and call(gs=p + 4) == E and call(rg=p + 4) == E and call(rl=p + 4) == E
    assert call(ws=p + 16) == E and call(rg=p + 8, rl=None, ql=None) == E
    # the order of check_topk_call: null / counts, the mode, the shape and the flags, the alignment
    assert call(rg=None, k=257) == E and call(mode=2, k=257) == E and call(rg=p + 4, k=257) == N and call(rg=p + 4, flags=1) == N
    assert call(Ng=0, C=40) == E and call(rg=p + 4, mode=5) == E and call(rl=None, C=40) == E


def test_threshold_kernel_never_gets_more_sample_values_than_it_sorts():
    """The plan is host code: for every shard size the threshold kernel is handed at most the 4096 sample values its LDS sort holds (4
    streams x at most 256 sample slices x 4 values with a filter; the int8 scan has no label ring, so the slice count does not grow)."""
    from cor_amd import _native
    lib = _native.load()
    ngs = [4096, 4097]
    n = 1
    while n <= 2 ** 31 - 1:
        ngs.append(n)
        n *= 3
    ngs.append(2 ** 31 - 1)
    seen = set()
    for Ng in ngs:
        for Bq in (1, 512, 513):
            for k in (1, 10, 100, 256):
                n = lib.cor_topk_i8_distinct_sample_values(Bq, Ng, k)
                assert 0 <= n <= 4096, (Bq, Ng, k, n)
                assert (n == 0) == (Ng <= 4096), (Bq, Ng, k, n)                     # a tiny shard has no sample pass
                seen.add(n)
    assert 4096 in seen                                                            # the bound is reached, not merely respected
    assert lib.cor_topk_i8_distinct_sample_values(8, 5000, 257) == _native.EINVAL
    assert lib.cor_topk_i8_distinct_sample_values(0, 5000, 10) == _native.EINVAL


def test_workspace_bytes():
    from cor_amd import _native
    lib = _native.load()
    E = _native.EINVAL
    ws = lib.cor_topk_i8_distinct_workspace_bytes
    assert ws(0, 10, 1) == E and ws(1, 0, 1) == E and ws(1, 10, 0) == E and ws(1, 10, 257) == E and ws(-3, 10, 1) == E
    for Ng, k in ((1, 1), (17, 256), (4096, 10), (4097, 10), (70001, 33), (100_000, 100), (1_000_000, 10), (1_000_000, 100), (1_000_000, 256)):
        prev = 0
        for Bq in (1, 7, 32, 257, 511, 512, 513, 1024, 1025, 4096):                 # across the 512-query groups, where the plan changes
            n = ws(Bq, Ng, k)
            assert n > 0 and n % 256 == 0 and n < 1 << 32, (Bq, Ng, k, n)
            assert n >= prev, (Bq, Ng, k, n, prev)
            prev = n


def test_python_validation_and_no_cpu_path():
    from cor_amd import _native, ops, retrieval
    Q, Gq, gs = torch.zeros((2, 32)), torch.zeros((5, 32), dtype=torch.int8), torch.zeros(5)
    rg, rl, ql = torch.arange(5, dtype=torch.int32), torch.zeros(5, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    f = ops.similarity_topk_i8_distinct
    for bad in (lambda: f(Q, Gq, gs, 0, rg), lambda: f(Q, Gq, gs, 257, rg), lambda: f(Q, Gq, gs, 3, rg, mode="lt"),
                lambda: f(Q, Gq, gs, 3, rg, rl, ql, mode="lt"),
                lambda: f(Q, Gq.float(), gs, 3, rg),                               # not int8 rows
                lambda: f(Q, Gq, gs[:4], 3, rg), lambda: f(Q, Gq, gs.double(), 3, rg),
                lambda: f(Q, Gq, gs, 3, rg[:4]), lambda: f(Q, Gq, gs, 3, rg.reshape(5, 1)), lambda: f(Q, Gq, gs, 3, rg.float()),
                lambda: f(Q, Gq, gs, 3, rg, rl[:4], ql), lambda: f(Q, Gq, gs, 3, rg, rl, ql[:1]), lambda: f(Q, Gq, gs, 3, rg, rl.float(), ql),
                lambda: f(Q, Gq, gs, 3, rg, rl, ql.double()),
                lambda: f(Q, Gq, gs, 3, rg, rl, None), lambda: f(Q, Gq, gs, 3, rg, None, ql),     # exactly one of the two label vectors
                lambda: f(Q, Gq, gs, 3, rg, flags=1), lambda: f(Q, Gq, gs, 3, rg, rl, ql, flags=_native.TOPK_NO_FALLBACK | 4)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(RuntimeError, match="GPU only"):                            # valid arguments on the CPU: no CPU path
        f(Q, Gq, gs, 3, rg)
    with pytest.raises(RuntimeError, match="GPU only"):
        f(Q, Gq, gs, 3, rg.long(), rg.long(), ql.long(), mode="ne", flags=_native.TOPK_NO_FALLBACK)
    sh = retrieval.QuantizedShard.__new__(retrieval.QuantizedShard)                 # the constructor refuses CPU tensors; search's own checks
    sh.rows, sh.scales, sh.offset, sh.labels, sh.groups = Gq, gs, 0, None, None
    with pytest.raises(ValueError, match="no group ids"):
        sh.search(Q, 3, distinct=True)                                             # a shard built without groups
    sh.groups = rg
    with pytest.raises(RuntimeError, match="GPU only"):                            # with groups the search reaches the op
        sh.search(Q, 3, distinct=True)
    with pytest.raises(ValueError):
        sh.search(Q, 3, query_labels=ql, distinct=True)                            # ... but a filter still needs row labels
    sh.labels = rg
    with pytest.raises(RuntimeError, match="GPU only"):
        sh.search(Q, 3, query_labels=ql, mode="ne", distinct=True)
    with pytest.raises(ValueError):
        retrieval.QuantizedShard(Gq, gs, groups=rg[:4])                            # group ids of the wrong length
    with pytest.raises(ValueError):
        retrieval.QuantizedShard(Gq, gs, offset=3, groups=torch.zeros((5, 1), dtype=torch.int32))
    with pytest.raises(RuntimeError):
        retrieval.QuantizedShard(Gq, gs, labels=rl, groups=rg)                     # well-formed, but on the CPU


def test_save_gallery_writes_groups_per_shard(tmp_path):
    from cor_amd import retrieval
    rows = torch.arange(7 * 16, dtype=torch.int32).reshape(7, 16).to(torch.int8)
    scales, labels = torch.arange(7, dtype=torch.float32) + 1, torch.tensor([4, 4, -1, 9, 0, 0, 4])
    groups = torch.tensor([0, 0, 1, 1, 1, -3, 2])
    path = str(tmp_path / "gal")
    retrieval.save_gallery(path, rows, world=2, scales=scales, groups=groups, labels=labels)
    man = json.load(open(path + ".manifest.json"))
    assert man["scales"] is True and man["labels"] is True and man["groups"] is True and len(man["shards"]) == 2
    for r, sh in enumerate(man["shards"]):
        lo, hi = retrieval.shard_bounds(7, 2, r)
        assert (sh["lo"], sh["hi"]) == (lo, hi)
        assert torch.equal(torch.load(sh["file"]), rows[lo:hi]) and torch.equal(torch.load(sh["scales_file"]), scales[lo:hi])
        got = torch.load(sh["groups_file"])
        assert got.dtype == torch.int32 and torch.equal(got, groups[lo:hi].to(torch.int32))
        assert torch.equal(torch.load(sh["labels_file"]), labels[lo:hi].to(torch.int32))


# ------------------------------------------------------------------------------------------------------------------ the reference

def _per_group(S, k, groups, rl, ql, mode, offset):
    """the definition the other way round: the top-1 of every group among the allowed rows (lexsort by (key desc, row asc)), then the
    representatives ranked the same way"""
    Bq, Ng = S.shape
    key = R.f2key(S).astype(np.int64)
    s, i = np.full((Bq, k), -np.inf, F), np.full((Bq, k), -1, np.int64)
    for b in range(Bq):
        members = {}
        for g in range(Ng):
            if rl is not None and not FR.allowed_rows(rl, int(ql[b]), mode)[g]:
                continue
            members.setdefault(int(groups[g]) if groups[g] >= 0 else ("row", g), []).append(g)
        reps = []
        for rows in members.values():
            rows = np.array(rows, np.int64)
            reps.append(int(rows[np.lexsort((rows, -key[b, rows]))][0]))
        reps = np.array(sorted(reps), np.int64)
        if reps.size:
            o = reps[np.lexsort((reps, -key[b, reps]))][:k]
            s[b, :len(o)], i[b, :len(o)] = S[b, o], o + offset
    return s, i


def _bits_equal(a, b):
    return np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.int32), b[0].view(np.int32))


def test_the_reference_on_hand_made_rows():
    # 10 rows. group 0 = rows 0, 4 (tie at 2.0: row 0 represents it), group 1 = rows 1, 2, group 2 = rows 3, 7 (+0.0 and -0.0: row 7,
    # the +0.0, represents it although its index is higher), rows 5, 6 carry negative ids (each its own group), group 3 = rows 8, 9
    groups = np.array([0, 1, 1, 2, 0, -1, -1, 2, 3, 3], np.int32)
    S = np.array([[2.0, 1.0, 3.0, -0.0, 2.0, 0.5, 0.5, 0.0, -1.0, -2.0]], F)
    s, i = DR.ref_topk_distinct(S, 8, groups)
    assert i[0].tolist() == [2, 0, 5, 6, 7, 8, -1, -1]
    assert s[0, :6].tolist() == [3.0, 2.0, 0.5, 0.5, 0.0, -1.0] and not np.signbit(s[0, 4]) and np.isneginf(s[0, 6:]).all()
    assert _bits_equal((s, i), _per_group(S, 8, groups, None, None, "eq", 0))
    # "ne" on the group ids: query label 1 drops group 1, so row 0 leads; label -1 is unrestricted
    ql = np.array([1], np.int32)
    s, i = DR.ref_topk_distinct(S, 3, groups, groups, ql, "ne", 100)
    assert i[0].tolist() == [100, 105, 106]
    s, i = DR.ref_topk_distinct(S, 3, groups, groups, np.array([-1], np.int32), "ne")
    assert i[0].tolist() == [2, 0, 5]
    # "eq" on labels that allow only rows 3 and 9: two groups, then the tail; a label no row carries: only the tail
    rl = np.array([0, 0, 0, 5, 0, 0, 0, 0, 0, 5], np.int32)
    s, i = DR.ref_topk_distinct(S, 4, groups, rl, np.array([5], np.int32), "eq")
    assert i[0].tolist() == [3, 9, -1, -1] and np.signbit(s[0, 0]) and s[0, 1] == -2.0
    s, i = DR.ref_topk_distinct(S, 4, groups, rl, np.array([6], np.int32), "eq")
    assert (i == -1).all() and np.isneginf(s).all()


def test_zero_scales_give_signed_zeros_and_the_reference_orders_them():
    rng = np.random.default_rng(3)
    G = rng.standard_normal((12, 32)).astype(F)
    gq, gs = R.ref_quantize(G)
    gq, gs = gq.copy(), gs.copy()
    gq[7] = -gq[2]
    gs[[2, 7]] = 0.0                                                               # rows 2 and 7: +0.0 and -0.0 (or the reverse) for any query
    Q = np.stack([G[2], -G[2], np.zeros(32, F)])
    S = R.ref_scores(Q, gq, gs)[0]
    assert np.signbit(S[0, 7]) and not np.signbit(S[0, 2]) and np.signbit(S[1, 2]) and not np.signbit(S[1, 7]) and (S[2] == 0).all()
    groups = np.array([0, 0, 9, 1, 1, 1, 2, 9, 3, 3, -1, -1], np.int32)            # rows 2 and 7 share group 9
    for k in (3, 12):
        got = DR.ref_search_distinct(Q, gq, gs, k, groups, offset=5)
        assert _bits_equal(got, _per_group(S, k, groups, None, None, "eq", 5))
    got = DR.ref_search_distinct(Q, gq, gs, 12, groups)
    assert 2 in got[1][0] and 7 not in got[1][0] and 7 in got[1][1] and 2 not in got[1][1]        # the +0.0 row represents group 9
    assert got[1][2].tolist() == [0, 2, 3, 6, 8, 10, 11, -1, -1, -1, -1, -1]       # the zero query: every group's lowest index


@pytest.mark.parametrize("mode", [None, "eq", "ne"])
@pytest.mark.parametrize("Bq,Ng,k", [(5, 40, 7), (3, 9, 16), (70, 33, 4)])
def test_the_reference_against_the_per_group_restatement(Bq, Ng, k, mode):
    rng = np.random.default_rng(Bq * 100 + Ng)
    S = rng.integers(-3, 4, (Bq, Ng)).astype(F) * F(0.25)                          # few distinct values: duplicate scores everywhere
    S[0, 1], S[0, 2] = F(0.0), F(-0.0)
    groups = np.repeat(np.arange(Ng), rng.integers(1, 5, Ng))[:Ng].astype(np.int32)
    groups[rng.permutation(Ng)[:4]] = -1 - rng.integers(0, 2, 4)                   # negative ids that repeat
    groups[2] = groups[1]                                                          # the signed zeros in one group
    rl = ql = None
    if mode == "eq":
        rl = rng.integers(0, 3, Ng).astype(np.int32)
        ql = rng.integers(0, 4, Bq).astype(np.int32)                               # label 3: no row carries it
        ql[0] = -1
    elif mode == "ne":
        rl = groups
        ql = groups[rng.integers(0, Ng, Bq)].copy()                                # the query's own image (a negative id: unrestricted)
    for off in (0, 2 ** 33 + 5):
        got = DR.ref_topk_distinct(S, k, groups, rl, ql, mode or "eq", off, chunk=3)
        assert _bits_equal(got, _per_group(S, k, groups, rl, ql, mode, off))
    for b in range(Bq):
        rows = got[1][b][got[1][b] >= 0] - (2 ** 33 + 5)
        keys = DR.group_keys(groups)[rows]
        assert len(set(keys.tolist())) == len(rows)                                # no group twice
        n = len(rows)
        assert (got[1][b, n:] == -1).all() and np.isneginf(got[0][b, n:]).all()

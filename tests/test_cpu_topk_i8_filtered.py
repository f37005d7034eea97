"""CPU side of the filtered int8 gallery search: the library's exports and argument checks (no device needed), the Python front's
validation, the save_gallery manifest of a labelled int8 gallery, and the restatement tests/i8_filtered_refs.py against a per-query
lexsort written out here."""
import json
import os
import re

import numpy as np
import pytest
import torch

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
    assert _proto_args(hdr, "int", "cor_similarity_topk_i8_filtered") == 16 == len(sig["cor_similarity_topk_i8_filtered"])
    assert _proto_args(hdr, "long", "cor_topk_i8_filtered_workspace_bytes") == 3 == len(sig["cor_topk_i8_filtered_workspace_bytes"])
    assert sig["cor_similarity_topk_i8_filtered"][7] is _native._ll                # g_offset
    assert sig["cor_similarity_topk_i8_filtered"][10] is _native._i                # filter_mode, behind the two label pointers
    assert sig["cor_similarity_topk_i8_filtered"][8] is _native._p and sig["cor_similarity_topk_i8_filtered"][9] is _native._p
    assert lib.cor_similarity_topk_i8_filtered.restype is _native._i
    assert lib.cor_topk_i8_filtered_workspace_bytes.restype is _native._l


def test_abi_argument_errors_need_no_gpu():
    """Every argument check comes before any HIP call, in the order and with the codes of cor_similarity_topk_i8."""
    from cor_amd import _native
    lib = _native.load()
    E, N = _native.EINVAL, _native.ENOSUPPORT
    buf = torch.zeros(4096, dtype=torch.uint8)
    p = (buf.data_ptr() + 255) & ~255                                              # 256-byte aligned, 3 KiB behind it

    def call(Q=p, G=p, gs=p, Bq=1, Ng=8, C=64, k=4, off=0, rl=p, ql=p, mode=_native.FILTER_EQ, out_s=p, out_i=p, ws=p, flags=0):
        return lib.cor_similarity_topk_i8_filtered(Q, G, gs, Bq, Ng, C, k, off, rl, ql, mode, out_s, out_i, ws, flags, None)

    assert call(Q=None) == E and call(G=None) == E and call(gs=None) == E and call(out_s=None) == E and call(out_i=None) == E
    assert call(rl=None) == E and call(ql=None) == E and call(rl=None, ql=None) == E
    assert call(ws=None) == E and call(Bq=0) == E and call(Ng=0) == E and call(k=0) == E and call(Bq=-1) == E and call(k=-5) == E
    assert call(mode=2) == E and call(mode=-1) == E and call(mode=_native.FILTER_NE, Q=None) == E
    assert call(k=257) == N and call(C=272) == N and call(C=40) == N and call(C=8) == N
    for flag in (_native.TOPK_FORCE_LISTS, _native.TOPK_FORCE_GLOBAL_THRESHOLD, _native.TOPK_WAVE_FINAL, 4, 1 << 20,
                 _native.TOPK_NO_FALLBACK | _native.TOPK_FORCE_LISTS):
        assert call(flags=flag) == N, flag
    assert call(Q=p + 4) == E and call(G=p + 8) == E and call(gs=p + 4) == E and call(rl=p + 4) == E and call(ws=p + 16) == E
    # the order of check_topk_call: null / counts, the mode, the shape and the flags, the alignment
    assert call(Q=None, k=257) == E and call(mode=2, k=257) == E and call(Q=p + 4, k=257) == N and call(rl=p + 4, flags=1) == N
    assert call(Ng=0, C=40) == E and call(rl=p + 4, mode=5) == E

    ws = lib.cor_topk_i8_filtered_workspace_bytes
    assert ws(0, 10, 1) == E and ws(1, 0, 1) == E and ws(1, 10, 0) == E and ws(1, 10, 257) == E and ws(-3, 10, 1) == E
    for Bq, Ng, k in ((1, 1, 1), (7, 17, 256), (512, 1_000_000, 10), (512, 1_000_000, 100), (257, 70001, 33)):
        n = ws(Bq, Ng, k)
        assert n > 0 and n % 256 == 0 and n < 1 << 31, (Bq, Ng, k, n)


def test_python_validation_and_no_cpu_path():
    from cor_amd import _native, ops, retrieval
    Q, Gq, gs = torch.zeros((2, 32)), torch.zeros((5, 32), dtype=torch.int8), torch.zeros(5)
    rl, ql = torch.zeros(5, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    f = ops.similarity_topk_i8_filtered
    for bad in (lambda: f(Q, Gq, gs, 0, rl, ql), lambda: f(Q, Gq, gs, 257, rl, ql), lambda: f(Q, Gq, gs, 3, rl, ql, mode="lt"),
                lambda: f(Q, Gq.float(), gs, 3, rl, ql),                           # not int8 rows
                lambda: f(Q, Gq, gs[:4], 3, rl, ql), lambda: f(Q, Gq, gs.double(), 3, rl, ql),
                lambda: f(Q, Gq, gs, 3, rl, ql, flags=1), lambda: f(Q, Gq, gs, 3, rl, ql, flags=_native.TOPK_NO_FALLBACK | 4),
                lambda: f(Q, Gq, gs, 3, rl[:4], ql), lambda: f(Q, Gq, gs, 3, rl, ql[:1]), lambda: f(Q, Gq, gs, 3, rl.reshape(5, 1), ql),
                lambda: f(Q, Gq, gs, 3, rl.float(), ql), lambda: f(Q, Gq, gs, 3, rl, ql.double())):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(RuntimeError, match="GPU only"):                            # valid arguments on the CPU: no CPU path
        f(Q, Gq, gs, 3, rl, ql)
    with pytest.raises(RuntimeError, match="GPU only"):
        f(Q, Gq, gs, 3, rl.long(), ql.long(), mode="ne", flags=_native.TOPK_NO_FALLBACK)
    sh = retrieval.QuantizedShard.__new__(retrieval.QuantizedShard)                 # the constructor refuses CPU tensors; search's own checks
    sh.rows, sh.scales, sh.offset, sh.labels, sh.groups = Gq, gs, 0, None, None
    with pytest.raises(ValueError):
        sh.search(Q, 3, query_labels=ql)                                           # a shard built without labels
    sh.labels = rl
    with pytest.raises(ValueError):
        sh.search(Q, 3, distinct=True)
    with pytest.raises(ValueError):
        sh.search(Q, 3, query_labels=ql, distinct=True)
    with pytest.raises(ValueError):
        retrieval.QuantizedShard(Gq, gs, labels=rl[:4])                            # labels of the wrong length
    with pytest.raises(ValueError):
        retrieval.QuantizedShard(Gq, gs, offset=3, labels=torch.zeros((5, 1), dtype=torch.int32))
    with pytest.raises(RuntimeError):
        retrieval.QuantizedShard(Gq, gs, labels=rl)                                # well-formed, but on the CPU


def test_save_gallery_writes_scales_and_labels_per_shard(tmp_path):
    from cor_amd import retrieval
    rows = torch.arange(7 * 16, dtype=torch.int32).reshape(7, 16).to(torch.int8)
    scales, labels = torch.arange(7, dtype=torch.float32) + 1, torch.tensor([4, 4, -1, 9, 0, 0, 4])
    path = str(tmp_path / "gal")
    retrieval.save_gallery(path, rows, world=2, scales=scales, labels=labels)
    man = json.load(open(path + ".manifest.json"))
    assert man["scales"] is True and man["labels"] is True and man["groups"] is False and len(man["shards"]) == 2
    for r, sh in enumerate(man["shards"]):
        lo, hi = retrieval.shard_bounds(7, 2, r)
        assert (sh["lo"], sh["hi"]) == (lo, hi)
        assert torch.equal(torch.load(sh["file"]), rows[lo:hi]) and torch.equal(torch.load(sh["scales_file"]), scales[lo:hi])
        got = torch.load(sh["labels_file"])
        assert got.dtype == torch.int32 and torch.equal(got, labels[lo:hi].to(torch.int32))


def _lexsort_filtered(S, k, rl, ql, mode, offset):
    """the definition spelled out: per query a lexsort of the allowed rows by (key desc, row asc)"""
    Bq, Ng = S.shape
    key = R.f2key(S).astype(np.int64)
    s, i = np.full((Bq, k), -np.inf, F), np.full((Bq, k), -1, np.int64)
    for b in range(Bq):
        rows = [g for g in range(Ng) if ql[b] < 0 or (mode == "eq" and rl[g] == ql[b]) or (mode == "ne" and rl[g] != ql[b])]
        rows = np.array(rows, np.int64)
        if rows.size:
            o = rows[np.lexsort((rows, -key[b, rows]))][:k]
            s[b, :len(o)], i[b, :len(o)] = S[b, o], o + offset
    return s, i


@pytest.mark.parametrize("mode", ["eq", "ne"])
@pytest.mark.parametrize("Bq,Ng,k", [(5, 40, 7), (3, 9, 16)])
def test_the_reference_against_a_lexsort(Bq, Ng, k, mode):
    rng = np.random.default_rng(Bq * 100 + Ng)
    S = rng.integers(-3, 4, (Bq, Ng)).astype(F) * F(0.25)                          # few distinct values: duplicate scores everywhere
    S[0, 1], S[0, 2] = F(0.0), F(-0.0)                                             # the key tells them apart
    rl = rng.integers(0, 3, Ng).astype(np.int32)
    rl[[0, 3]] = -7                                                                # negative row labels: equal to no restricted query label
    ql = np.zeros(Bq, np.int32)
    ql[0] = -1                                                                     # unrestricted
    if mode == "eq":
        ql[1] = 5                                                                  # no row carries it: nothing allowed
        rl[rl == 2] = 1
        rl[[4, 6, 7]] = 2
        ql[2] = 2                                                                  # 3 allowed rows < k
    else:
        rl2 = np.full(Ng, 1, np.int32)
        rl2[[4, 6, 7]] = 0
        rl2[[0, 3]] = -7
        rl = rl2
        ql[1] = 1                                                                  # ne 1: rows 4, 6, 7 and the two negative ones: 5 < k
        ql[2] = 1                                                                  # (ne allows no row only on a single-label gallery: below)
    n_allowed = [int(FR.allowed_rows(rl, int(q), mode).sum()) for q in ql]
    assert n_allowed[0] == Ng and min(n_allowed[1:]) < k
    if mode == "eq":
        assert n_allowed[1] == 0 and n_allowed[2] == 3
    for off in (0, 2 ** 33 + 5):
        got, want = FR.ref_topk_filtered(S, k, rl, ql, mode, off), _lexsort_filtered(S, k, rl, ql, mode, off)
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[0].view(np.int32), want[0].view(np.int32))
    got = FR.ref_topk_filtered(S, k, rl, ql, mode)
    for b in range(Bq):
        n = min(k, n_allowed[b])
        assert (got[1][b, n:] == -1).all() and np.isneginf(got[0][b, n:]).all() and (got[1][b, :n] >= 0).all()
        assert len(set(got[1][b, :n].tolist())) == n
    assert any(len(np.unique(S[b])) < Ng for b in range(Bq))


def test_ne_with_no_allowed_row_gives_only_the_tail():
    S = np.ones((2, 9), F)
    rl, ql = np.full(9, 3, np.int32), np.array([3, 4], np.int32)
    s, i = FR.ref_topk_filtered(S, 4, rl, ql, "ne", 10)
    assert (i[0] == -1).all() and np.isneginf(s[0]).all() and i[1].tolist() == [10, 11, 12, 13]

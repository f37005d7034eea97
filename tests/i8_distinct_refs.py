"""CPU restatement of the distinct-group int8 gallery search (include/cor_amd.h, "Distinct-group int8 search"), on top of tests/i8_refs.py
and tests/i8_filtered_refs.py. It never calls the code under test.

    group_keys(groups)                                             -> int64 [Ng]: the group of every row; a negative id is a group of its own
    ref_topk_distinct(S, k, groups, rl, ql, mode, offset)          -> (scores f32 [Bq,k], idx i64 [Bq,k]): per query, every group's FIRST
                                                                      allowed row in the order of i8_refs.ref_topk (score key desc, row asc),
                                                                      the k best of those in the same order, then the (-inf, -1) tail
    ref_search_distinct(Q, gq, gscale, k, groups, rl, ql, mode, offset) = ref_topk_distinct(i8_refs.ref_scores(...))

rl / ql None: every row is allowed. The order is one int64 per (query, row), all different (i8_refs.ref_topk's composite: key in the high
word, 2^32 - 1 - row in the low word, largest first), so "a group's first row" is the maximum of its rows' composites and "the k best
representatives" the k largest of those maxima; a disallowed row carries the smallest int64, below every score's composite."""
import numpy as np
import torch

from tests import i8_filtered_refs as FR
from tests import i8_refs as R

F = np.float32
_LOW = np.iinfo(np.int64).min                  # below the composite of every float (key 0 belongs to a NaN pattern no score has)


def group_keys(groups):
    g = np.asarray(groups).astype(np.int64)
    return np.where(g >= 0, g, -1 - np.arange(g.shape[0], dtype=np.int64))      # distinct negative keys for the rows that stand alone


def ref_topk_distinct(S, k, groups, rl=None, ql=None, mode="eq", offset=0, chunk=64):
    Bq, Ng = S.shape
    gk = group_keys(groups)
    assert gk.shape == (Ng,) and (rl is None) == (ql is None)
    order = np.argsort(gk, kind="stable")                                        # rows, group by group
    starts = np.flatnonzero(np.r_[True, gk[order][1:] != gk[order][:-1]])
    ngr = starts.size
    low = (2 ** 32 - 1 - np.arange(Ng, dtype=np.int64))[None, :]
    s, i = np.full((Bq, k), -np.inf, F), np.full((Bq, k), -1, np.int64)
    kk = min(k, ngr)
    for b0 in range(0, Bq, chunk):
        Sb = S[b0:b0 + chunk]
        comp = ((R.f2key(Sb).astype(np.int64) - 2 ** 31) << 32) | low
        if rl is not None:
            for j in range(Sb.shape[0]):
                comp[j, ~FR.allowed_rows(rl, int(ql[b0 + j]), mode)] = _LOW
        best = np.maximum.reduceat(comp[:, order], starts, axis=1)              # every group's first allowed row (or _LOW)
        top = torch.topk(torch.from_numpy(best), kk, dim=1, largest=True, sorted=True).values.numpy()
        rows = 2 ** 32 - 1 - (top & 0xFFFFFFFF)
        ok = top != _LOW
        for j in range(Sb.shape[0]):
            n = int(ok[j].sum())
            assert ok[j, :n].all()
            s[b0 + j, :n], i[b0 + j, :n] = Sb[j, rows[j, :n]], rows[j, :n] + offset
    return s, i


def ref_search_distinct(Q, gq, gscale, k, groups, rl=None, ql=None, mode="eq", offset=0):
    return ref_topk_distinct(R.ref_scores(Q, gq, gscale)[0], k, groups, rl, ql, mode, offset)

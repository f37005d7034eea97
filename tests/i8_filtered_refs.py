"""CPU restatement of the filtered int8 gallery search (include/cor_amd.h, "Filtered int8 search"), on top of tests/i8_refs.py. It never
calls the code under test.

    allowed_rows(row_labels, ql, mode)                          -> bool [Ng]: the rows allowed for a query with label ql
    ref_topk_filtered(S, k, row_labels, query_labels, mode, offset) -> (scores f32 [Bq,k], idx i64 [Bq,k]): per query, i8_refs.ref_topk on the
                                                                   allowed columns of S, indices mapped back, then the (-inf, -1) tail
    ref_search_filtered(Q, gq, gscale, k, rl, ql, mode, offset) = ref_topk_filtered(i8_refs.ref_scores(...))"""
import numpy as np

from tests import i8_refs as R

F = np.float32


def allowed_rows(row_labels, ql, mode):
    rl = np.asarray(row_labels)
    assert mode in ("eq", "ne")
    if ql < 0:
        return np.ones(rl.shape[0], bool)
    return rl == ql if mode == "eq" else rl != ql


def ref_topk_filtered(S, k, row_labels, query_labels, mode, offset=0):
    Bq, Ng = S.shape
    rl, ql = np.asarray(row_labels), np.asarray(query_labels)
    assert rl.shape == (Ng,) and ql.shape == (Bq,)
    s, i = np.full((Bq, k), -np.inf, F), np.full((Bq, k), -1, np.int64)
    for b in range(Bq):
        cols = np.flatnonzero(allowed_rows(rl, int(ql[b]), mode))
        if cols.size == 0:
            continue
        sb, ib = R.ref_topk(np.ascontiguousarray(S[b:b + 1, cols]), k)
        kk = min(k, cols.size)
        s[b, :kk], i[b, :kk] = sb[0, :kk], cols[ib[0, :kk]] + offset
    return s, i


def ref_search_filtered(Q, gq, gscale, k, rl, ql, mode, offset=0):
    return ref_topk_filtered(R.ref_scores(Q, gq, gscale)[0], k, rl, ql, mode, offset)

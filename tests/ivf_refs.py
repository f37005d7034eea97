"""CPU restatements of cor_ivf_build and cor_ivf_search (include/cor_amd.h, "Cell-probing search"), in NumPy / torch on the CPU. They never
call the code under test.

    ref_ivf_build(segs, assigns, K)                                  -> (rows [m,C] as stored, scales f32 [m] or None, ids i64 [m], cell_start i32 [K+1])
    ref_candidates(cell_start, probes_b, K)                          -> the slots of one query's probed cells, in slot order
    ref_ivf_search(Q, rows, scales, ids, cell_start, probes, k)      -> (scores f32 [Bq,k], idx i64 [Bq,k], scanned i32 [Bq])
    ref_exact(Q, rows, scales, ids, k)                               -> the exact search of ALL rows with the ids as indices
    recall(idx, truth)                                               -> the mean share of truth's entries found in idx, per query

segs: [(rows, offset)] or [(rows int8, scales, offset)], rows a CPU torch tensor in its stored dtype (the bits are copied, never converted);
assigns: one int array per segment. m is the number of indexed rows: the reference returns exactly the written slots.
The search gathers the candidate rows in ascending global id and runs the restatement that exists for the dtype: the chain top-k of
oracle.retrieval (float rows; the query rounded to the row dtype for 16-bit rows, as the exact search rounds it) or tests/i8_refs.py
(int8 rows), then maps the indices back to global ids."""
import numpy as np
import torch

from tests import i8_refs

F = np.float32


def ref_ivf_build(segs, assigns, K):
    live = [n for n in range(len(segs)) if segs[n][0].shape[0]]
    C = segs[0][0].shape[1]
    i8 = len(segs[0]) == 3
    if not live:
        return segs[0][0][:0].clone(), (np.zeros(0, F) if i8 else None), np.zeros(0, np.int64), np.zeros(K + 1, np.int32)
    rows = torch.cat([segs[n][0] for n in live])
    scales = np.concatenate([np.asarray(segs[n][1], F) for n in live]) if i8 else None
    ids = np.concatenate([np.arange(segs[n][0].shape[0], dtype=np.int64) + int(segs[n][-1]) for n in live])
    cell = np.concatenate([np.asarray(assigns[n]).astype(np.int64) for n in live])
    assert len(set(ids.tolist())) == ids.shape[0], "the segments' id ranges overlap"
    inside = np.flatnonzero((cell >= 0) & (cell < K))
    order = inside[np.lexsort((ids[inside], cell[inside]))]               # by (cell, id)
    counts = np.bincount(cell[inside], minlength=K).astype(np.int64)
    cell_start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    assert rows.shape[1] == C
    return rows[torch.from_numpy(order)].clone(), (scales[order] if i8 else None), ids[order], cell_start


def ref_candidates(cell_start, probes_b, K):
    cells = sorted({int(c) for c in probes_b if 0 <= int(c) < K})
    if not cells:
        return np.zeros(0, np.int64)
    return np.concatenate([np.arange(int(cell_start[c]), int(cell_start[c + 1]), dtype=np.int64) for c in cells])


def _rank(Q, rows, scales, ids, k):
    """the exact search of that dtype over `rows` (already in ascending id), indices mapped to `ids`, padded to k with (-inf, -1)"""
    Bq = Q.shape[0]
    s, i = np.full((Bq, k), -np.inf, F), np.full((Bq, k), -1, np.int64)
    if rows.shape[0] == 0:
        return s, i
    if scales is not None:
        ss, ii = i8_refs.ref_search(Q, rows.numpy(), scales, k)
        got = ii >= 0
        s[got], i[got] = ss[got], ids[ii[got]]
        return s, i
    from oracle import retrieval as oret
    Qr = torch.from_numpy(np.ascontiguousarray(Q, F)).to(rows.dtype).float()                     # rounded to the row dtype, widened back
    ss, ii = oret.similarity_topk(Qr, rows.float(), k, exact_chain=True)                         # (score desc as floats, index asc)
    kk = ss.shape[1]
    s[:, :kk], i[:, :kk] = ss.numpy(), ids[ii.numpy()]
    return s, i


def ref_ivf_search(Q, rows, scales, ids, cell_start, probes, k):
    Q = np.ascontiguousarray(Q, F)
    Bq, K = Q.shape[0], cell_start.shape[0] - 1
    s, i = np.full((Bq, k), -np.inf, F), np.full((Bq, k), -1, np.int64)
    scanned = np.zeros(Bq, np.int32)
    probes = np.asarray(probes)
    for b in range(Bq):
        cand = ref_candidates(cell_start, probes[b], K)
        scanned[b] = cand.shape[0]
        cand = cand[np.argsort(ids[cand], kind="stable")]                 # ascending global id
        t = torch.from_numpy(cand)
        s[b:b + 1], i[b:b + 1] = _rank(Q[b:b + 1], rows[t], None if scales is None else scales[cand], ids[cand], k)
    return s, i, scanned


def ref_exact(Q, rows, scales, ids, k):
    order = np.argsort(ids, kind="stable")
    return _rank(np.ascontiguousarray(Q, F), rows[torch.from_numpy(order)], None if scales is None else scales[order], ids[order], k)


def recall(idx, truth):
    hit = [len(set(a.tolist()) & set(t.tolist()) - {-1}) / max(len(set(t.tolist()) - {-1}), 1) for a, t in zip(idx, truth)]
    return float(np.mean(hit))

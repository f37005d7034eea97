"""NumPy restatement of cor_similarity_range_filtered (include/cor_amd.h): the ALLOWED rows whose score is at least a per-query floor,
and how many.

score(b, g) is range_refs.chain_scores (the fmaf chain over the operands the GPU multiplies). Allowed(b) is the rule of
cor_similarity_topk_filtered: a query label < 0 is unrestricted, mode "eq" allows the rows that carry the query's label, "ne" the rows
that do not. In(b) = { g in Allowed(b) : score(b, g) >= thr[b] } by the IEEE comparison, count[b] = |In(b)|, and the lists hold the
first k members by a stable sort on (score desc, index asc), indices g + g_offset, followed by the (-inf, -1) tail."""
import numpy as np
import torch

from tests import range_refs as R


def _np(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def allow_mask(row_labels, query_labels, mode: str) -> np.ndarray:
    """bool [Bq, Ng]: row g is allowed for query b."""
    rl, ql = _np(row_labels).astype(np.int64), _np(query_labels).astype(np.int64)
    same = rl[None, :] == ql[:, None]
    return (ql < 0)[:, None] | (same if mode == "eq" else ~same)


def range_from_scores(S: np.ndarray, allow: np.ndarray, thr, k: int, g_offset: int = 0):
    """(scores f32 [Bq,k], idx i64 [Bq,k], count i32 [Bq]) of the definition, from a full score matrix S f32 [Bq, Ng] and the mask."""
    S = np.asarray(S, dtype=np.float32)
    Bq, Ng = S.shape
    t = R.floors(thr, Bq)
    with np.errstate(invalid="ignore"):
        member = allow & (S >= t[:, None])                         # IEEE: anything >= NaN is false
    count = member.sum(axis=1).astype(np.int32)
    out_s = np.full((Bq, k), -np.inf, dtype=np.float32)
    out_i = np.full((Bq, k), -1, dtype=np.int64)
    for b in range(Bq):
        g = np.nonzero(member[b])[0]                               # index asc
        order = np.argsort(-S[b, g], kind="stable")[:k]            # score desc, ties keep the index order
        n = order.shape[0]
        out_s[b, :n] = S[b, g[order]]
        out_i[b, :n] = g[order] + g_offset
    return out_s, out_i, count


def similarity_range_filtered(Q: torch.Tensor, G: torch.Tensor, thr, k: int, row_labels, query_labels, mode: str = "eq", g_offset: int = 0):
    """The restatement on CPU tensors: (scores, idx, count) as numpy arrays."""
    return range_from_scores(R.chain_scores(Q, G), allow_mask(row_labels, query_labels, mode), thr, k, g_offset)


def allowed_sorted(S: np.ndarray, allow: np.ndarray) -> np.ndarray:
    """Every query's allowed scores sorted descending, f32 [Bq, Ng]; the disallowed rows' places at the end hold -inf."""
    return -np.sort(-np.where(allow, np.asarray(S, dtype=np.float32), np.float32(-np.inf)), axis=1)

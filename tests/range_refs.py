"""NumPy restatement of cor_similarity_range (include/cor_amd.h): the rows whose score is at least a per-query floor, and how many.

score(b, g) is the fp32 fmaf-chain score of cor_similarity_topk (oracle.retrieval.scores_fma_chain, oracle/c/sim_chain.c) over the
operands the GPU multiplies: for a 16-bit gallery the query rounded to the gallery dtype and the rows widened exactly. From the full
score matrix: In(b) = { g : score(b, g) >= thr[b] } by the IEEE comparison (a NaN floor: empty; -inf: every row; +0.0 and -0.0 one
floor), count[b] = |In(b)|, and the lists hold the first k members by a stable sort on (score desc, index asc), indices g + g_offset,
followed by the (-inf, -1) tail."""
import numpy as np
import torch

from oracle import retrieval as oret


def chain_scores(Q: torch.Tensor, G: torch.Tensor) -> np.ndarray:
    """The chain score matrix f32 [Bq, Ng] of fp32 queries Q against a gallery G of dtype fp32 / bf16 / fp16 (CPU tensors)."""
    Qr = Q.float() if G.dtype == torch.float32 else Q.to(G.dtype).float()
    return oret.scores_fma_chain(Qr.numpy(), G.float().numpy())


def floors(thr, Bq: int) -> np.ndarray:
    """A scalar or a vector of floors -> f32 [Bq]."""
    if isinstance(thr, torch.Tensor):
        thr = thr.detach().cpu().numpy()
    t = np.asarray(thr, dtype=np.float32)
    return np.full((Bq,), t, dtype=np.float32) if t.ndim == 0 else t.reshape(Bq)


def range_from_scores(S: np.ndarray, thr, k: int, g_offset: int = 0):
    """(scores f32 [Bq,k], idx i64 [Bq,k], count i32 [Bq]) of the definition, from a full score matrix S f32 [Bq, Ng]."""
    S = np.asarray(S, dtype=np.float32)
    Bq, Ng = S.shape
    t = floors(thr, Bq)
    with np.errstate(invalid="ignore"):
        member = S >= t[:, None]                                   # IEEE: anything >= NaN is false
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


def similarity_range(Q: torch.Tensor, G: torch.Tensor, thr, k: int, g_offset: int = 0):
    """The restatement on CPU tensors: (scores, idx, count) as numpy arrays."""
    return range_from_scores(chain_scores(Q, G), thr, k, g_offset)


def merge_lists(parts, k: int):
    """Per-segment (scores, idx, count) results -> the set's: the k best entries by (score desc, index asc), the counts added."""
    s = np.concatenate([p[0] for p in parts], axis=1)
    i = np.concatenate([p[1] for p in parts], axis=1)
    out_s = np.full((s.shape[0], k), -np.inf, dtype=np.float32)
    out_i = np.full((s.shape[0], k), -1, dtype=np.int64)
    for b in range(s.shape[0]):
        live = np.nonzero(i[b] >= 0)[0]
        live = live[np.argsort(i[b, live], kind="stable")]
        order = live[np.argsort(-s[b, live], kind="stable")][:k]
        out_s[b, :order.shape[0]] = s[b, order]
        out_i[b, :order.shape[0]] = i[b, order]
    return out_s, out_i, sum(p[2].astype(np.int64) for p in parts).astype(np.int32)

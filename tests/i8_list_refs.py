"""CPU restatements of the list stages over int8 galleries (include/cor_amd.h, "Int8-only galleries"), in NumPy / torch on the CPU. They
never call the code under test. Every floating-point step is one float32 NumPy operation, i.e. one separately rounded fp32 operation.

    ref_dequantize(q, scale, dtype)               -> torch CPU tensor [n,C]: float32(q) * scale[row], then (16-bit) rounded again by torch
    RefRescore(Q, gq, gscale, cand, offset).top(k) -> (scores f32, idx i64, pos i32) [Bq,k]: cor_rescore_topk_i8
    ref_expand_sq(Q, qw, segments, ...)           -> f32 [Bq,C]: cor_expand_queries_sq; a segment is (rows, offset) with float rows (torch
                                                     CPU tensor of any gallery dtype) or (q int8, scale f32, offset)

The quantiser and the int8 score come from tests/i8_refs.py, the summation of the expansion from tests/test_cpu_expand.ref_expand, which
takes the stored values already widened: for an int8 row that widening is ref_dequantize, the one added line of the definition."""
import numpy as np
import torch

from tests.i8_refs import F, ref_scores
from tests.test_cpu_expand import ref_expand


def _np(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def ref_dequantize(q, scale, dtype=torch.float32):
    q, scale = _np(q), _np(scale)
    assert q.dtype == np.int8 and scale.dtype == F
    x = (q.astype(F) * scale[:, None]).astype(F)                      # ONE rounded fp32 multiply
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype)        # 16-bit: the rounded product rounded again, nearest even


class RefRescore:
    """The definition for one (queries, int8 shard, candidate lists, offset): ranked once, cut to any k."""

    def __init__(self, Q, gq, gscale, cand, g_offset=0):
        gq, gscale, c = _np(gq), _np(gscale), _np(cand)
        S = ref_scores(Q, gq, gscale)[0]                              # [Bq,Ng]: ((float)d * qscale[b]) * gscale[g]
        Bq, Ng = c.shape[0], gq.shape[0]
        self.lists = []
        for b in range(Bq):
            ids = [int(v) for v in c[b]]                              # Python integers: no wrap-around in the range test
            seen, keep = set(), []
            for j, v in enumerate(ids):
                if g_offset <= v < g_offset + Ng and v not in seen:   # PRESENT: in range, first occurrence
                    seen.add(v)
                    keep.append(j)
            pj = np.asarray(keep, dtype=np.int64)
            pid = np.asarray([ids[j] for j in keep], dtype=np.int64)
            sc = S[b, pid - g_offset] if len(keep) else np.zeros(0, F)
            order = np.lexsort((pid, -sc.astype(np.float64)))         # score desc (-0.0 ties +0.0), then id asc
            self.lists.append((sc[order], pid[order], pj[order]))

    def top(self, k):
        Bq = len(self.lists)
        s, i, p = np.full((Bq, k), -np.inf, F), np.full((Bq, k), -1, np.int64), np.full((Bq, k), -1, np.int32)
        for b, (ls, li, lp) in enumerate(self.lists):
            n = min(k, ls.shape[0])
            s[b, :n], i[b, :n], p[b, :n] = ls[:n], li[:n], lp[:n]
        return torch.from_numpy(s), torch.from_numpy(i), torch.from_numpy(p)


def widened(segments):
    """[(rows float tensor, offset) | (q int8, scale, offset)] -> [(f32 ndarray of the values the kernel sums, offset)]"""
    out = []
    for seg in segments:
        if len(seg) == 3:
            out.append((ref_dequantize(seg[0], seg[1]).numpy(), int(seg[2])))
        else:
            out.append((seg[0].detach().cpu().float().numpy(), int(seg[1])))
    return out


def ref_expand_sq(Q, query_weight, segments, scores, idx, m, alpha, normalize):
    return ref_expand(None if Q is None else _np(Q), query_weight, widened(segments), _np(scores), _np(idx), m, alpha, normalize)

"""The CPU restatement of cor_fuse_lists' definition (include/cor_amd.h), which tests/test_gpu_fuse.py compares the kernel with bit for bit
and tests/test_cpu_fuse.py checks against an independent float64 formulation. Explicit per-query loops and np.float32 scalar operations
alone, each in the stated order: a NumPy float32 operation is one correctly rounded IEEE operation, which is what the kernel is held to."""
import numpy as np

F = np.float32


def is_finite_bits(s):
    """Exponent bits not all ones."""
    return (int(np.asarray(s, F).view(np.uint32)) & 0x7F800000) != 0x7F800000


def held_entries(scores, idx, b):
    """Per list p of query b: {id: position} of its VALID entries: idx >= 0, a finite score, the lowest such position of the id."""
    held = []
    for p in range(scores.shape[0]):
        h = {}
        for e in range(scores.shape[2]):
            i = int(idx[p, b, e])
            if i >= 0 and is_finite_bits(scores[p, b, e]) and i not in h:
                h[i] = e
        held.append(h)
    return held


def list_stats(scores, held, b):
    """Per list: (mn, mx) over its valid entries with -0.0 counted as +0.0, or None for a list without one."""
    out = []
    for p, h in enumerate(held):
        vals = [scores[p, b, e] + F(0) if scores[p, b, e] == 0 else scores[p, b, e] for e in h.values()]   # (-0.0 + 0.0 = +0.0)
        out.append((min(vals), max(vals)) if vals else None)
    return out


def contribution(s, e, w, st, mode, rrf_c, normalize):
    """c_p of a list that holds the id: its valid entry has score s at position e."""
    if mode == "rrf":
        return w / (rrf_c + F(e + 1))
    v = s
    if normalize == "minmax":
        mn, mx = st
        v = F(1) if mx == mn else (s - mn) / (mx - mn)
    return w * v


def ref_fuse(scores, idx, weights, mode, rrf_c, normalize, missing, k):
    """scores f32 [P,Bq,kin], idx i64 [P,Bq,kin], weights P floats, mode "rrf" / "sum" / "max", normalize "none" / "minmax", missing "zero" /
    "floor" -> (scores f32 [Bq,k], idx i64 [Bq,k], count i32 [Bq,k])."""
    scores, idx = np.ascontiguousarray(scores, F), np.ascontiguousarray(idx, np.int64)
    P, Bq, kin = scores.shape
    w = [F(x) for x in weights]
    rrf_c = F(rrf_c)
    out_s, out_i, out_c = np.full((Bq, k), -np.inf, F), np.full((Bq, k), -1, np.int64), np.full((Bq, k), -1, np.int32)
    with np.errstate(all="ignore"):
        for b in range(Bq):
            held = held_entries(scores, idx, b)
            stats = list_stats(scores, held, b)
            fused = {}
            for i in sorted(set().union(*held)):
                acc, cnt = F(0), 0
                for p in range(P):
                    if not held[p]:
                        continue                                       # a list with no valid entry contributes nothing, in any mode
                    if i in held[p]:
                        e = held[p][i]
                        c = contribution(scores[p, b, e], e, w[p], stats[p], mode, rrf_c, normalize)
                        if mode == "max":
                            if cnt == 0 or c > acc:
                                acc = c
                        else:
                            acc = acc + c
                        cnt += 1
                    elif missing == "floor":
                        f = F(0) if normalize == "minmax" else stats[p][0]
                        acc = acc + w[p] * f
                fused[i] = (F(acc), cnt)
            ranked = sorted(fused, key=lambda i: (-float(fused[i][0]), i))   # -0.0 == +0.0: the id decides
            for r, i in enumerate(ranked[:k]):
                out_s[b, r], out_i[b, r], out_c[b, r] = fused[i][0], i, fused[i][1]
    return out_s, out_i, out_c

"""CPU restatement of cor_rerank_diffusion (include/cor_amd.h, "Diffusion re-ranking"), in NumPy. It never calls the code under test.

    ref_diffusion(scores, idx, segs, k, kd=8, kq=None, gamma=3, alpha=0.9, iters=20) -> (scores f32, idx i64, pos i32) [Bq,k]
        scores f32 / idx i64 [Bq,kin]; segs [(rows f32 ndarray [n,C], offset)]: the row VALUES, already widened (tests/i8_list_refs.widened
        turns (rows, offset) / (q int8, scale, offset) segments into these); kq None = every present entry.
    diffusion_graph(X, rows, kd, gamma) -> (a [n,n], N, M): the affinities, the neighbour lists and the mutual lists of one query.

Explicit loops in the order the definition states, float32 throughout: every * + - / and sqrt is one NumPy float32 operation, i.e. one
separately rounded fp32 operation. The pair similarities are the fmaf chain of oracle/c/sim_chain.c (tests/diversify_refs.chain_pairs,
both triangles computed, so the symmetry is observed and not assumed). NumPy has no fmaf, so the iteration's g = fmaf(S, f, g) over M(p)
is walked by that same C chain: the t-th member's (S, f) sits in the column the chain visits t-th, the other columns hold S = +0 beside
a finite f >= +0, and fmaf(+0, f, g) == g for the g >= +0 that occur. The neighbour selection is a Python sort by (-a, p'), the mutual test a list membership,
the ranking a Python sort by (-float(f), id, position), where -0.0 == 0.0 so that the id decides."""
import numpy as np

from tests.diversify_refs import chain_pairs

F = np.float32
CHAIN_ORDER = [8 * c + h + i for c in range(4) for i in range(4) for h in (0, 4)]   # the column the chain visits t-th, 32 columns


def pw(v, gamma):
    v = np.asarray(v, dtype=F)
    w = v.copy()
    for _ in range(int(gamma) - 1):
        w = w * v
    assert w.dtype == F
    return np.where(v > 0, w, F(0)).astype(F)


def diffusion_graph(X, rows, kd, gamma):
    n = len(rows)
    qi, gi = np.repeat(np.arange(n), n), np.tile(np.arange(n), n)
    rows = np.asarray(rows, dtype=np.int64)
    a = pw(chain_pairs(X, rows[qi], rows[gi]), gamma).reshape(n, n) if n else np.zeros((0, 0), F)
    for p in range(n):
        a[p, p] = F(0)
    N = [sorted((q for q in range(n) if q != p and a[p, q] > 0), key=lambda q: (-float(a[p, q]), q))[:kd] for p in range(n)]
    M = [[q for q in N[p] if p in N[q]] for p in range(n)]
    return a, N, M


def _fma_rows(S, Fv):
    """g[p] = fmaf chain over row p of S and Fv (both [n,32], members in list order) starting from +0."""
    n = S.shape[0]
    A, B = np.zeros((n, 32), F), np.zeros((n, 32), F)
    A[:, CHAIN_ORDER], B[:, CHAIN_ORDER] = S, Fv
    X = np.ascontiguousarray(np.concatenate([A, B]))
    return chain_pairs(X, np.arange(n), np.arange(n, 2 * n))


def ref_diffusion(scores, idx, segs, k, kd=8, kq=None, gamma=3, alpha=0.9, iters=20):
    scores, idx = np.asarray(scores), np.asarray(idx)
    assert scores.dtype == F and idx.dtype == np.int64 and 1 <= kd <= 32
    Bq, kin = idx.shape
    live = [(np.ascontiguousarray(r, dtype=F), int(o)) for r, o in segs if r.shape[0]]
    X = np.ascontiguousarray(np.concatenate([r for r, _ in live])) if live else np.zeros((0, 16), F)
    base = np.cumsum([0] + [r.shape[0] for r, _ in live])
    alpha = F(alpha)
    out_s, out_i, out_p = np.full((Bq, k), -np.inf, F), np.full((Bq, k), -1, np.int64), np.full((Bq, k), -1, np.int32)
    for b in range(Bq):
        ids = [int(v) for v in idx[b]]                                # Python integers: no wrap-around in the range test
        pos, rows = [], []                                            # the present entries in list order: position, row of X
        for j, v in enumerate(ids):
            for s, (r, o) in enumerate(live):
                if o <= v < o + r.shape[0]:
                    pos.append(j)
                    rows.append(int(base[s]) + (v - o))
        n = len(pos)
        if n == 0:
            continue
        a, N, M = diffusion_graph(X, rows, kd, gamma)
        d = np.zeros(n, F)
        for p in range(n):
            for q in M[p]:
                d[p] = d[p] + a[p, q]
        r = np.zeros(n, F)
        for p in range(n):
            if d[p] > 0:
                r[p] = F(1.0) / np.sqrt(d[p])
        assert d.dtype == F and r.dtype == F
        S = np.zeros((n, 32), F)
        nb = np.zeros((n, 32), np.int64)
        for p in range(n):
            for t, q in enumerate(M[p]):
                S[p, t] = a[p, q] * (r[p] * r[q])
                nb[p, t] = q
        y = np.zeros(n, F)
        for p in range(n):
            if kq is None or p < kq:
                y[p] = pw(scores[b, pos[p]], gamma)                   # a missing entry's score is never read
        f = y.copy()
        keep = (F(1.0) - alpha) * y
        for _ in range(iters):
            g = _fma_rows(S, f[nb])                                   # columns past |M(p)|: S = +0 (and f of entry 0), fmaf(+0, x, g) == g
            f = (alpha * g) + keep
            assert f.dtype == F
        order = sorted(range(n), key=lambda p: (-float(f[p]), ids[pos[p]], pos[p]))[:k]
        for t, p in enumerate(order):
            out_s[b, t], out_i[b, t], out_p[b, t] = f[p], ids[pos[p]], pos[p]
    return out_s, out_i, out_p

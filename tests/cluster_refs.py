"""CPU restatements of cor_kmeans_seed, cor_kmeans_update (include/cor_amd.h, "Clustering of a gallery") and of the k-means loop of
cor_amd.retrieval (.cluster), in NumPy. They never call the code under test.

    ref_seed(segs, K, first_id=None)                      -> (ids i64 [K], centroids f32 [K,C])
    ref_update(segs, assigns, K, scores=None, prev=None)  -> (centroids f32 [K,C], counts i32 [K], score_sums f32 [K] or None)
    ref_assign(cent, X)                                   -> (cluster i32 [n], score f32 [n]): the search of the rows X in the centres, k = 1
    ref_cluster(segs, K, iters=20, init="maxmin", first_id=None) -> dict(centroids, assign [per segment], counts, objective, iters, converged)
    planted(...)                                          -> the purpose fixture of the issue

segs [(rows f32 ndarray [n,C], offset)]: the row VALUES, already widened (tests/i8_list_refs.widened turns (rows, offset) / (q int8, scale,
offset) segments into these); assigns / scores: one array per segment. Every floating-point step is one float32 NumPy operation, i.e. one
separately rounded fp32 operation, in the order the definition states. The similarities are the fmaf chain of oracle/c/sim_chain.c
(oracle.retrieval.scores_fma_chain). A running sum x_0, x_1, .. from +0 is np.cumsum over [+0, x_0, x_1, ..] in float32, which adds one
element at a time in that order (sequential_sum below; tests/test_cpu_cluster.py checks it against the explicit loop)."""
import math

import numpy as np

F = np.float32
CHUNK = 256


def _chain(Q, G):
    from oracle import retrieval as oret
    return oret.scores_fma_chain(np.ascontiguousarray(Q, dtype=F), np.ascontiguousarray(G, dtype=F))


def by_id(segs, *per_segment):
    """All rows in ascending global id: (ids i64 [n], X f32 [n,C], then every per-segment list concatenated in the same order)."""
    live = [n for n, (r, _) in enumerate(segs) if r.shape[0]]
    live.sort(key=lambda n: int(segs[n][1]))
    C = segs[0][0].shape[1] if segs else 16
    ids = np.concatenate([np.arange(segs[n][0].shape[0], dtype=np.int64) + int(segs[n][1]) for n in live]) if live else np.zeros(0, np.int64)
    X = np.ascontiguousarray(np.concatenate([segs[n][0] for n in live]), dtype=F) if live else np.zeros((0, C), F)
    assert np.all(np.diff(ids) > 0), "the segments' id ranges overlap"
    return (ids, X) + tuple(None if p is None else (np.concatenate([np.asarray(p[n]) for n in live]) if live else np.zeros(0)) for p in per_segment)


def sequential_sum(x):
    """+0, then + x[0], + x[1], ... along axis 0, one rounded float32 addition each."""
    x = np.asarray(x, dtype=F)
    return np.cumsum(np.concatenate([np.zeros((1,) + x.shape[1:], F), x]), axis=0, dtype=F)[-1]


def norm_tree(v):
    """Step 3 of cor_expand_queries: squares into 256 slots, the stride-halving tree, d = max(sqrt(s[0]), 1e-12), v / d."""
    s = np.zeros(256, F)
    s[:v.shape[0]] = v * v
    h = 128
    while h >= 1:
        s[:h] = s[:h] + s[h:2 * h]
        h //= 2
    out = v / max(np.sqrt(s[0]), F(1e-12))
    assert out.dtype == F
    return out


def ref_seed(segs, K, first_id=None):
    ids, X = by_id(segs)
    n = ids.shape[0]
    assert 1 <= K <= n
    first_id = int(ids[0]) if first_id is None else int(first_id)
    cur = int(np.flatnonzero(ids == first_id)[0])
    best = np.full(n, -np.inf, F)
    chosen = np.zeros(n, bool)
    out_ids, cent = np.zeros(K, np.int64), np.zeros((K, X.shape[1]), F)
    for t in range(K):
        out_ids[t], cent[t] = ids[cur], X[cur]
        s = _chain(X[cur:cur + 1], X)[0]
        raise_ = s > best
        best[raise_] = s[raise_]
        chosen[cur] = True
        if t + 1 < K:
            cand = np.flatnonzero(~chosen)                            # ascending id
            b = best[cand]
            cur = int(cand[np.flatnonzero(b == b.min())[0]])          # IEEE: -0.0 == +0.0; the first = the smallest id
    return out_ids, cent


def ref_update(segs, assigns, K, scores=None, prev=None):
    ids, X, a, sc = by_id(segs, assigns, scores)
    a = a.astype(np.int64)
    C = X.shape[1]
    cent, counts = np.zeros((K, C), F), np.zeros(K, np.int32)
    sums = None if scores is None else np.zeros(K, F)
    for c in range(K):
        mem = np.flatnonzero(a == c)                                  # ascending id
        counts[c] = mem.shape[0]
        if mem.shape[0] == 0:
            if prev is not None:
                cent[c] = prev[c]
            continue
        parts = [sequential_sum(X[mem[j:j + CHUNK]]) for j in range(0, mem.shape[0], CHUNK)]
        cent[c] = norm_tree(sequential_sum(np.stack(parts)))
        if scores is not None:
            sums[c] = sequential_sum(np.stack([sequential_sum(sc[mem[j:j + CHUNK]].astype(F)) for j in range(0, mem.shape[0], CHUNK)]))
    return cent, counts, sums


def ref_assign(cent, X):
    S = _chain(X, cent)                                               # [n,K]
    idx = np.argmax(S, axis=1)                                        # the first maximum: (score desc, index asc)
    return idx.astype(np.int32), S[np.arange(X.shape[0]), idx]


def ref_cluster(segs, K, iters=20, init="maxmin", first_id=None):
    live = sorted((s for s in segs if s[0].shape[0]), key=lambda s: int(s[1]))
    n = sum(r.shape[0] for r, _ in live)
    cent = ref_seed(live, K, first_id)[1] if isinstance(init, str) else np.ascontiguousarray(init, dtype=F).copy()
    assign = [np.full(r.shape[0], -1, np.int32) for r, _ in live]
    objective, converged, passes, counts = [], False, 0, None
    while passes < iters and not converged:
        pairs = [ref_assign(cent, r) for r, _ in live]
        new, score = [p[0] for p in pairs], [p[1] for p in pairs]
        changed = sum(int((x != y).sum()) for x, y in zip(new, assign))
        cent, counts, sums = ref_update(live, new, K, scores=score, prev=cent)
        objective.append(math.fsum(float(v) for v in sums) / n)
        converged = changed == 0
        assign = new
        passes += 1
    return dict(centroids=cent, assign=assign, counts=counts, objective=objective, iters=passes, converged=converged)


def planted(n=3000, modes=30, C=64, noise=0.05, seed=1234, skew=False):
    """The purpose fixture: `modes` planted unit directions from default_rng(seed), row i from direction i mod modes (skew: a direction
    drawn with probability proportional to 1 / (1 + mode)) plus noise * N(0, 1) per coordinate, normalised. -> (rows f32 [n,C], mode [n],
    directions f32 [modes,C])"""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((modes, C))
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    if skew:
        w = 1.0 / (1.0 + np.arange(modes))
        mode = rng.choice(modes, size=n, p=w / w.sum())
    else:
        mode = np.arange(n) % modes
    x = d[mode] + noise * rng.standard_normal((n, C))
    x = x / np.linalg.norm(x, axis=1, keepdims=True)
    return np.ascontiguousarray(x, dtype=F), mode, np.ascontiguousarray(d, dtype=F)


def purity(assign, mode, K):
    """The share of rows whose planted mode is the most frequent one of their cluster."""
    hit = 0
    for c in range(K):
        m = mode[assign == c]
        if m.shape[0]:
            hit += np.bincount(m).max()
    return hit / assign.shape[0]

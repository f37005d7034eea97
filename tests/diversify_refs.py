"""CPU restatement of cor_diversify_mmr (include/cor_amd.h, "Result diversification"), in NumPy. It never calls the code under test.

    ref_diversify(scores, idx, segs, k, lam, max_sim) -> (scores f32, idx i64, pos i32, value f32) [Bq,k]
        scores f32 / idx i64 [Bq,kin]; segs [(rows f32 ndarray [n,C], offset)]: the row VALUES, already widened (tests/i8_list_refs.widened
        turns (rows, offset) / (q int8, scale, offset) segments into these); max_sim None = +inf.

The pair similarities are the fmaf chain of oracle/c/sim_chain.c (sim_chain_pairs of oracle.retrieval._chain_lib(), loaded read-only, the
rows passed as both operands); the mixing is elementwise np.float32 operations in the stated order, i.e. one separately rounded fp32
operation each; the winner is a Python min over (-float(f), id, position), where -0.0 == 0.0 so that the id decides."""
import ctypes

import numpy as np

F = np.float32


def chain_pairs(X, qi, gi):
    """out[p] = chain(X[qi[p]], X[gi[p]]), bit for bit the GPU's similarity of two rows."""
    from oracle import retrieval as oret
    lib = oret._chain_lib()
    fp, ip = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_longlong)
    lib.sim_chain_pairs.argtypes = [fp, fp, ip, ip, ctypes.c_longlong, ctypes.c_int, fp]
    lib.sim_chain_pairs.restype = None
    qi, gi = np.ascontiguousarray(qi, dtype=np.int64), np.ascontiguousarray(gi, dtype=np.int64)
    out = np.empty(qi.shape[0], dtype=F)
    if qi.shape[0]:
        lib.sim_chain_pairs(X.ctypes.data_as(fp), X.ctypes.data_as(fp), qi.ctypes.data_as(ip), gi.ctypes.data_as(ip), qi.shape[0], X.shape[1],
                            out.ctypes.data_as(fp))
    return out


def ref_diversify(scores, idx, segs, k, lam, max_sim=None):
    scores, idx = np.asarray(scores), np.asarray(idx)
    assert scores.dtype == F and idx.dtype == np.int64
    Bq, kin = idx.shape
    live = [(np.ascontiguousarray(r, dtype=F), int(o)) for r, o in segs if r.shape[0]]
    X = np.ascontiguousarray(np.concatenate([r for r, _ in live])) if live else np.zeros((0, 16), F)
    base = np.cumsum([0] + [r.shape[0] for r, _ in live])
    lam, ms = F(lam), F(np.inf if max_sim is None else max_sim)
    out_s, out_i = np.full((Bq, k), -np.inf, F), np.full((Bq, k), -1, np.int64)
    out_p, out_v = np.full((Bq, k), -1, np.int32), np.full((Bq, k), -np.inf, F)
    for b in range(Bq):
        ids = [int(v) for v in idx[b]]                                # Python integers: no wrap-around in the range test
        row = {}                                                      # position -> row of X, present entries only
        for j, v in enumerate(ids):
            for n, (r, o) in enumerate(live):
                if o <= v < o + r.shape[0]:
                    row[j] = int(base[n]) + (v - o)
        s = np.zeros(kin, F)
        for j in row:
            s[j] = scores[b, j]                                       # a missing entry's score is never read
        m = np.zeros(kin, F)
        alive = sorted(row)
        for t in range(k):
            if not alive:
                break
            a = np.asarray(alive)
            f = (lam * s[a]) - ((F(1) - lam) * m[a])
            assert f.dtype == F
            fj = dict(zip(alive, f))
            w = min(alive, key=lambda j: (-float(fj[j]), ids[j], j))
            out_s[b, t], out_i[b, t], out_p[b, t], out_v[b, t] = scores[b, w], ids[w], w, fj[w]
            alive.remove(w)
            if not alive or t + 1 == k:
                continue
            a = np.asarray(alive)
            v = chain_pairs(X, [row[j] for j in alive], [row[w]] * len(alive))
            m[a] = np.where(v > m[a], v, m[a])
            alive = [j for j, vj in zip(alive, v) if not vj >= ms]
    return out_s, out_i, out_p, out_v

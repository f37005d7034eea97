"""CPU restatement of the int8 gallery search (include/cor_amd.h, "Int8 galleries"), in NumPy / torch on the CPU. It never calls the code
under test. Every floating-point step is one float32 NumPy operation, i.e. one separately rounded fp32 operation.

    ref_quantize(X)                -> (q int8 [n,C], scale f32 [n])
    ref_scores(Q, q, scale)        -> (S f32 [Bq,Ng], qq, qscale): S = ((float)d * qscale[b]) * scale[g], d the exact integer dot product
    ref_topk(S, k, offset)         -> (scores f32 [Bq,k], idx i64 [Bq,k]) by (order-preserving key of the score bits desc, row asc)
    ref_search(Q, q, scale, k, offset) = ref_topk(ref_scores(...))

The integer products come from an fp32 matmul of the int8 values: every product and every partial sum is an integer of magnitude at most
127^2 * 256 < 2^24, so each is exact in fp32 whatever the order (test_cpu_topk_i8 checks it against Python integers)."""
import numpy as np
import torch

F = np.float32


def _f32(X):
    """float32 ndarray of a tensor / array in fp32, bf16 or fp16 (16-bit values widen exactly)"""
    if isinstance(X, torch.Tensor):
        return X.detach().cpu().to(torch.float32).numpy()
    return np.asarray(X).astype(F)


def ref_quantize(X):
    x = _f32(X)
    assert x.ndim == 2 and np.isfinite(x).all()
    amax = np.abs(x).max(axis=1).astype(F) if x.shape[1] else np.zeros(x.shape[0], F)
    nz = amax != 0
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = (F(127.0) / amax).astype(F)
        t = np.rint((x * inv[:, None]).astype(F)).astype(F)           # np.rint: half to even, as rintf
    t = np.where(nz[:, None], np.clip(t, F(-127.0), F(127.0)), F(0.0))
    q = t.astype(np.int32).astype(np.int8)
    scale = np.where(nz, (amax / F(127.0)).astype(F), F(0.0)).astype(F)
    return q, scale


def int_dots(qq, gq):
    """d int32 [Bq,Ng] = qq . gq^T, by an fp32 matmul of the int8 values (exact, see above)"""
    d = torch.from_numpy(qq.astype(F)) @ torch.from_numpy(gq.astype(F)).T
    return d.numpy().astype(np.int32)


def ref_scores(Q, gq, gscale):
    qq, qscale = ref_quantize(Q)
    d = int_dots(qq, np.asarray(gq))
    S = ((d.astype(F) * qscale[:, None]).astype(F) * np.asarray(gscale, F)[None, :]).astype(F)
    return S, qq, qscale


def f2key(S):
    """the order-preserving unsigned key of float32 bits: -0.0 below +0.0, as the kernels' f2key"""
    u = np.ascontiguousarray(S, F).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def ref_topk(S, k, offset=0):
    Bq, Ng = S.shape
    # one int64 per (query, row), all different: [key - 2^31 : 32 bits | 2^32 - 1 - row : 32 bits], largest first
    comp = ((f2key(S).astype(np.int64) - 2 ** 31) << 32) | (2 ** 32 - 1 - np.arange(Ng, dtype=np.int64))[None, :]
    kk = min(k, Ng)
    o = torch.topk(torch.from_numpy(comp), kk, dim=1, largest=True, sorted=True).indices.numpy()
    s, i = np.full((Bq, k), -np.inf, F), np.full((Bq, k), -1, np.int64)
    s[:, :kk], i[:, :kk] = np.take_along_axis(S, o, axis=1), o + offset
    return s, i


def ref_topk_slow(S, k, offset=0):
    """ref_topk spelled out with a lexsort per query (tiny shapes: the check of the composite key above)"""
    Bq, Ng = S.shape
    key = f2key(S).astype(np.int64)
    s, i = np.full((Bq, k), -np.inf, F), np.full((Bq, k), -1, np.int64)
    for b in range(Bq):
        o = np.lexsort((np.arange(Ng), -key[b]))[:k]
        s[b, :len(o)], i[b, :len(o)] = S[b, o], o + offset
    return s, i


def ref_search(Q, gq, gscale, k, offset=0):
    return ref_topk(ref_scores(Q, gq, gscale)[0], k, offset)

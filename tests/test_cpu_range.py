"""CPU side of the threshold (range) search, cor_similarity_range: the library's exports and argument checks (no device needed), the
Python front's validation, the workspace query swept over shard sizes, the restatement tests/range_refs.py against a float64
formulation and hand-checkable floors, and the purpose fixture: a score floor separates planted queries from random ones where
top-1 accepts all of them."""
import os
import re

import numpy as np
import pytest
import torch

from tests import range_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _proto_args(hdr, ret, name):
    proto = re.search(r"^" + ret + r"\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr, flags=re.M | re.S)
    assert proto, f"{name} is not declared in include/cor_amd.h"
    return len(proto.group(1).split(","))


def _unit(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def test_library_exports_the_range_symbols():
    from cor_amd import _native
    lib = _native.load()
    hdr = open(os.path.join(ROOT, "include", "cor_amd.h")).read()
    assert _proto_args(hdr, "long", "cor_range_workspace_bytes") == 3 == len(_native.SIGNATURES["cor_range_workspace_bytes"])
    assert _proto_args(hdr, "int", "cor_similarity_range") == 15 == len(_native.SIGNATURES["cor_similarity_range"])
    assert lib.cor_similarity_range.restype is _native._i and lib.cor_range_workspace_bytes.restype is _native._l
    assert _native.SIGNATURES["cor_similarity_range"][8] is _native._ll            # g_offset


def test_range_argument_errors_need_no_gpu():
    """Every argument check comes before any HIP call, in the order and with the codes of cor_similarity_topk."""
    from cor_amd import _native
    lib = _native.load()
    E, N = _native.EINVAL, _native.ENOSUPPORT
    buf = torch.zeros(4096, dtype=torch.uint8)
    p = (buf.data_ptr() + 255) & ~255                                              # 256-byte aligned, 3 KiB behind it

    def call(Q=p, G=p, dt=_native.F32, Bq=1, Ng=8, C=64, thr=p, k=4, off=0, out_s=p, out_i=p, out_c=p, ws=p, flags=0):
        return lib.cor_similarity_range(Q, G, dt, Bq, Ng, C, thr, k, off, out_s, out_i, out_c, ws, flags, None)

    assert call(Q=None) == E and call(G=None) == E and call(thr=None) == E and call(out_c=None) == E
    assert call(out_s=None) == E and call(out_i=None) == E and call(ws=None) == E
    assert call(Bq=0) == E and call(Ng=0) == E and call(k=0) == E and call(Bq=-1) == E and call(k=-5) == E
    assert call(k=257) == N and call(C=272) == N and call(C=40) == N and call(C=8) == N
    for flag in (_native.TOPK_FORCE_LISTS, _native.TOPK_FORCE_GLOBAL_THRESHOLD, _native.TOPK_WAVE_FINAL, 4, 1 << 20,
                 _native.TOPK_NO_FALLBACK | _native.TOPK_FORCE_LISTS):
        assert call(flags=flag) == N, flag
        assert call(flags=flag, k=40) == N, flag
    assert call(Q=p + 4) == E and call(G=p + 8) == E and call(ws=p + 16) == E
    assert call(dt=9) == N and call(dt=_native.BF16X3) == N                        # after every other check: no kernel for the dtype
    # the order of check_topk_call: null / counts before the shape, the shape and the flags before the alignment
    assert call(Q=None, k=257) == E and call(thr=None, k=257) == E and call(out_c=None, flags=1) == E
    assert call(Q=p + 4, k=257) == N and call(Q=p + 4, flags=1) == N and call(Ng=0, C=40) == E and call(Q=p + 4, dt=9) == E

    ws = lib.cor_range_workspace_bytes
    assert ws(0, 10, 1) == E and ws(1, 0, 1) == E and ws(1, 10, 0) == E and ws(1, 10, 257) == E


def test_range_workspace_covers_every_shard_size():
    """Positive for Ng from 1 to 2^31 - 1 at k = 1 and 256, and at least the wide top-k's workspace (whose plan it extends) at k >= 33."""
    from cor_amd import _native
    lib = _native.load()
    sizes = sorted({1, 2, 31, 32, 33, 63, 64, 65, 4095, 4096, 4097, 20000, 125000, 1_000_000, 2 ** 31 - 1}
                   | {2 ** e for e in range(1, 31)} | {2 ** e + 1 for e in range(1, 31)} | {3 * 2 ** e - 1 for e in range(1, 29)})
    for Ng in sizes:
        for Bq in (1, 33, 512, 513):
            for k in (1, 256):
                n = lib.cor_range_workspace_bytes(Bq, Ng, k)
                assert n > 0 and n % 256 == 0, (Bq, Ng, k, n)
            for k in (33, 100, 256):
                assert lib.cor_range_workspace_bytes(Bq, Ng, k) >= lib.cor_topk_workspace_bytes(Bq, Ng, k), (Bq, Ng, k)


def test_python_validation_and_no_cpu_path():
    from cor_amd import ops, retrieval
    Q, G = torch.zeros((2, 32)), torch.zeros((5, 32))
    for k in (0, 257, -1):
        with pytest.raises(ValueError):
            ops.similarity_range(Q, G, 0.5, k)
    with pytest.raises(ValueError):
        ops.similarity_range(Q, G, torch.zeros(3), 3)                              # one floor per query
    with pytest.raises(ValueError):
        ops.similarity_range(Q, G, torch.zeros((2, 1)), 3)
    with pytest.raises(ValueError):
        ops.similarity_range(Q, G, torch.zeros(2, dtype=torch.float64), 3)
    with pytest.raises(ValueError):
        ops.similarity_range(Q, G, torch.zeros(2, dtype=torch.int32), 3)
    with pytest.raises(ValueError):
        ops.similarity_range(Q, G, "0.5", 3)
    with pytest.raises(RuntimeError, match="GPU only"):                            # valid arguments on the CPU: no CPU path
        ops.similarity_range(Q, G, 0.5, 3)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.similarity_range(Q, G, torch.zeros(2), 3)
    sh = retrieval.GalleryShard.__new__(retrieval.GalleryShard)                     # the constructor refuses CPU tensors
    sh.rows, sh.offset, sh.labels, sh.groups = G, 0, None, None
    with pytest.raises(RuntimeError, match="GPU only"):
        sh.range_search(Q, 0.5, 3)
    with pytest.raises(ValueError):
        sh.range_search(Q, 0.5, 300)
    i8 = retrieval.QuantizedShard.__new__(retrieval.QuantizedShard)
    i8.rows, i8.scales, i8.offset, i8.labels, i8.groups = torch.zeros((5, 32), dtype=torch.int8), torch.zeros(5), 5, None, None
    with pytest.raises(ValueError, match="int8"):
        retrieval.GallerySet([sh, i8]).range_search(Q, 0.5, 3)
    assert not hasattr(i8, "range_search")
    # nothing to search: all-missing lists and zero counts, on the queries' device
    for empty in (retrieval.GallerySet(),):
        s, i, c = empty.range_search(Q, 0.5, 3)
        assert s.shape == (2, 3) and torch.isneginf(s).all() and (i == -1).all() and i.dtype == torch.int64
        assert c.dtype == torch.int32 and c.tolist() == [0, 0]
    with pytest.raises(ValueError):
        retrieval.GallerySet().range_search(Q, 0.5, 0)


@pytest.mark.parametrize("gdt", [torch.float32, torch.bfloat16, torch.float16])
def test_restatement_against_float64(gdt):
    """The chain counts may differ from a float64 evaluation only where a float64 score lies within 3.1e-5 of the floor (the bound
    oracle/retrieval.py states for unit vectors); the listed rows are members and come in (score desc, index asc) order."""
    rng = np.random.default_rng(11)
    C, Ng, Bq, k = 64, 4000, 24, 50
    G = torch.from_numpy(_unit(rng.standard_normal((Ng, C))).astype(F)).to(gdt)
    Q = torch.from_numpy(_unit(rng.standard_normal((Bq, C))).astype(F))
    thr = np.linspace(-0.05, 0.35, Bq).astype(F)
    s, i, c = R.similarity_range(Q, G, thr, k, g_offset=7)
    Qr = Q if gdt == torch.float32 else Q.to(gdt).float()
    S64 = Qr.double().numpy() @ G.double().numpy().T
    S32 = R.chain_scores(Q, G)
    assert np.abs(S32 - S64).max() < 3.1e-5
    m64 = S64 >= thr.astype(np.float64)[:, None]
    near = np.abs(S64 - thr.astype(np.float64)[:, None]) <= 3.1e-5
    m32 = S32 >= thr[:, None]
    assert not ((m32 != m64) & ~near).any()
    assert (np.abs(c.astype(np.int64) - m64.sum(1)) <= near.sum(1)).all()
    assert (c == m32.sum(1)).all() and c.min() < k < c.max()                       # both a tail and a cut list occur
    for b in range(Bq):
        n = min(int(c[b]), k)
        assert (i[b, n:] == -1).all() and np.isneginf(s[b, n:]).all()
        rows = i[b, :n] - 7
        assert (S32[b, rows] == s[b, :n]).all() and (s[b, :n] >= thr[b]).all()
        key = list(zip((-s[b, :n]).tolist(), rows.tolist()))
        assert key == sorted(key)
        if n == k < c[b]:                                                          # the k best members: nothing better was left out
            rest = np.setdiff1d(np.nonzero(m32[b])[0], rows)
            assert S32[b, rest].max() <= s[b, n - 1]


def test_hand_checkable_floors():
    # rows 0..5 against q = e0: scores 0.5, 0.25, 0.5, -1, 0, 0.25
    G = np.zeros((6, 8), dtype=F)
    G[:, 0] = [0.5, 0.25, 0.5, -1.0, 0.0, 0.25]
    Q = np.zeros((7, 8), dtype=F)
    Q[:, 0] = 1.0
    S = R.chain_scores(torch.from_numpy(Q), torch.from_numpy(G))
    assert S[0].tolist() == [0.5, 0.25, 0.5, -1.0, 0.0, 0.25]
    thr = np.array([np.nan, np.inf, -np.inf, 0.5, np.nextafter(F(0.5), F(1)), 0.25, -0.0], dtype=F)
    s, i, c = R.range_from_scores(S, thr, 4, g_offset=100)
    assert c.tolist() == [0, 0, 6, 2, 0, 4, 5]
    assert (i[0] == -1).all() and (i[1] == -1).all() and np.isneginf(s[:2]).all()                # NaN and +inf: the empty set
    assert i[2].tolist() == [100, 102, 101, 105] and s[2].tolist() == [0.5, 0.5, 0.25, 0.25]      # -inf: every row, the first k listed
    assert i[3].tolist() == [100, 102, -1, -1] and s[3, :2].tolist() == [0.5, 0.5]                # a floor equal to a tied pair's score
    assert (i[4] == -1).all()                                                                     # one ulp above it: nobody
    assert i[5].tolist() == [100, 102, 101, 105]
    assert i[6].tolist() == [100, 102, 101, 105]                                                  # -0.0: the row that scores +0.0 is in
    # all-zero rows: every score is +0.0, and +0.0 and -0.0 are one floor
    Z = np.zeros((2, 5), dtype=F)
    for z in (0.0, -0.0):
        s, i, c = R.range_from_scores(Z, F(z), 3)
        assert c.tolist() == [5, 5] and i.tolist() == [[0, 1, 2]] * 2 and (s == 0).all()
    s, i, c = R.range_from_scores(-Z, F(0.0), 3)                                                  # scores of -0.0 against a floor of +0.0
    assert c.tolist() == [5, 5]
    s, i, c = R.range_from_scores(Z, np.nextafter(F(0), F(1)), 3)
    assert c.tolist() == [0, 0] and (i == -1).all()
    # a scalar floor is the vector of that floor; k beyond the shard leaves the tail
    a, b = R.range_from_scores(S, F(0.25), 8), R.range_from_scores(S, np.full(7, 0.25, dtype=F), 8)
    assert all((x == y).all() for x, y in zip(a, b)) and a[1][0].tolist() == [0, 2, 1, 5, -1, -1, -1, -1]
    m = R.merge_lists([R.range_from_scores(S[:, :3], F(0.25), 3, 0), R.range_from_scores(S[:, 3:], F(0.25), 3, 3)], 3)
    assert m[1][0].tolist() == [0, 2, 1] and m[2].tolist() == [4] * 7


def test_purpose_a_floor_separates_planted_from_random_queries():
    """Open-set retrieval: 3 000 unit rows at C = 64; 300 queries are a planted row + 0.10 noise per channel, renormalised; 300 are
    random unit vectors. Top-1 accepts all 600. With a floor of 0.6 every planted query has exactly one member, the planted row, and no
    random query has any. The smallest planted score is 0.639 and the best score of any random query 0.542 (plain fp32, checked here),
    so the floor sits more than 0.03 from either: a thousand times the chain-vs-fp32 difference."""
    rng = np.random.default_rng(20261020)
    G = _unit(rng.standard_normal((3000, 64)))
    planted = rng.permutation(3000)[:300]
    Qp = _unit(G[planted] + 0.10 * rng.standard_normal((300, 64)))
    Qr = _unit(rng.standard_normal((300, 64)))
    G, Q = G.astype(F), np.concatenate([Qp, Qr]).astype(F)
    S = Q @ G.T                                                                    # plain fp32 scores
    assert (S[:300].argmax(1) == planted).all()
    lo, hi = float(S[np.arange(300), planted].min()), float(S[300:].max())
    assert abs(lo - 0.639) < 5e-4 and abs(hi - 0.542) < 5e-4, (lo, hi)
    assert lo - 0.6 > 0.03 and 0.6 - hi > 0.03
    S[np.arange(300), planted] = -1.0
    assert S[:300].max() < 0.6 - 0.03                                              # nobody else comes near the floor either
    assert np.isfinite(Q @ G.T).all() and ((Q @ G.T).max(1) > -1).all()            # top-1 alone accepts all 600
    s, i, c = R.similarity_range(torch.from_numpy(Q), torch.from_numpy(G), 0.6, 10)
    assert c[:300].tolist() == [1] * 300 and c[300:].tolist() == [0] * 300
    assert (i[:300, 0] == planted).all() and (i[:300, 1:] == -1).all() and (i[300:] == -1).all()
    assert np.abs(R.chain_scores(torch.from_numpy(Q), torch.from_numpy(G)) - Q @ G.T).max() < 3.1e-5

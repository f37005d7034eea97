"""CPU side of the int8 gallery search: the library's exports and argument checks (no device needed), the Python front's validation, the
restatement tests/i8_refs.py against plain Python integers and floats rounded step by step, the quantiser's edge rows, and the recall of
the int8 coarse stage + fp32 re-scoring on a seeded gallery."""
import os
import re

import numpy as np
import pytest
import torch

from tests import i8_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _proto_args(hdr, ret, name):
    proto = re.search(r"^" + ret + r"\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr, flags=re.M | re.S)
    assert proto, f"{name} is not declared in include/cor_amd.h"
    return len(proto.group(1).split(","))


def test_library_exports_the_i8_symbols():
    from cor_amd import _native
    lib = _native.load()
    hdr = open(os.path.join(ROOT, "include", "cor_amd.h")).read()
    assert _proto_args(hdr, "int", "cor_quantize_rows_i8") == 7 == len(_native.SIGNATURES["cor_quantize_rows_i8"])
    assert _proto_args(hdr, "long", "cor_topk_i8_workspace_bytes") == 3 == len(_native.SIGNATURES["cor_topk_i8_workspace_bytes"])
    assert _proto_args(hdr, "int", "cor_similarity_topk_i8") == 13 == len(_native.SIGNATURES["cor_similarity_topk_i8"])
    assert lib.cor_quantize_rows_i8.restype is _native._i and lib.cor_similarity_topk_i8.restype is _native._i
    assert lib.cor_topk_i8_workspace_bytes.restype is _native._l
    assert _native.SIGNATURES["cor_similarity_topk_i8"][7] is _native._ll          # g_offset


def test_i8_argument_errors_need_no_gpu():
    """Every argument check comes before any HIP call, in the order and with the codes of cor_similarity_topk."""
    from cor_amd import _native
    lib = _native.load()
    E, N = _native.EINVAL, _native.ENOSUPPORT
    buf = torch.zeros(4096, dtype=torch.uint8)
    p = (buf.data_ptr() + 255) & ~255                                              # 256-byte aligned, 3 KiB behind it

    def call(Q=p, G=p, gs=p, Bq=1, Ng=8, C=64, k=4, off=0, out_s=p, out_i=p, ws=p, flags=0):
        return lib.cor_similarity_topk_i8(Q, G, gs, Bq, Ng, C, k, off, out_s, out_i, ws, flags, None)

    assert call(Q=None) == E and call(G=None) == E and call(gs=None) == E and call(out_s=None) == E and call(out_i=None) == E
    assert call(ws=None) == E and call(Bq=0) == E and call(Ng=0) == E and call(k=0) == E and call(Bq=-1) == E and call(k=-5) == E
    assert call(k=257) == N and call(C=272) == N and call(C=40) == N and call(C=8) == N
    for flag in (_native.TOPK_FORCE_LISTS, _native.TOPK_FORCE_GLOBAL_THRESHOLD, _native.TOPK_WAVE_FINAL, 4, 1 << 20,
                 _native.TOPK_NO_FALLBACK | _native.TOPK_FORCE_LISTS):
        assert call(flags=flag) == N, flag
    assert call(Q=p + 4) == E and call(G=p + 8) == E and call(gs=p + 4) == E and call(ws=p + 16) == E
    # the order of check_topk_call: null / counts before the shape, the shape and the flags before the alignment
    assert call(Q=None, k=257) == E and call(Q=p + 4, k=257) == N and call(Q=p + 4, flags=1) == N and call(Ng=0, C=40) == E

    def quant(X=p, dt=_native.F32, n=4, C=64, q=p, sc=p):
        return lib.cor_quantize_rows_i8(X, dt, n, C, q, sc, None)

    assert quant(X=None) == E and quant(q=None) == E and quant(sc=None) == E and quant(n=-1) == E and quant(C=0) == E
    assert quant(C=272) == N and quant(C=24) == N and quant(dt=_native.BF16X3) == N and quant(dt=9) == N
    assert quant(X=p + 4) == E and quant(q=p + 8) == E and quant(sc=p + 2) == E
    assert quant(n=0) == 0 and quant(n=0, dt=_native.F16, C=256) == 0              # nothing to do: no launch

    ws = lib.cor_topk_i8_workspace_bytes
    assert ws(0, 10, 1) == E and ws(1, 0, 1) == E and ws(1, 10, 0) == E and ws(1, 10, 257) == E
    for Bq, Ng, k in ((1, 1, 1), (7, 17, 256), (512, 1_000_000, 10), (512, 1_000_000, 100), (32, 100_000, 100), (257, 70001, 33)):
        n = ws(Bq, Ng, k)
        assert n > 0 and n % 256 == 0 and n < 1 << 31, (Bq, Ng, k, n)


def test_python_validation_and_no_cpu_path(tmp_path):
    from cor_amd import ops, retrieval
    Q, Gq, gs = torch.zeros((2, 32)), torch.zeros((5, 32), dtype=torch.int8), torch.zeros(5)
    with pytest.raises(ValueError):
        ops.similarity_topk_i8(Q, Gq, gs, 0)
    with pytest.raises(ValueError):
        ops.similarity_topk_i8(Q, Gq, gs, 257)
    with pytest.raises(ValueError):
        ops.similarity_topk_i8(Q, Gq.float(), gs, 3)                               # not int8 rows
    with pytest.raises(ValueError):
        ops.similarity_topk_i8(Q, Gq, gs[:4], 3)
    with pytest.raises(ValueError):
        ops.similarity_topk_i8(Q, Gq, gs.double(), 3)
    with pytest.raises(ValueError):
        ops.similarity_topk_i8(Q, Gq, gs, 3, flags=1)
    with pytest.raises(ValueError):
        ops.quantize_rows_i8(torch.zeros((4, 40)))
    with pytest.raises(ValueError):
        ops.quantize_rows_i8(torch.zeros((4, 512)))
    with pytest.raises(ValueError):
        ops.quantize_rows_i8(torch.zeros((4, 32), dtype=torch.float64))
    with pytest.raises(ValueError):
        ops.quantize_rows_i8(torch.zeros(32))
    with pytest.raises(RuntimeError, match="GPU only"):                            # valid arguments on the CPU: no CPU path
        ops.similarity_topk_i8(Q, Gq, gs, 3)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.quantize_rows_i8(torch.zeros((4, 32)))
    with pytest.raises(RuntimeError):
        retrieval.QuantizedShard(Gq, gs)
    with pytest.raises(RuntimeError):
        retrieval.QuantizedShard.from_rows(torch.zeros((4, 32)))
    sh = retrieval.QuantizedShard.__new__(retrieval.QuantizedShard)                 # the constructor refuses CPU tensors; search's own checks
    sh.rows, sh.scales, sh.offset, sh.labels, sh.groups = Gq, gs, 0, None, None
    assert len(sh) == 5
    with pytest.raises(ValueError):
        sh.search(Q, 3, query_labels=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError):
        sh.search(Q, 3, distinct=True)
    assert not hasattr(sh, "rescore") and not hasattr(sh, "expand") and not hasattr(sh, "rerank")
    with pytest.raises(ValueError):
        retrieval.save_gallery(str(tmp_path / "g"), torch.zeros((5, 32)), scales=gs)          # scales go with int8 rows
    with pytest.raises(ValueError):
        retrieval.save_gallery(str(tmp_path / "g"), Gq, scales=gs[:3])


def test_save_gallery_without_scales_is_unchanged(tmp_path):
    import json
    from cor_amd import retrieval
    rows = torch.arange(7 * 16, dtype=torch.float32).reshape(7, 16)
    retrieval.save_gallery(str(tmp_path / "a"), rows, world=2, labels=torch.arange(7))
    man = json.load(open(tmp_path / "a.manifest.json"))
    assert list(man) == ["rows", "dim", "dtype", "world", "labels", "groups", "shards"] and "scales" not in man
    assert sorted(os.listdir(tmp_path)) == ["a.manifest.json", "a.shard00.labels.pt", "a.shard00.pt", "a.shard01.labels.pt", "a.shard01.pt"]
    q = (torch.arange(7 * 16).reshape(7, 16) % 255 - 127).to(torch.int8)
    sc = torch.linspace(0.1, 0.7, 7)
    retrieval.save_gallery(str(tmp_path / "b"), q, world=2, scales=sc)
    man = json.load(open(tmp_path / "b.manifest.json"))
    assert man["scales"] is True and man["dtype"] == "torch.int8"
    for r, (lo, hi) in enumerate((retrieval.shard_bounds(7, 2, 0), retrieval.shard_bounds(7, 2, 1))):
        assert torch.equal(torch.load(man["shards"][r]["scales_file"]), sc[lo:hi]) and torch.equal(torch.load(man["shards"][r]["file"]), q[lo:hi])


# ------------------------------------------------------------------------------------------------------------- the restatement

def _py_quantize_row(row):
    """The definition spelled out element by element: Python floats (doubles) hold the product of two float32 values exactly, so
    rounding that product once to float32 is the fp32 multiply; the two divisions are NumPy float32 divisions."""
    amax = max(abs(float(x)) for x in row)
    if amax == 0.0:
        return [0] * len(row), F(0.0)
    inv = F(127.0) / F(amax)                                                       # one float32 division
    q = []
    for x in row:
        t = F(float(F(x)) * float(inv))                                            # the exact product, rounded once
        r = float(np.rint(t))
        q.append(int(min(max(r, -127.0), 127.0)))
    return q, F(amax) / F(127.0)


@pytest.mark.parametrize("n,C,seed", [(5, 16, 0), (9, 48, 1), (4, 256, 2)])
def test_restatement_against_python_integers(n, C, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, C)).astype(F)
    X[0, 3] = 0.0
    Qf = rng.standard_normal((3, C)).astype(F)
    q, sc = R.ref_quantize(X)
    for g in range(n):
        pq, ps = _py_quantize_row(X[g])
        assert q[g].tolist() == pq and sc[g].view(np.int32) == F(ps).view(np.int32)
    S, qq, qs = R.ref_scores(Qf, q, sc)
    d = R.int_dots(qq, q)
    for b in range(3):
        for g in range(n):
            di = sum(int(a) * int(c) for a, c in zip(qq[b].tolist(), q[g].tolist()))              # Python integers
            assert int(d[b, g]) == di and abs(di) < 2 ** 24
            want = F(F(F(di) * qs[b]) * sc[g])
            assert S[b, g].view(np.int32) == want.view(np.int32)
    for k in (1, 3, n, n + 2):
        a, b = R.ref_topk(S, k, offset=11), R.ref_topk_slow(S, k, offset=11)
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.int32), b[0].view(np.int32))
        assert (a[1][:, n:] == -1).all() and np.isneginf(a[0][:, n:]).all()


def test_int_dots_extreme_values_are_exact():
    q = np.full((2, 256), 127, np.int8)
    g = np.stack([np.full(256, -127, np.int8), np.full(256, 127, np.int8), np.tile(np.array([127, -127], np.int8), 128)])
    assert R.int_dots(q, g).tolist() == [[-127 * 127 * 256, 127 * 127 * 256, 0]] * 2 and 127 * 127 * 256 < 2 ** 24


def test_order_puts_plus_zero_above_minus_zero_and_the_index_decides_ties():
    S = np.array([[-0.0, 0.0, 1.0, 0.0, -0.0, -1.0, 1.0]], F)
    s, i = R.ref_topk(S, 7)
    assert i.tolist() == [[2, 6, 1, 3, 0, 4, 5]]
    assert np.signbit(s[0]).tolist() == [False, False, False, False, True, True, True]


def edge_rows(C=64):
    """The quantiser's edge rows, shared with the GPU test: X f32 [n, C] and what each row is there for."""
    X = np.zeros((12, C), F)
    why = {}
    why[0] = "a zero row"
    X[1, 5] = -3.25; why[1] = "a single non-zero element"
    X[2, 0], X[2, 1], X[2, 7] = 2.5, -2.5, 1.0; why[2] = "+amax and -amax tie"
    X[3, :4] = [1.0, 0.5 / 127, 1.5 / 127, 2.5 / 127]; why[3] = "half-way cases of rintf (amax = 1: inv = 127 exactly)"
    X[3, 4:8] = [-0.5 / 127, -1.5 / 127, -2.5 / 127, 63.5 / 127]
    X[4, :6] = [127.0, 0.5, 1.5, 2.5, -0.5, -126.5]; why[4] = "exact halves (amax = 127: inv = 1)"
    X[5, :3] = [F(0.1), F(0.1) * F(0.999), -F(0.1)]; why[5] = "a value just below amax"
    # amax values with an inexact 127 / amax; for the first two fl(amax * fl(127 / amax)) = 127.00001 > 127
    for j, a in enumerate((F(86.31925964355469), F(12.437085151672363), F(1e-3), F(49.0), F(1e20), F(1e-30))):
        X[6 + j, 0], X[6 + j, 1], X[6 + j, 2] = a, -a, a * F(0.5)
        why[6 + j] = f"amax = {a}"
    return X, why


def test_quantiser_edge_rows_on_the_restatement():
    X, why = edge_rows()
    q, sc = R.ref_quantize(X)
    assert (q[0] == 0).all() and sc[0] == 0
    assert q[1, 5] == -127 and (np.delete(q[1], 5) == 0).all() and sc[1] == F(3.25) / F(127.0)
    assert q[2, :2].tolist() == [127, -127] and q[2, 7] == 51                      # 50.8 -> 51
    assert q[3, :8].tolist() == [127, 0, 2, 2, 0, -2, -2, 64]                      # halves go to the even neighbour
    assert q[4, :6].tolist() == [127, 0, 2, 2, 0, -126]
    assert np.abs(q.astype(np.int32)).max() == 127 and (q != -128).all()
    assert q[5, :3].tolist() == [127, 127, -127]                                   # 126.87 -> 127
    for g in range(5, 12):
        assert q[g, 0] == 127 and (g == 5 or (q[g, 1] == -127 and q[g, 2] == 64)), why[g]      # (63.5 -> 64: half to even)
        pq, ps = _py_quantize_row(X[g])
        assert q[g].tolist() == pq and sc[g].view(np.int32) == F(ps).view(np.int32), why[g]
    # rows 6 and 7: x * inv lands above 127 before the clamp (the clamp is not dead code), and rintf still gives 127
    for g in (6, 7):
        a = X[g, 0]
        assert F(a * F(F(127.0) / a)) > F(127.0)


# ------------------------------------------------------------------------------------------------------------- recall

@pytest.mark.parametrize("C", [256, 64])
def test_int8_coarse_stage_plus_fp32_rescoring_recovers_the_exact_top10(C):
    """Seeded gallery: 20000 unit rows, 64 queries = a row + 0.05 N(0, I), renormalised. The int8 top-k_coarse followed by fp32 re-scoring
    to k = 10 must equal the exact fp32 top-10 for all 64 queries at k_coarse = 100. (On this data it is already complete at k_coarse = 16;
    at k_coarse = 10 it is not, for C = 256 87.5 % of the queries: the coarse stage needs its slack.) The GPU path inherits this through
    bitwise equality with the restatement."""
    rng = np.random.default_rng(7)
    G = rng.standard_normal((20000, C)).astype(F)
    G /= np.linalg.norm(G, axis=1, keepdims=True).astype(F)
    src = rng.integers(0, 20000, 64)
    Q = G[src] + F(0.05) * rng.standard_normal((64, C)).astype(F)
    Q /= np.linalg.norm(Q, axis=1, keepdims=True).astype(F)
    exact = (torch.from_numpy(Q) @ torch.from_numpy(G).T).numpy()
    want = np.argsort(-exact, axis=1, kind="stable")[:, :10]
    gq, gs = R.ref_quantize(G)

    def complete(k_coarse):
        _, cand = R.ref_search(Q, gq, gs, k_coarse)
        fine = np.take_along_axis(exact, cand, axis=1)
        got = np.take_along_axis(cand, np.argsort(-fine, axis=1, kind="stable")[:, :10], axis=1)
        return (got == want).all(axis=1)

    assert complete(100).all()
    assert complete(16).all()
    assert not complete(10).all()

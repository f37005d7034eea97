"""tests/gemm_refs.py proved on the CPU (no GPU, no library call):
  * the reference equals torch's fp64 matmul and torch.nn.functional activations;
  * a plain numpy fp32 emulation of the kernels' accumulation (one rounding per MFMA instruction in K-step order, or per product; adders
    that round to nearest, and adders that TRUNCATE) followed by the fp32 epilogue lies inside the bound, for every activation, both
    output dtypes and every (operand dtype, K) of the GPU file;
  * gelu_erf_bf16out_f's polynomial, transcribed from common.h into fp32 numpy, stays within the 1.3e-4 common.h states;
  * the bound REJECTS planted errors at every shape of the GPU file.

Where a planted error applies. Errors of the product (a product, a 16-byte K chunk, rows, columns, the bias column) are planted at
every shape that has the rows / columns / K for them, on an fp32 output with a bias. A K tail that is not zero-filled is planted where K
has a tail (K bytes not a multiple of 128). Errors of the epilogue are planted at the shapes whose GPU cases use that part of the
epilogue (gemm_refs.all_shapes' features): the periodic residual, the activation / column-scale order and the two GELUs where the GPU
file runs them (the epilogue-matrix and cross-kernel shapes, K of 3 steps), bf16 truncation wherever a bf16 output of at least 64 elements is compared (truncating
and rounding agree on about half of all values, so a handful of elements can pass by chance). The GELU
exchange is planted on fp32 outputs only: the two GELUs differ by at most 4.8e-4, which a bf16 output (ulp 2^-8 at 1) cannot resolve
and gelu_erf_bf16out_f's own 1.3e-4 nearly reaches.
"""
import math

import numpy as np
import pytest
import torch

from tests import gemm_refs as G
from tests import parity_util as pu

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
torch.set_grad_enabled(False)

SHAPES = G.all_shapes()
TK = sorted({(T, K) for T, M, N, K, f in SHAPES}, key=lambda c: (str(c[0]), c[1]))


def d(t):
    return None if t is None else t.to(F64)


# ---------------------------------------------------------------- the reference is torch's
@pytest.mark.parametrize("act", [0, 1, 2, 3, 4])
def test_reference_equals_torch_fp64(act):
    x = G.inputs(3, BF16, 37, 44, 72, period=5)
    a, w = d(x["a"]), d(x["w"])
    z = torch.matmul(a, w.T) + d(x["bias"])
    fn = {0: lambda v: v, 1: torch.nn.functional.gelu, 2: torch.nn.functional.relu, 3: torch.sigmoid,
          4: lambda v: torch.nn.functional.gelu(v, approximate="tanh")}[act]
    want = fn(z) * d(x["col_scale"]) + d(x["residual_p"])[torch.arange(37) % 5]
    ref, bound = G.gemm(a, w, d(x["bias"]), act, d(x["col_scale"]), d(x["residual_p"]), 5)
    assert ref.dtype == F64 and bound.dtype == F64 and bool((bound > 0).all())
    assert torch.allclose(ref, want, rtol=1e-13, atol=1e-15)
    ref32, _ = G.gemm(x["a"].to(F32), x["w"].to(F32), x["bias"], act, x["col_scale"], x["residual_p"], 5)
    assert ref32.dtype == F32                                    # called with fp32: a plain fp32 evaluation
    y3, b3 = G.gemm_x3(a, w, d(x["bias"]), act)
    assert torch.allclose(y3, fn(z), rtol=1e-13, atol=1e-15) and bool((b3 > 0).all())


# ---------------------------------------------------------------- fp32 emulation inside the bound
def trunc32(x64):
    """fp64 -> fp32 rounded TOWARD ZERO"""
    f = x64.astype(np.float32)
    over = np.abs(f.astype(np.float64)) > np.abs(x64)
    return np.where(over, np.nextafter(f, np.float32(0)), f).astype(np.float32)


def gelu_bf16out_np(x):
    """gelu_erf_bf16out_f of common.h in fp32 numpy (an fma is emulated by an fp64 multiply-add rounded once)"""
    fma = lambda p, q, r: (p.astype(np.float64) * q.astype(np.float64) + np.float64(r)).astype(np.float32)
    x = x.astype(np.float32)
    xc = np.clip(x, np.float32(-4), np.float32(4))
    t = xc * xc
    p = fma(np.full_like(t, -2.557373525739815e-09), t, np.float32(2.0897032832641423e-07))
    for c in (-7.421273508272735e-06, 0.00015240515430200944, -0.0020422501798044567, 0.01916329039530596, -0.13212890465728208,
              0.7976113602924678):
        p = fma(p, t, np.float32(c))
    hx = np.float32(0.5) * x
    return (hx.astype(np.float64) * (xc * p).astype(np.float64) + hx.astype(np.float64)).astype(np.float32)


def emulate(x, T, act, extra, out_bf16, chunk, trunc):
    a, w = x["a"].to(F32).numpy(), x["w"].to(F32).numpy()
    M, K = a.shape
    acc = np.zeros((M, w.shape[0]), np.float32)
    for c0 in range(0, K, chunk):                                # K order; inside one instruction the products are summed exactly
        part = a[:, c0:c0 + chunk].astype(np.float64) @ w[:, c0:c0 + chunk].astype(np.float64).T
        acc = trunc32(acc.astype(np.float64) + part) if trunc else (acc.astype(np.float64) + part).astype(np.float32)
    v = acc + x["bias"].numpy()
    if act == 1 and out_bf16:
        v = gelu_bf16out_np(v)
    else:
        v = G.act_ref(torch.from_numpy(v), act).numpy().astype(np.float32)
    if extra == "col_scale":
        v = v * x["col_scale"].numpy()
    if extra == "residual":
        v = v + x["residual_p"].numpy()[np.arange(M) % G.PERIOD]
    t = torch.from_numpy(v.astype(np.float32))
    return t.to(BF16) if out_bf16 else t


@pytest.mark.parametrize("trunc", [False, True])
@pytest.mark.parametrize("T,K", TK, ids=[f"{'bf16' if T == BF16 else 'f32'}-K{K}" for T, K in TK])
def test_fp32_emulation_inside_bound(T, K, trunc):
    M, N = 41, 24
    x = G.inputs(K, T, M, N, K, period=G.PERIOD)
    z0, S0 = G.product(d(x["a"]), d(x["w"]))
    mfma = 16 if T == BF16 else 2                                # k per MFMA instruction: 32x32x16 bf16, 32x32x2 f32
    worst = 0.0
    for chunk in sorted({1, mfma}):
        for act in range(5):
            for extra in ("bias", "col_scale", "residual"):
                for out_bf16 in (False, True):
                    ref, bound = G.epilogue(z0, S0, K, d(x["bias"]), act, d(x["col_scale"]) if extra == "col_scale" else None,
                                            d(x["residual_p"]) if extra == "residual" else None, G.PERIOD, out_bf16)
                    got = emulate(x, T, act, extra, out_bf16, chunk, trunc)
                    rec, fails = pu.compare(got, ref, bound)
                    assert not fails and rec["max_ratio"] <= 1.0, (chunk, act, extra, out_bf16, rec, fails)
                    if not out_bf16:                             # (the ratio of a bf16 output is against its rounding interval)
                        worst = max(worst, rec["max_ratio"])
    print(f"emulation K={K} trunc={trunc}: worst fp32-output ratio {worst:.3f}")


def test_gelu_bf16out_polynomial_within_stated_error():
    x = np.linspace(-6.0, 6.0, 1_200_001)
    got = gelu_bf16out_np(x.astype(np.float32)).astype(np.float64)
    x32 = x.astype(np.float32).astype(np.float64)
    want = np.array(0.5 * x32 * (1.0 + torch.erf(torch.from_numpy(x32) / math.sqrt(2.0)).numpy()))
    err = np.abs(got - want)
    i = int(err.argmax())
    print(f"gelu_erf_bf16out_f: max |error| {err[i]:.4e} at x = {x32[i]:.5f}")
    assert err[i] <= G.GELU_BF16OUT, (err[i], x32[i])


# ---------------------------------------------------------------- planted errors are rejected
def trunc_bf16(y64):
    """fp64 -> bfloat16 by dropping the low 16 bits of the fp32 value (round toward zero) instead of rounding to nearest"""
    b = trunc32(np.asarray(y64, np.float64)).view(np.uint32) & np.uint32(0xFFFF0000)
    return torch.from_numpy(b.view(np.float32).copy()).to(BF16)


def rejected(got64, ref, bound):
    """-> (rejected?, max error / bound) of a planted fp32 output"""
    rec, fails = pu.compare(torch.from_numpy(np.asarray(got64, np.float64)).to(F32), ref, bound)
    return bool(fails), rec["max_ratio"]


def plant_all(T, M, N, K, feat):
    """every planted error that applies at this shape -> {name: (rejected, ratio)}"""
    x = G.inputs(1000 + M + 7 * N + 13 * K, T, M, N, K, period=G.PERIOD)
    a, w, bias, cs = d(x["a"]), d(x["w"]), d(x["bias"]), d(x["col_scale"])
    z0, S0 = G.product(a, w)
    ref, bound = G.epilogue(z0, S0, K, bias)
    z = z0 + bias
    out = {}
    # one product dropped: a typical one (the median |a w| of one output element)
    m0, n0 = M // 2, N // 2
    prods = a[m0] * w[n0]
    k0 = int(prods.abs().argsort()[K // 2])
    g = z.clone(); g[m0, n0] -= prods[k0]
    out["product_dropped"] = rejected(g, ref, bound)
    # one 16-byte K chunk dropped / duplicated
    ce = 16 // G.esz(T)
    c0 = ((K + ce - 1) // ce // 2) * ce
    part = a[:, c0:c0 + ce] @ w[:, c0:c0 + ce].T
    out["chunk_dropped"] = rejected(z - part, ref, bound)
    out["chunk_duplicated"] = rejected(z + part, ref, bound)
    # K tail not zero-filled: the rest of the last K-step holds other values
    pad = -(K * G.esz(T)) % G.ROWB // G.esz(T)
    if pad:
        y = G.inputs(77, T, M, N, pad)
        out["tail_not_zeroed"] = rejected(z + d(y["a"]) @ (d(y["w"]) * math.sqrt(pad / K)).T, ref, bound)
    if M >= 2:
        g = z.clone(); g[[M - 2, M - 1]] = g[[M - 1, M - 2]]
        out["rows_swapped"] = rejected(g, ref, bound)
    if N >= 2:
        c = 4 * ((N - 2) // 4)
        g = z.clone(); g[:, [c, c + 1]] = g[:, [c + 1, c]]
        out["cols_swapped_in_4"] = rejected(g, ref, bound)
    if N >= 5:
        c = 8 * ((N - 5) // 8) + 3
        g = z.clone(); g[:, [c, c + 1]] = g[:, [c + 1, c]]
        out["cols_swapped_in_8"] = rejected(g, ref, bound)
        out["bias_from_n+4"] = rejected(z0 + torch.roll(bias, -4), ref, bound)
        out["bias_from_n-4"] = rejected(z0 + torch.roll(bias, 4), ref, bound)
    if "res" in feat and M > G.PERIOD:
        rp, rf = d(x["residual_p"]), d(x["residual"])
        r2, b2 = G.epilogue(z0, S0, K, bias, 0, None, rp, G.PERIOD)
        wrong = torch.cat([rp, rf[G.PERIOD:]])                   # row m where row m % period was asked
        out["residual_row_not_periodic"] = rejected(z + wrong, r2, b2)
    if "act" in feat:
        for act in (1, 3, 4):                                    # ReLU commutes with a positive scale
            r2, b2 = G.epilogue(z0, S0, K, bias, act, cs)
            out[f"act{act}_after_col_scale"] = rejected(G.act_ref(z * cs, act), r2, b2)
        for asked, given in ((1, 4), (4, 1)):
            r2, b2 = G.epilogue(z0, S0, K, bias, asked)
            out[f"gelu{given}_for_gelu{asked}"] = rejected(G.act_ref(z, given), r2, b2)
    if "bf16" in feat and M * N >= 64:                          # truncation equals rounding on about half of all values
        r2, b2 = G.epilogue(z0, S0, K, bias, 0, None, None, 0, True)
        _, fails = pu.compare(trunc_bf16(r2.numpy()), r2, b2)
        out["bf16_truncated"] = (bool(fails), float("nan"))
    return out


NGROUP = 8


@pytest.mark.parametrize("grp", range(NGROUP))
def test_planted_errors_rejected_at_every_gpu_shape(grp):
    for T, M, N, K, feat in SHAPES[grp::NGROUP]:
        res = plant_all(T, M, N, K, feat)
        missed = [k for k, (rej, _) in res.items() if not rej]
        assert not missed, (T, M, N, K, missed, res)


def test_dropped_product_factor_at_largest_k():
    """The cap on K: the bound grows like K^2 u against one product. At the largest K of each operand dtype a typical dropped product
    still fails by a clear factor (recorded in DESIGN.md 4.1)."""
    for T in (BF16, F32):
        kmax = max(K for t, K in TK if t == T)
        worst = min(plant_all(t, M, N, K, f)["product_dropped"][1] for t, M, N, K, f in SHAPES if t == T and K == kmax)
        print(f"dropped product at K = {kmax} ({'bf16' if T == BF16 else 'f32'}): error / bound >= {worst:.1f}")
        assert worst >= 8.0, (T, kmax, worst)


# ---------------------------------------------------------------- cor_gemm_kernel_id (host only: no launch, nothing is dereferenced)
def test_kernel_id_constants_and_routes():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not os.path.exists(os.path.join(root, "cor_amd", "csrc", "libcor_amd.so")):
        import __graft_entry__ as ge
        ge.build()
    from cor_amd import _native as n
    hdr = open(os.path.join(root, "include", "cor_amd.h")).read()
    for name, val in (("COR_GEMM_KERNEL_SCALAR", n.GEMM_KERNEL_SCALAR), ("COR_GEMM_KERNEL_MASK", n.GEMM_KERNEL_MASK)):
        assert int(re.search(rf"#define {name} (\w+)", hdr).group(1), 0) == val
    assert re.search(r"#define COR_GEMM_EPILOGUE_VEC \(1 << 8\)", hdr) and n.GEMM_EPILOGUE_VEC == 1 << 8
    proto = lambda f: re.search(rf"int {f}\((.*?)\);", hdr, flags=re.S).group(1).split(",")
    assert len(proto("cor_gemm_kernel_id")) == len(proto("cor_gemm")) - 1 == len(n.SIGNATURES["cor_gemm_kernel_id"])
    assert n.SIGNATURES["cor_gemm_kernel_id"] == n.SIGNATURES["cor_gemm"][:-1]
    lib = n.load()
    P = 1 << 20                                                  # an aligned address; the function only looks at its low bits
    V, S = n.GEMM_EPILOGUE_VEC, n.GEMM_KERNEL_SCALAR

    def kid(dt, M, N, K, cd=None, cfg=0, A=P, lda=None, W=P, ldw=None, C=P, ldc=None, bias=0, cs=0, res=0, ldr=0):
        return lib.cor_gemm_kernel_id(A, lda or K, W, ldw or K, dt, C, ldc or N, dt if cd is None else cd, M, N, K, bias, 0, cs, res, ldr, 0, cfg)

    # the automatic dispatch, as documented in gemm.hip
    assert kid(n.BF16, 4096, 2304, 768) == 13 | V                # 144 tiles of 256 x 256
    assert kid(n.F32, 4096, 2304, 768) == 2 | V                  # fp32 operands never take the persistent kernel: 576 tiles of 128 x 128
    assert kid(n.BF16, 4096, 2304, 768, cs=P) == 2 | V           # nor does a column scale
    assert kid(n.F32, 8192, 768, 768) == 3 | V                   # 384 tiles
    assert kid(n.BF16, 2048, 768, 768) == 4 | V                  # 96 tiles
    assert kid(n.BF16, 64, 768, 768) == 4 | V                    # few rows
    assert kid(n.F32, 65536, 256, 2048) == 9 | V
    assert kid(n.BF16, 600, 32, 768) == 1 | V                    # N < 64
    assert kid(n.BF16, 600, 768, 72) == 1 | V                    # K tail
    # demotions of a forced selector
    for cfg in (2, 3, 4, 9, 13):
        assert kid(n.BF16, 300, 264, 72, cfg=cfg) == 1 | V
    assert kid(n.F32, 300, 264, 64, cfg=13) == 2 | V
    assert kid(n.BF16, 300, 268, 64, cfg=13, ldc=272) == 2 | V   # N % 8 != 0
    assert kid(n.BF16, 300, 264, 64, cfg=13, res=P, ldr=264) == 2 | V   # bf16 C with a residual
    assert kid(n.BF16, 300, 264, 64, cfg=13, cd=n.F32, res=P, ldr=264) == 13 | V
    assert kid(n.BF16, 300, 264, 64, cfg=13 | n.ORDER_REVERSE) == 13 | V
    # the epilogue form
    assert kid(n.F32, 300, 7, 64, cfg=2) == 2 and kid(n.F32, 300, 4, 64, cfg=2) == 2 and kid(n.F32, 300, 266, 64, cfg=2) == 2
    assert kid(n.F32, 300, 264, 64, cfg=2, ldc=265) == 2 and kid(n.BF16, 300, 264, 64, cfg=2, ldc=268) == 2
    assert kid(n.BF16, 300, 264, 64, cd=n.F32, cfg=2, ldc=268) == 2 | V
    for kw in (dict(C=P + 4), dict(bias=P + 4), dict(cs=P + 8), dict(res=P + 4, ldr=264), dict(res=P, ldr=266)):
        assert kid(n.F32, 300, 264, 64, cfg=2, **kw) == 2, kw
    assert kid(n.BF16, 300, 264, 64, cfg=13, C=P + 2) == 2       # 13 has the vector form only
    # the scalar kernel: each reason
    assert kid(n.BF16, 33, 31, 65) == S and kid(n.F32, 33, 31, 3) == S
    assert kid(n.F32, 33, 31, 64, lda=65) == S and kid(n.F32, 33, 31, 64, ldw=65) == S
    assert kid(n.BF16, 33, 31, 64, A=P + 2, lda=72) == S and kid(n.BF16, 33, 31, 64, W=P + 2, ldw=72) == S
    assert kid(n.BF16, 33, 31, 64, lda=72, ldw=72) == 1          # aligned strides: a tile kernel (N = 31: scalar epilogue)
    # x3: the route of bf16 operands over 3K
    assert kid(n.BF16X3, 2048, 768, 768, cd=n.F32, lda=2304, ldw=2304) == kid(n.BF16, 2048, 768, 2304, cd=n.F32)
    # refusals, as cor_gemm
    assert kid(n.F32, 0, 8, 8) == n.EINVAL and kid(n.F32, 8, 8, 8, A=0) == n.EINVAL and kid(n.F32, 8, 8, 8, cfg=5) == n.EINVAL
    assert kid(n.F32, 8, 8, 8, cfg=2 | (1 << 12)) == n.EINVAL and kid(n.F32, 8, 8, 8, res=P, ldr=7) == n.EINVAL
    assert kid(n.F16, 8, 8, 8) == n.ENOSUPPORT and kid(n.F32, 8, 8, 8, cd=n.F16) == n.ENOSUPPORT

"""fp64 reference of cor_gemm (cor_amd/csrc/gemm.hip) with its a-priori error bound, and the case tables the GPU file
(tests/test_gpu_gemm_kernels.py) runs and the CPU file (tests/test_cpu_gemm_refs.py) proves the bound on.

Same rule and style as tests/small_kernel_refs.py (U, MARGIN, act_ref and act_err are ITS objects, not copies): every function takes
torch CPU tensors and returns (ref, bound) in the dtype of its inputs. Called with float64 it is the reference and the bound a kernel
is held to; called with float32 its first result is a plain fp32 evaluation. bf16 operands are widened by the caller first: the
reference sees the values the kernel sees.

    C = residual[m % period] + col_scale * act(a . w^T + bias)

  z  = a . w^T + bias                      in fp64
  S  = |a| . |w|^T + |bias|
  dz = (K + 2) u S                         a chain or tree of K fp32 accumulations in ANY order, plus the bias add. The factor is
                                           K + 1 for round-to-nearest adders; the rounding of the MFMA's internal adder is not
                                           documented, and a TRUNCATING adder loses up to 2u per addition instead of u. That case is
                                           what MARGIN (the factor 2 on the whole bound) covers for the accumulation term: this part of
                                           the bound is reasoned, not derived from a specification.
  act: act_err(z, dz, act) of small_kernel_refs. COR_ACT_GELU_ERF with a bf16 OUTPUT runs gelu_erf_bf16out_f (a polynomial erf,
       common.h) instead of erf_as: its stated |GELU error| <= 1.3e-4 (GELU_BF16OUT; checked on a dense grid by the CPU file, fp32
       evaluation included) replaces the erf_as term; the argument error is still carried by 1.13 dz.
  col_scale: one rounding, u |y cs|;  residual: one rounding, u |y + r|.
  The whole bound is multiplied by MARGIN. bf16 outputs go through parity_util.check's rounding interval: no blanket ulp here.

x3 operands (COR_BF16X3): the same reference on the fp32 values; the bound is the existing contract of tests/test_gpu_query_exact.py,
2.5e-6 of the error scale plus 1e-6 |ref| for the fp32 epilogue functions (gemm_x3).
Nothing here is fitted to what a kernel returns.
"""
from __future__ import annotations

import numpy as np
import torch

from tests.small_kernel_refs import MARGIN, U, act_err, act_ref

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
GELU_BF16OUT = 1.3e-4              # |gelu_erf_bf16out_f(x) - GELU(x)|, common.h
X3_REL, X3_EPI = 2.5e-6, 1e-6      # tests/test_gpu_query_exact.py::test_x3_gemm_epilogues_and_configs


# ---------------------------------------------------------------- reference and bound
def product(a, w):
    """(a . w^T, |a| . |w|^T): the part of a case that its epilogue variants share."""
    return a @ w.T, a.abs() @ w.abs().T


def epilogue(z0, S0, K, bias=None, act=0, col_scale=None, residual=None, res_row_mod=0, out_bf16=False):
    z, S = z0, S0
    if bias is not None:
        z, S = z + bias, S + bias.abs()
    dz = (K + 2) * U * S
    y = act_ref(z, act)
    if act == 1 and out_bf16:
        dy = 1.13 * dz + GELU_BF16OUT
    else:
        dy = act_err(z, dz, act)
    if col_scale is not None:
        y = y * col_scale
        dy = dy * col_scale.abs() + U * y.abs()
    if residual is not None:
        r = residual
        if res_row_mod > 0:
            r = residual[torch.arange(z.shape[0]) % res_row_mod]
        y = y + r
        dy = dy + U * y.abs()
    return y, MARGIN * dy


def gemm(a, w, bias=None, act=0, col_scale=None, residual=None, res_row_mod=0, out_bf16=False):
    z0, S0 = product(a, w)
    return epilogue(z0, S0, a.shape[1], bias, act, col_scale, residual, res_row_mod, out_bf16)


def gemm_x3(a, w, bias=None, act=0, col_scale=None, residual=None):
    """x3 GEMM on the fp32 values a, w: (ref, bound) under the 2.5e-6 contract (error scale as test_gpu_query_exact._ref_gemm forms it)."""
    z, S = product(a, w)
    if bias is not None:
        z, S = z + bias, S + bias.abs()
    y = act_ref(z, act)
    if col_scale is not None:
        y, S = y * col_scale, S * col_scale.abs()
    if residual is not None:
        y, S = y + residual, S + residual.abs()
    return y, X3_REL * S + X3_EPI * y.abs()


# ---------------------------------------------------------------- inputs (CPU generator, seeded)
def inputs(seed, T, M, N, K, period=0):
    """a ~ N(0,1), w ~ N(0,1)/sqrt K in the operand dtype T; bias ~ N(0,1), col_scale in [0.5, 1.5], residual ~ N(0,1) fp32."""
    r = np.random.default_rng(seed)
    f = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    return dict(a=f(r.standard_normal((M, K))).to(T), w=f(r.standard_normal((N, K)) / np.sqrt(K)).to(T), bias=f(r.standard_normal(N)),
                col_scale=f(r.uniform(0.5, 1.5, N)), residual=f(r.standard_normal((M, N))),
                residual_p=f(r.standard_normal((period, N))) if period else None)


# ---------------------------------------------------------------- the cases of the GPU file
TILE = {1: (128, 128), 2: (128, 128), 3: (128, 64), 4: (64, 64), 9: (256, 128), 13: (256, 256)}   # selector -> BM x BN
TILE_CFGS = (1, 2, 3, 4, 9)
KSTEPS = (1, 2, 3, 4, 5, 7)
ROWB = 128                                                       # bytes of K per K-step
KTAIL_BYTES = (16, 48, 128 + 16, 256 + 112)
SCALAR_K = (1, 3, 31, 33, 65)
SCALAR_MN = (1, 31, 33)
PERIOD = 37
PAIRS = ((F32, F32), (BF16, BF16), (BF16, F32), (F32, BF16))
EXTRAS = ("bias", "nobias", "col_scale", "residual", "residual_periodic", "residual_strided", "residual_inplace")


def esz(T):
    return 2 if T == BF16 else 4


def step(T):
    return ROWB // esz(T)


def operand_dtypes(cfg):
    return (BF16,) if cfg == 13 else (BF16, F32)


def kstep_cases():
    return [(cfg, T, TILE[cfg][0] + 1, TILE[cfg][1] + 8, step(T) * n) for cfg in TILE for T in operand_dtypes(cfg) for n in KSTEPS]


def ktail_cases():
    return [(T, 129, 136, kb // esz(T)) for T in (BF16, F32) for kb in KTAIL_BYTES]


def scalar_k_cases():
    return [(T, M, N, K) for T in (BF16, F32) for K in SCALAR_K for M in SCALAR_MN for N in SCALAR_MN]


SCALAR_ALIGNED = (33, 31, 64)                                    # M, N, K of the odd-lda / odd-ldw / misaligned-base cases


def edge_ns(cfg, vec):
    BN = TILE[cfg][1]
    if not vec:
        return (1, 7, BN + 1)
    ns = (8, 12, BN - 4, BN + 4)                                 # N % 8 == 4: the bf16 half store
    return ns + (16, BN - 8, BN + 8) if cfg == 13 else ns        # the persistent kernel takes N % 8 == 0 only


def edge_cases():
    out = []
    for cfg in TILE:
        BM = TILE[cfg][0]
        for T in operand_dtypes(cfg):
            for vec in (True, False):
                out += [(cfg, T, vec, M, N, 2 * step(T)) for M in (1, BM - 1, BM + 1) for N in edge_ns(cfg, vec)]
    return out


def epilogue_shapes(cfg, T):
    """M = BM + 33, N = BN + 12, K of 3 steps. The persistent kernel takes N % 8 == 0 only (N = BN + 12 is demoted to cfg 2, which the
    GPU file asserts and still checks), so bf16 operands on cfg 13 run N = BN + 8 as well."""
    BM, BN = TILE[cfg]
    ns = (BN + 12, BN + 8) if cfg == 13 and T == BF16 else (BN + 12,)
    return [(BM + 33, N, 3 * step(T)) for N in ns]


ORDER_TILES = ((1, 1), (7, 1), (3, 3), (17, 1), (9, 2))          # (tm, tn): 1, 7, 9, 17 tiles and the ragged band tm = 9, tn = 2
PP_ORDER_SHAPES = ((2 * 256 - 3, 256), (3 * 256 - 3, 3 * 256 - 8), (300, 3 * 256 - 8), (300, 5 * 256 - 8), (300, 1288))


def order_cases():
    out = [(cfg, T, tm * TILE[cfg][0] - 5, tn * TILE[cfg][1] - 4, 2 * step(T)) for cfg in TILE_CFGS for T in (BF16, F32) for tm, tn in ORDER_TILES]
    return out + [(13, BF16, M, N, 3 * step(BF16)) for M, N in PP_ORDER_SHAPES]


CROSS_SHAPE = (289, 264)                                         # M, N of the cross-kernel / batch-invariance cases; K = 3 steps
GUARD = (2, 3)                                                   # guard rows above / below a C view


def all_shapes():
    """Every (T, M, N, K, features) the GPU file compares against this reference; features: what the epilogue of that case uses
    ("act": activations and the column scale, "res": the periodic residual, "bf16": a bf16 output)."""
    s = {}

    def add(T, M, N, K, *feat):
        s.setdefault((T, M, N, K), set()).update(feat)
    for cfg, T, M, N, K in kstep_cases():
        add(T, M, N, K)
    for T, M, N, K in ktail_cases():
        add(T, M, N, K)
    for T, M, N, K in scalar_k_cases():
        add(T, M, N, K)
    for T in (BF16, F32):
        add(T, *SCALAR_ALIGNED)
    for cfg, T, vec, M, N, K in edge_cases():
        add(T, M, N, K, "bf16")
    for cfg in TILE:
        for T in (BF16, F32):
            for shp in epilogue_shapes(cfg, T):
                add(T, *shp, "act", "res", "bf16")
    for cfg, T, M, N, K in order_cases():
        add(T, M, N, K)
    for T in (BF16, F32):
        add(T, *CROSS_SHAPE, 3 * step(T), "act", "res", "bf16")
    return sorted(((T, M, N, K, frozenset(f)) for (T, M, N, K), f in s.items()), key=lambda c: (str(c[0]), c[1:4]))

"""cor_gemm kernel by kernel: every selector (the scalar kernel, cfg 1, 2, 3, 4, 9, 13), operand / output dtype pair, epilogue form and
edge, called directly through cor_amd.ops.gemm on small seeded inputs and compared - the WHOLE output - with the fp64 reference and a-priori
bound of tests/gemm_refs.py (proved on the CPU, planted errors included, by tests/test_cpu_gemm_refs.py). Every case first asserts with
cor_gemm_kernel_id that the intended kernel and epilogue form are the ones that run: a forced selector that the dispatch demotes is
named as such, never run under the wrong label. Every check leaves its error / bound ratio in the parity report (parity_util)."""
import pytest
import torch

from tests import gemm_refs as G
from tests import parity_util as pu

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

DEV = "cuda:0"
F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
SENTINEL = -7777.0


def ops():
    from cor_amd import ops as o
    return o


def nat():
    from cor_amd import _native
    return _native


def nm(dt):
    return "bf16" if dt == BF16 else "f32"


def d(t):
    return None if t is None else t.detach().cpu().to(F64)


def g(t):
    return None if t is None else t.to(DEV)


def up8(n):
    return (n + 7) // 8 * 8


def make_out(M, N, TO, vec, fill=None):
    """an output view that takes the vector epilogue (16-byte aligned, ldc a multiple of 8) or, for an N that would, the scalar one (base
    one element off, odd ldc). N % 4 != 0 or N < 8 is scalar by itself."""
    if vec:
        buf = torch.empty((M, up8(N)), dtype=TO, device=DEV)
        out = buf[:, :N]
    else:
        buf = torch.empty((M, (N + 3) | 1), dtype=TO, device=DEV)
        out = buf[:, 1:1 + N]
    if fill is not None:
        buf.fill_(fill)
    return out


def route(a, w, out, bias=None, act=0, col_scale=None, residual=None, res_row_mod=0, cfg=0, reverse=False, x3=False):
    """cor_gemm_kernel_id for exactly the call ops.gemm makes"""
    o, n = ops(), nat()
    M, K, lda = o._rows(a)
    N, _, ldw = o._rows(w)
    _, _, ldc = o._rows(out)
    ldr = o._rows(residual)[2] if residual is not None else 0
    p = lambda t: 0 if t is None else t.data_ptr()
    return n.load().cor_gemm_kernel_id(a.data_ptr(), lda, w.data_ptr(), ldw, n.BF16X3 if x3 else o._dt(a), out.data_ptr(), ldc, o._dt(out), M, N,
                                       K // 3 if x3 else K, p(bias), act, p(col_scale), p(residual), ldr, res_row_mod,
                                       int(cfg) | (n.ORDER_REVERSE if reverse else 0))


def expected(cfg, T, TO, N, K, vec, col_scale=False, residual=False):
    """the kernel a FORCED tile selector runs after the documented demotions, with the epilogue form the case intends"""
    k = cfg
    if K * G.esz(T) % G.ROWB:
        k = 1                                                    # K tail: only the register-staged kernel zero-fills it
    elif cfg == 13 and not (T == BF16 and vec and not col_scale and N % 8 == 0 and not (TO == BF16 and residual)):
        k = 2
    return k | (nat().GEMM_EPILOGUE_VEC if vec else 0)


def run(want, a, w, out, **kw):
    """assert the route, then launch"""
    got = route(a, w, out, **kw)
    assert got == want, f"cor_gemm_kernel_id {got:#x}, the case needs {want:#x}"
    return ops().gemm(a, w, out=out, **kw)


def label(kid):
    n = nat()
    k = kid & n.GEMM_KERNEL_MASK
    return ("scalar" if k == n.GEMM_KERNEL_SCALAR else f"k{k}") + ("v" if kid & n.GEMM_EPILOGUE_VEC else "s")


# ====================================================================================================== K steps
@pytest.mark.parametrize("cfg,T", [(c, T) for c in G.TILE for T in G.operand_dtypes(c)], ids=lambda v: nm(v) if isinstance(v, torch.dtype) else str(v))
def test_k_steps(cfg, T):
    """nkt = 1, 2, 3, 4, 5, 7 K-steps: prologue only, the first in-loop wait, steady state, cfg 9's three-buffer wrap, gemm_pp's ring wrap"""
    for c, t, M, N, K in G.kstep_cases():
        if (c, t) != (cfg, T):
            continue
        x = G.inputs(K + cfg, T, M, N, K)
        ref, bound = G.gemm(d(x["a"]), d(x["w"]), d(x["bias"]))
        for TO in (F32, BF16):
            want = expected(cfg, T, TO, N, K, True)
            assert want & 0xff == cfg
            out = run(want, g(x["a"]), g(x["w"]), make_out(M, N, TO, True), bias=g(x["bias"]), cfg=cfg)
            pu.check(f"gemm.ksteps[{label(want)},{nm(T)}->{nm(TO)},{M}x{N}x{K}]", out.cpu(), ref, bound)


@pytest.mark.parametrize("T", [BF16, F32], ids=nm)
def test_cfg1_k_tails(T):
    """K bytes 16, 48, 128 + 16, 256 + 112: the zero-filled tail of the register-staged kernel; a forced 2, 3, 4, 9 or 13 is demoted to 1"""
    for t, M, N, K in G.ktail_cases():
        if t != T:
            continue
        x = G.inputs(K, T, M, N, K)
        ref, bound = G.gemm(d(x["a"]), d(x["w"]), d(x["bias"]))
        first = None
        for cfg in (1, 2, 3, 4, 9, 13):
            want = 1 | nat().GEMM_EPILOGUE_VEC
            out = run(want, g(x["a"]), g(x["w"]), make_out(M, N, F32, True), bias=g(x["bias"]), cfg=cfg)
            if cfg == 1:
                pu.check(f"gemm.ktail[k1v,{nm(T)}->f32,{M}x{N}x{K}]", out.cpu(), ref, bound)
                first = out.clone()
            else:
                assert torch.equal(out, first)
        out = run(1, g(x["a"]), g(x["w"]), make_out(M, N, BF16, False), bias=g(x["bias"]), cfg=1)
        pu.check(f"gemm.ktail[k1s,{nm(T)}->bf16,{M}x{N}x{K}]", out.cpu(), ref, bound)


# ====================================================================================================== the scalar kernel
@pytest.mark.parametrize("T", [BF16, F32], ids=nm)
def test_scalar_kernel_by_each_reason(T):
    S = nat().GEMM_KERNEL_SCALAR
    for t, M, N, K in G.scalar_k_cases():                        # K * esz % 16 != 0
        if t != T:
            continue
        x = G.inputs(M * 100 + N * 10 + K, T, M, N, K)
        ref, bound = G.gemm(d(x["a"]), d(x["w"]), d(x["bias"]), 1)
        for TO in (F32, BF16):
            out = run(S, g(x["a"]), g(x["w"]), torch.empty((M, N), dtype=TO, device=DEV), bias=g(x["bias"]), act=1, cfg=0)
            rb = G.gemm(d(x["a"]), d(x["w"]), d(x["bias"]), 1, out_bf16=True) if TO == BF16 else (ref, bound)
            pu.check(f"gemm.scalar_k[{label(S)},{nm(T)}->{nm(TO)},{M}x{N}x{K}]", out.cpu(), *rb)
    M, N, K = G.SCALAR_ALIGNED
    x = G.inputs(5, T, M, N, K, period=7)
    a, w = g(x["a"]), g(x["w"])
    wide = lambda t, pad, off: torch.cat([torch.zeros((t.shape[0], off), dtype=T, device=DEV), t,
                                          torch.zeros((t.shape[0], pad - off), dtype=T, device=DEV)], 1)[:, off:off + K]
    per = 16 // G.esz(T)
    # an aligned K each time: an odd row stride, or a base one element off an aligned buffer whose row stride stays a multiple of 16 bytes
    views = {"aligned": (a, w, False), "odd_lda": (wide(a, 1, 0), w, True), "odd_ldw": (a, wide(w, 1, 0), True),
             "a_base_off": (wide(a, per, 1), w, True), "w_base_off": (a, wide(w, per, 1), True)}
    ref, bound = G.gemm(d(x["a"]), d(x["w"]), d(x["bias"]), 3, d(x["col_scale"]), d(x["residual_p"]), 7)
    for name, (av, wv, scalar) in views.items():
        assert av.stride(1) == 1 and torch.equal(av, a) and torch.equal(wv, w)
        out = torch.empty((M, N), dtype=F32, device=DEV)
        kid = route(av, wv, out, bias=g(x["bias"]), act=3, col_scale=g(x["col_scale"]), residual=g(x["residual_p"]), res_row_mod=7)
        assert (kid == S) == scalar, (name, kid)
        ops().gemm(av, wv, out=out, bias=g(x["bias"]), act=3, col_scale=g(x["col_scale"]), residual=g(x["residual_p"]), res_row_mod=7)
        pu.check(f"gemm.scalar_reason[{label(kid)},{nm(T)}->f32,{name}]", out.cpu(), ref, bound)


# ====================================================================================================== M / N edges
@pytest.mark.parametrize("vec", [True, False], ids=["vec", "scalar_epi"])
@pytest.mark.parametrize("cfg,T", [(c, T) for c in G.TILE for T in G.operand_dtypes(c)], ids=lambda v: nm(v) if isinstance(v, torch.dtype) else str(v))
def test_mn_edges(cfg, T, vec):
    """M = 1, BM - 1, BM + 1; vector epilogue N = 8, 12, BN - 4, BN + 4 (N % 8 == 4: the bf16 half store), scalar epilogue N = 1, 7, BN + 1"""
    ran = set()
    for c, t, v, M, N, K in G.edge_cases():
        if (c, t, v) != (cfg, T, vec):
            continue
        x = G.inputs(M + N, T, M, N, K)
        ref, bound = G.gemm(d(x["a"]), d(x["w"]), d(x["bias"]))
        want = expected(cfg, T, T, N, K, vec)
        out = run(want, g(x["a"]), g(x["w"]), make_out(M, N, T, vec), bias=g(x["bias"]), cfg=cfg)
        pu.check(f"gemm.edges[{label(want)},{nm(T)}->{nm(T)},{M}x{N}x{K}]", out.cpu(), ref, bound)
        ran.add(want & 0xff)
    assert cfg in ran or not vec                                 # the selector itself ran (13 has no scalar epilogue: those run as 2)


# ====================================================================================================== the epilogue matrix
def _extra(x, name, M, N, vec):
    """-> (kwargs for ops.gemm on the device, kwargs for the reference)"""
    bias = None if name == "nobias" else x["bias"]
    dev, ref = dict(bias=g(bias)), dict(bias=d(bias))
    if name == "col_scale":
        dev["col_scale"], ref["col_scale"] = g(x["col_scale"]), d(x["col_scale"])
    elif name == "residual":
        dev["residual"], ref["residual"] = g(x["residual"]), d(x["residual"])
    elif name == "residual_periodic":
        dev.update(residual=g(x["residual_p"]), res_row_mod=G.PERIOD)
        ref.update(residual=d(x["residual_p"]), res_row_mod=G.PERIOD)
    elif name == "residual_strided":
        buf = torch.zeros((M, N + 8), dtype=F32, device=DEV)
        off = 4 if vec else 3                                    # a 16-byte aligned view / a misaligned one
        buf[:, off:off + N] = g(x["residual"])
        dev["residual"], ref["residual"] = buf[:, off:off + N], d(x["residual"])
    return dev, ref


def _epilogue_matrix(cfg, T, TO, M, N, K):
    x = G.inputs(cfg * 7 + K + N, T, M, N, K, period=G.PERIOD)
    a, w = g(x["a"]), g(x["w"])
    z0, S0 = G.product(d(x["a"]), d(x["w"]))
    ran = set()
    for vec in (True, False):
        for extra in G.EXTRAS:
            if extra == "residual_inplace" and TO != F32:
                continue                                         # the residual is fp32: it can alias an fp32 output only
            for act in range(5):
                out = make_out(M, N, TO, vec)
                if extra == "residual_inplace":
                    out.copy_(g(x["residual"]))
                    dev, ref = dict(bias=g(x["bias"]), residual=out), dict(bias=d(x["bias"]), residual=d(x["residual"]))
                else:
                    dev, ref = _extra(x, extra, M, N, vec)
                want = expected(cfg, T, TO, N, K, vec, "col_scale" in dev, "residual" in dev)
                if extra == "col_scale":
                    assert want & 0xff != 13
                run(want, a, w, out, act=act, cfg=cfg, **dev)
                r, b = G.epilogue(z0, S0, K, act=act, out_bf16=TO == BF16, **ref)
                pu.check(f"gemm.epilogue[{label(want)},{nm(T)}->{nm(TO)},N{N},act{act},{extra}]", out.cpu(), r, b)
                ran.add(want)
    return ran


@pytest.mark.parametrize("T,TO", G.PAIRS, ids=nm)
@pytest.mark.parametrize("cfg", list(G.TILE))
def test_epilogue_matrix(cfg, T, TO):
    """activation 0-4 x {bias, no bias, column scale, residual, periodic residual (37 rows), strided residual view, residual aliased to the
    output} in both epilogue forms, at M = BM + 33, N = BN + 12 (N % 8 == 4), K of 3 steps; cfg 13 (N % 8 == 0 only) also at N = BN + 8"""
    ran = set()
    for M, N, K in G.epilogue_shapes(cfg, T):
        ran |= _epilogue_matrix(cfg, T, TO, M, N, K)
    V = nat().GEMM_EPILOGUE_VEC
    if cfg != 13:
        assert ran == {cfg | V, cfg}                             # both forms of the selector itself
    elif T == BF16:
        assert ran == {13 | V, 2 | V, 2}                         # 13 has the vector form only and no column scale; the rest runs as 2
    else:
        assert ran == {2 | V, 2}


# ====================================================================================================== tile order
@pytest.mark.parametrize("cfg,T", [(c, T) for c in G.TILE for T in G.operand_dtypes(c)], ids=lambda v: nm(v) if isinstance(v, torch.dtype) else str(v))
def test_tile_order(cfg, T):
    """grids of 1, 7, 9, 17 tiles (xcd_remap's remainder branch), the ragged band tm = 9 x tn = 2; gemm_pp with 2 and 9 tiles (idle
    blocks), tn = 3 (XCD-stationary order, a partial group of W-panels), tn = 5 and N = 1288 (banded order). COR_ORDER_REVERSE: equal bits."""
    BM, BN = G.TILE[cfg]
    for c, t, M, N, K in G.order_cases():
        if (c, t) != (cfg, T):
            continue
        x = G.inputs(M + N + cfg, T, M, N, K)
        ref, bound = G.gemm(d(x["a"]), d(x["w"]), d(x["bias"]))
        want = expected(cfg, T, T, N, K, True)
        assert want & 0xff == cfg
        kw = dict(bias=g(x["bias"]), cfg=cfg)
        out = run(want, g(x["a"]), g(x["w"]), make_out(M, N, T, True), **kw)
        tiles = f"{-(-M // BM)}x{-(-N // BN)}"
        pu.check(f"gemm.order[{label(want)},{nm(T)}->{nm(T)},tiles{tiles},{M}x{N}x{K}]", out.cpu(), ref, bound)
        rev = run(want, g(x["a"]), g(x["w"]), make_out(M, N, T, True), reverse=True, **kw)
        pu.check_bitwise(f"gemm.order_reverse[{label(want)},{nm(T)},tiles{tiles}]", rev.cpu(), out.cpu())


# ====================================================================================================== cross-kernel bits, batch invariance
@pytest.mark.parametrize("T,TO", G.PAIRS, ids=nm)
def test_cross_kernel_bits_and_batch_invariance(T, TO):
    """K bytes a multiple of 128: cfg 1, 2, 3, 4, 9 (and 13 for bf16 operands) give equal bits with every epilogue, and rows r0:r0+m of A
    run alone equal those rows of the full call (the batch-invariance contract of DESIGN.md; the scalar kernel is excluded: alignment
    selects it, not M)."""
    M, N = G.CROSS_SHAPE
    K = 3 * G.step(T)
    x = G.inputs(17, T, M, N, K, period=G.PERIOD)
    a, w = g(x["a"]), g(x["w"])
    for extra in ("bias", "col_scale", "residual", "residual_periodic"):
        dev, ref = _extra(x, extra, M, N, True)
        for act in range(5):
            first = None
            for cfg in G.TILE:
                want = expected(cfg, T, TO, N, K, True, "col_scale" in dev, "residual" in dev)
                if want & 0xff != cfg:
                    continue                                     # a demoted 13 would only repeat cfg 2
                out = run(want, a, w, make_out(M, N, TO, True), act=act, cfg=cfg, **dev)
                if first is None:
                    first = out.clone()
                    r, b = G.gemm(d(x["a"]), d(x["w"]), act=act, out_bf16=TO == BF16, **ref)
                    pu.check(f"gemm.cross[{label(want)},{nm(T)}->{nm(TO)},act{act},{extra}]", out.cpu(), r, b)
                else:
                    assert torch.equal(out, first), (cfg, act, extra)
    full = {cfg: ops().gemm(a, w, out=make_out(M, N, TO, True), bias=g(x["bias"]), cfg=cfg) for cfg in (0,) + tuple(G.TILE)}
    for cfg, y in full.items():
        assert torch.equal(y, full[0]), cfg
        for r0, m in ((0, 1), (100, 37), (160, 129), (288, 1)):
            part = ops().gemm(a[r0:r0 + m], w, out=make_out(m, N, TO, True), bias=g(x["bias"]), cfg=cfg)
            assert torch.equal(part, full[0][r0:r0 + m]), (cfg, r0, m)


# ====================================================================================================== guard bands
@pytest.mark.parametrize("TO", [F32, BF16], ids=nm)
@pytest.mark.parametrize("cfg,T", [(c, T) for c in G.TILE for T in G.operand_dtypes(c)], ids=lambda v: nm(v) if isinstance(v, torch.dtype) else str(v))
def test_guard_bands(cfg, T, TO):
    """C is a view in the middle of a sentinel-filled buffer: rows above and below, columns left and right (a 16-byte aligned column offset
    for the vector form, one element for the scalar form). The vector epilogues write 16 bytes at a time: the sentinel stays intact."""
    M, N, K = G.TILE[cfg][0] + 1, G.TILE[cfg][1] + 8, 2 * G.step(T)
    x = G.inputs(cfg + 31, T, M, N, K)
    ref, bound = G.gemm(d(x["a"]), d(x["w"]), d(x["bias"]), 2)
    top, bot = G.GUARD
    for vec in (True, False):
        left, right = (8, 8) if vec else (1, 4)
        buf = torch.full((top + M + bot, left + N + right), SENTINEL, dtype=TO, device=DEV)
        out = buf[top:top + M, left:left + N]
        want = expected(cfg, T, TO, N, K, vec)
        run(want, g(x["a"]), g(x["w"]), out, bias=g(x["bias"]), act=2, cfg=cfg)
        pu.check(f"gemm.guard[{label(want)},{nm(T)}->{nm(TO)}]", out.cpu(), ref, bound)
        got = buf.clone()
        got[top:top + M, left:left + N] = SENTINEL
        pu.check_bitwise(f"gemm.guard_sentinel[{label(want)},{nm(T)}->{nm(TO)}]", got.cpu(), torch.full_like(buf, SENTINEL).cpu())


# ====================================================================================================== x3
@pytest.mark.parametrize("cfg", list(G.TILE))
def test_x3_whole_output(cfg):
    """x3 operands on every selector, the whole output under the 2.5e-6 contract of test_gpu_query_exact.py, at the depth that contract
    is stated for (include/cor_amd.h: K = 768). The contract is a statistical one: the format itself drops a_lo w_lo and rounds lo, up to
    3 * 2^-18 = 1.1e-5 of sum|a w| in the worst case, and the error of a sum of K such terms shrinks like 1 / sqrt K against sum|a w|. At
    K = 64 (129 x 136, every selector) this comparison measured 3.2e-6 ... 4.4e-6 of the scale: above the contract, below the format's
    worst case, the same on all six kernels."""
    M, N, K = 129, 136, 768
    x = G.inputs(cfg, F32, M, N, K)
    A3, W3 = ops().split_x3(g(x["a"])), ops().split_weight_x3(g(x["w"]))
    out = make_out(M, N, F32, True)
    want = expected(cfg, BF16, F32, N, 3 * K, True)
    run(want, A3, W3, out, bias=g(x["bias"]), act=1, cfg=cfg, x3=True)
    ref, bound = G.gemm_x3(d(x["a"]), d(x["w"]), d(x["bias"]), 1)
    pu.check(f"gemm.x3[{label(want)},x3->f32,{M}x{N}x{K}]", out.cpu(), ref, bound)


# ====================================================================================================== refusals
def test_refusals_leave_c_untouched():
    n = nat()
    lib = n.load()
    M, N, K = 8, 16, 64
    a = torch.ones((M, 3 * K), dtype=F32, device=DEV)
    w = torch.ones((N, 3 * K), dtype=F32, device=DEV)
    c = torch.full((M, N), SENTINEL, dtype=F32, device=DEV)
    res = torch.ones((M, N), dtype=F32, device=DEV)
    base = dict(A=a.data_ptr(), lda=3 * K, W=w.data_ptr(), ldw=3 * K, ab=n.F32, C=c.data_ptr(), ldc=N, cd=n.F32, M=M, N=N, K=K, bias=0, act=0,
                cs=0, res=0, ldr=0, mod=0, cfg=0)
    order = ("A", "lda", "W", "ldw", "ab", "C", "ldc", "cd", "M", "N", "K", "bias", "act", "cs", "res", "ldr", "mod", "cfg")
    stream = torch.cuda.current_stream().cuda_stream

    def both(want, **ch):
        args = [dict(base, **ch)[k] for k in order]
        assert lib.cor_gemm_kernel_id(*args) == want, ch
        assert lib.cor_gemm(*args, stream) == want, ch
        torch.cuda.synchronize()
        assert bool((c == SENTINEL).all()), ch

    for ch in (dict(A=0), dict(W=0), dict(C=0), dict(M=0), dict(M=-1), dict(N=0), dict(N=-1), dict(K=0), dict(K=-1), dict(lda=K - 1),
               dict(ldw=K - 1), dict(ldc=N - 1), dict(res=res.data_ptr(), ldr=N - 1), dict(ab=n.BF16X3, lda=3 * K - 1),
               dict(ab=n.BF16X3, ldw=3 * K - 1), dict(cfg=-1), dict(cfg=-(1 << 31) + 2), dict(cfg=5), dict(cfg=14), dict(cfg=255),
               dict(cfg=2 | n.ORDER_REVERSE | (1 << 8))):
        both(n.EINVAL, **ch)
    for bit in range(8, 30):                                     # every ablation bit of the development builds
        both(n.EINVAL, cfg=2 | (1 << bit))
    for ch in (dict(ab=n.F16), dict(cd=n.F16), dict(ab=7), dict(cd=n.BF16X3)):
        both(n.ENOSUPPORT, **ch)
    args = [base[k] for k in order]                              # and the same arguments unharmed are accepted
    assert lib.cor_gemm_kernel_id(*args) == 1 | n.GEMM_EPILOGUE_VEC
    assert lib.cor_gemm(*args, stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(c, torch.full_like(c, float(K)))

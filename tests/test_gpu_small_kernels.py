"""The small kernels of rows.hip, misc.hip and postproc.hip, each called directly through cor_amd.ops at the smallest shapes that reach
every tail of its decomposition, against the fp64 references and a-priori bounds of tests/small_kernel_refs.py (proved on the CPU by
tests/test_cpu_small_kernel_refs.py). Pure moves are bitwise. Every check leaves its error/bound ratio in the parity report (parity_util)."""
import numpy as np
import pytest
import torch

from tests import parity_util as pu
from tests import small_kernel_refs as R

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

DEV = "cuda:0"
F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
PAIRS = [(F32, F32), (F32, BF16), (BF16, F32), (BF16, BF16)]
SIZES = [((1, 1), (5, 7)), ((7, 5), (3, 2)), ((24, 24), (24, 24)), ((5, 9), (64, 48))]


def ops():
    from cor_amd import ops as o
    return o


def rnd(seed, *shape, lo=-1.0, hi=1.0, dtype=F32):
    """seeded numpy values, rounded to the kernel's input dtype: the reference widens exactly what the kernel reads"""
    r = np.random.default_rng(seed)
    return torch.from_numpy(r.uniform(lo, hi, size=shape).astype(np.float32)).to(dtype)


def g(t):
    return None if t is None else t.to(DEV)


def d(t):
    return None if t is None else t.to(F64)


def nm(dt):
    return "bf16" if dt == BF16 else "f32"


# ====================================================================================================== rows.hip
def _ln_inputs(rows, C, TI, seed=1):
    x = rnd(seed, rows, C, lo=-3, hi=3)
    if rows > 2:
        x[1] += 1e3                                              # mean 1e3, std ~1
        x[2] = 1.5                                               # constant row
    return x.to(TI), rnd(seed + 1, C), rnd(seed + 2, C, lo=0.25, hi=1)


@pytest.mark.parametrize("TI,TO", PAIRS)
@pytest.mark.parametrize("rows", [1, 9])
@pytest.mark.parametrize("C", [896, 1280, 260, 1156, 1536, 2048])   # half-wave NV 7, 10; wave-per-row nv 2, 5, 6 -> 8, 8 full
def test_layernorm(C, rows, TI, TO):
    x, w, b = _ln_inputs(rows, C, TI)
    ref, bound = R.layernorm(d(x), d(w), d(b), 1e-6)
    out = ops().layernorm(g(x), g(w), g(b), 1e-6, out_dtype=TO)
    pu.check(f"layernorm[{C},{rows},{nm(TI)}->{nm(TO)}]", out.cpu(), ref, bound)
    rev = ops().layernorm(g(x), g(w), g(b), 1e-6, out_dtype=TO, reverse=True)
    pu.check_bitwise(f"layernorm_reverse[{C},{rows},{nm(TI)}->{nm(TO)}]", rev.cpu(), out.cpu())
    if rows > 2 and TI == F32 and TO == F32:
        # 1.5 C and every partial sum of it are exact in fp32, so mean = 1.5, d = 0 and the row is b to the bit
        pu.check_bitwise(f"layernorm_constant_row[{C}]", out[2].cpu(), b)


@pytest.mark.parametrize("C", [896, 1156])
def test_layernorm_gelu(C):
    x, w, b = _ln_inputs(9, C, F32, seed=5)
    ref, bound = R.layernorm(d(x), d(w), d(b), 1e-6, act=1)
    out = ops().layernorm(g(x), g(w), g(b), 1e-6, act=ops().ACT_GELU_ERF)
    pu.check(f"layernorm_gelu[{C}]", out.cpu(), ref, bound)


@pytest.mark.parametrize("TI,TO", PAIRS)
@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("C", [1, 63, 64, 65, 768])
def test_l2norm_rows(C, rows, TI, TO):
    x = rnd(10, rows, C, lo=-2, hi=2)
    if rows > 2:
        x[1] = 0.0                                               # zero row -> zeros
        x[2] = x[2] / x[2].norm() * 1e-13                        # norm 1e-13 < eps: divided by eps
    x = x.to(TI)
    ref, bound = R.l2norm_rows(d(x))
    out = ops().l2norm_rows(g(x), out_dtype=TO)
    pu.check(f"l2norm_rows[{C},{rows},{nm(TI)}->{nm(TO)}]", out.cpu(), ref, bound)
    if rows > 2:
        assert float(out[1].float().abs().max()) == 0.0


@pytest.mark.parametrize("TA", [F32, BF16])
@pytest.mark.parametrize("TB", [F32, BF16])
@pytest.mark.parametrize("TO", [F32, BF16])
def test_add(TA, TB, TO):
    for tag, sa, sb in (("period=n", (6, 8), (6, 8)), ("period<n", (6, 8), (8,)), ("n=4", (4,), (4,))):
        a, b = rnd(20, *sa, lo=-4, hi=4, dtype=TA), rnd(21, *sb, lo=-4, hi=4, dtype=TB)
        ref, bound = R.add(d(a), d(b))
        out = ops().add(g(a), g(b), out_dtype=TO)
        pu.check(f"add[{nm(TA)}+{nm(TB)}->{nm(TO)},{tag}]", out.cpu(), ref, bound)


def _copy(src, ld_in, rows, C, TO, ld_out, src_offset=0):
    out = torch.full((rows, ld_out), -7.0, dtype=TO)
    got = ops().copy_rows(g(src), ld_in, rows, C, g(out), ld_out=ld_out, src_offset=src_offset).cpu()
    idx = src_offset + torch.arange(rows)[:, None] * ld_in + torch.arange(C)[None, :]
    want = out.clone()
    want[:, :C] = src[idx].to(TO)                                # torch's cast is round-to-nearest-even
    return got, want


@pytest.mark.parametrize("TI,TO", PAIRS)
def test_copy_rows(TI, TO):
    src = rnd(30, 200, lo=-9, hi=9, dtype=TI)
    for tag, ld_in, rows, C, ld_out, off in (("vec,ld8", 8, 5, 8, 8, 0), ("vec,ld12", 12, 5, 8, 12, 0), ("scalar,C6", 7, 5, 6, 9, 0),
                                            ("scalar,odd offset", 8, 5, 8, 8, 3), ("broadcast,vec", 0, 5, 8, 12, 0), ("broadcast,scalar", 0, 5, 6, 6, 1)):
        got, want = _copy(src, ld_in, rows, C, TO, ld_out, off)
        pu.check_bitwise(f"copy_rows[{nm(TI)}->{nm(TO)},{tag}]", got, want)


def test_copy_rows_f32_to_bf16_special_values():
    fmax = float(np.finfo(np.float32).max)
    v = torch.tensor([0.0, -0.0, float("inf"), -float("inf"), float("nan"), 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, fmax,
                      -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8), -fmax, 1 + 2.0 ** -8 + 2.0 ** -23, 1 + 2.0 ** -8 - 2.0 ** -23, 65504.0, 1e-30, -1e-30], dtype=F32)
    want = v.to(BF16)
    assert want[5].item() == 1.0 and want[6].item() == 1 + 2.0 ** -6 and torch.isinf(want[7]) and torch.isnan(want[4])   # ties to even, both ways
    src = torch.cat([torch.zeros(1), v])
    for tag, off in (("vec", 0), ("scalar", 1)):
        s = v if off == 0 else src
        out = torch.full((2, 8), -7.0, dtype=BF16)
        got = ops().copy_rows(g(s), 8, 2, 8, g(out), ld_out=8, src_offset=off).cpu()
        pu.check_bitwise(f"copy_rows_cast_special[{tag}]", got, want.reshape(2, 8))


@pytest.mark.parametrize("T", [F32, BF16])
@pytest.mark.parametrize("B,HW,C", [(1, 1, 1), (2, 33, 31), (3, 64, 32), (1, 31, 65)])
def test_token_layouts(B, HW, C, T):
    x = rnd(40, B, HW, C, lo=-9, hi=9, dtype=T)
    got = ops().tokens_to_nchw(g(x), B, HW, C).cpu()
    pu.check_bitwise(f"tokens_to_nchw[{B},{HW},{C},{nm(T)}]", got, R.tokens_to_nchw(x.float(), B, HW, C))
    n = rnd(41, B, C, HW, lo=-9, hi=9)
    got = ops().nchw_to_tokens(g(n), T).cpu()
    pu.check_bitwise(f"nchw_to_tokens[{B},{HW},{C},{nm(T)}]", got, R.nchw_to_tokens(n, B, HW, C).to(T))


@pytest.mark.parametrize("D", [4, 32])
def test_embed_tokens(D):
    N, ctx, vocab = 3, 5, 11
    r = np.random.default_rng(50)
    ids = torch.from_numpy(r.integers(0, vocab, size=(N, ctx)))
    ids[0, 1], ids[1, 4], ids[2, 0] = -1, vocab, 2 ** 40
    table, pos = rnd(51, vocab, D), rnd(52, ctx + 2, D)
    got = ops().embed_tokens(g(ids), g(table), g(pos)).cpu()
    flat = ids.reshape(-1)
    oob = (flat < 0) | (flat >= vocab)
    want = table[flat.clamp(0, vocab - 1)] + pos[torch.arange(N * ctx) % ctx]      # one correctly rounded fp32 add per element
    want[oob] = float("nan")
    assert int(oob.sum()) == 3
    pu.check_bitwise(f"embed_tokens[{D}]", got, want)
    assert bool(torch.isnan(got[oob]).all()) and not bool(torch.isnan(got[~oob]).any())


@pytest.mark.parametrize("T", [F32, BF16])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("p", [5, 6])
def test_patchify(p, C, T):
    img = rnd(60, 2, C, 17, 13, lo=-3, hi=3)                     # H, W no multiples of p
    K = C * p * p
    Kpad = K + (-K) % 4 + 4                                      # zero padding beyond K
    got = ops().patchify(g(img), p, Kpad, T).cpu()
    pu.check_bitwise(f"patchify[{p},{C},{nm(T)}]", got, R.patchify(img, p, Kpad).to(T))


@pytest.mark.parametrize("T", [F32, BF16])
@pytest.mark.parametrize("B,H,W,C", [(1, 1, 1, 8), (2, 1, 5, 4)])
def test_im2col3x3(B, H, W, C, T):
    x = rnd(70, B * H * W, C, lo=-3, hi=3, dtype=T)
    got = ops().im2col3x3(g(x), B, H, W).cpu()
    pu.check_bitwise(f"im2col3x3[{B},{H},{W},{C},{nm(T)}]", got, R.im2col3x3(x, B, H, W))


# ====================================================================================================== misc.hip
@pytest.mark.parametrize("src,dst", SIZES)
def test_bilinear(src, dst):
    x = rnd(80, 2, 3, *src, lo=-1, hi=2)                         # values outside [0, 1] for the clamp
    for clamp in (False, True):
        ref, bound = R.bilinear(d(x), *dst, clamp01=clamp)
        out = ops().bilinear(g(x), *dst, clamp01=clamp)
        pu.check(f"bilinear[{src}->{dst},clamp={int(clamp)}]", out.cpu(), ref, bound)


@pytest.mark.parametrize("H,W", [(1, 1), (2, 7), (7, 8), (8, 2)])
@pytest.mark.parametrize("Cout", [1, 5])
@pytest.mark.parametrize("Cin", [1, 3])
def test_conv3x3s2_small(Cin, Cout, H, W):
    B = 2
    x, w, bias = rnd(90, B, Cin, H, W), rnd(91, Cout, Cin, 3, 3), rnd(92, Cout)
    for b in (bias, None):
        ref, bound = R.conv3x3s2(d(x), d(w), d(b))
        for cl in (False, True):
            xin = x.permute(0, 2, 3, 1).contiguous() if cl else x
            out = ops().conv3x3s2_small(g(xin), cl, g(w), g(b), B, Cin, H, W)
            pu.check(f"conv3x3s2_small[{Cin},{Cout},{H}x{W},cl={int(cl)},bias={int(b is not None)}]", out.cpu(), ref, bound)


@pytest.mark.parametrize("TO", [F32, BF16])
@pytest.mark.parametrize("C", [4, 5])
@pytest.mark.parametrize("H,W", [(3, 2), (9, 11)])
def test_dwconv7x7(H, W, C, TO):
    B = 2
    x, w_t, bias = rnd(100, B * H * W, C), rnd(101, 49, C), rnd(102, C)
    ref, bound = R.dwconv7x7(d(x), d(w_t), d(bias), B, H, W)
    out = ops().dwconv7x7(g(x), g(w_t), g(bias), B, H, W, out_dtype=TO)
    pu.check(f"dwconv7x7[{H}x{W},{C},{nm(TO)}]", out.cpu(), ref, bound)


@pytest.mark.parametrize("M", [1, 3, 4, 5])
@pytest.mark.parametrize("P", [1, 63, 65, 257])
def test_adapter_pool(P, M):
    B = 2
    maps = rnd(110, B, P, M, lo=-30, hi=30)
    for D in (1, 255, 257):
        feat = rnd(111, B, P, D)
        ref, bound = R.adapter_pool(d(maps), d(feat))
        out = ops().adapter_pool(g(maps), g(feat), B, P, M, D)
        pu.check(f"adapter_pool[{P},{M},{D}]", out.cpu(), ref, bound)


@pytest.mark.parametrize("D", [1, 5, 256, 300])
@pytest.mark.parametrize("P", [1, 63, 257])
def test_masked_pool(P, D):
    B = 3
    feat = rnd(120, B, P, D)
    for clamp in (False, True):
        mask = rnd(121, B, P, lo=-0.5, hi=1.5) if clamp else rnd(122, B, P, lo=0, hi=1)
        mask[1] = 0.0                                            # an all-zero mask
        for l2 in (False, True):
            ref, bound = R.masked_pool(d(feat), d(mask), clamp01=clamp, l2norm=l2)
            for nchw in (False, True):
                f = feat.transpose(1, 2).contiguous() if nchw else feat
                out = ops().masked_pool(g(f), g(mask), B, P, D, feat_nchw=nchw, clamp01=clamp, l2norm=l2)
                pu.check(f"masked_pool[{P},{D},nchw={int(nchw)},clamp={int(clamp)},l2={int(l2)}]", out.cpu(), ref, bound)
                assert float(out[1].abs().max()) == 0.0


@pytest.mark.parametrize("D", [1, 63, 65, 768])
@pytest.mark.parametrize("N", [1, 3, 5])
def test_fuse_gate_and_mix(N, D):
    img, txt, aI, aT = rnd(130, N, D), rnd(131, N, D), rnd(132, N, D, lo=0, hi=1), rnd(133, N, D, lo=0, hi=1)
    if N > 2:
        img[2] = 0.0                                             # a zero row
        txt[2] = 0.0
    ref, bound = R.fuse_gate(d(img), d(txt), d(aI), d(aT))
    cat = ops().fuse_gate(g(img), g(txt), g(aI), g(aT))
    pu.check(f"fuse_gate[{N},{D}]", cat.cpu(), ref, bound)
    dyn = torch.tensor([0.0, 1.0, 0.3, 0.3, 0.3][:N] if N > 1 else [0.3], dtype=F32)
    ref, bound = R.fuse_mix(d(cat.cpu()), d(dyn))                # the kernel's own input, widened
    out = ops().fuse_mix(cat, g(dyn))
    pu.check(f"fuse_mix[{N},{D}]", out.cpu(), ref, bound)
    for a in ([0.0], [1.0]):                                     # dyn = 0 / 1 on every row
        dyn1 = torch.tensor(a * N, dtype=F32)
        ref, bound = R.fuse_mix(d(cat.cpu()), d(dyn1))
        pu.check(f"fuse_mix[{N},{D},dyn={a[0]}]", ops().fuse_mix(cat, g(dyn1)).cpu(), ref, bound)


@pytest.mark.parametrize("F", [1, 5, 128])
@pytest.mark.parametrize("size", [1, 3, 16])
def test_dense_pe(size, F):
    G = torch.from_numpy(np.random.default_rng(140).standard_normal((2, F)).astype(np.float32))
    ref, bound = R.dense_pe(d(G), size)
    pu.check(f"dense_pe[{size},{F}]", ops().dense_pe(g(G), size).cpu(), ref, bound)


@pytest.mark.parametrize("TI,TO", PAIRS)
@pytest.mark.parametrize("C,B,H,W", [(1, 2, 2, 3), (63, 2, 2, 3), (65, 2, 2, 3), (256, 2, 2, 3), (64, 1, 1, 3), (64, 1, 3, 3)])   # C = 64: 12 / 36 pixels, no multiple of 16
def test_upscale_shuffle(C, B, H, W, TI, TO):
    y = rnd(150, B * H * W, 4 * C, lo=-2, hi=2, dtype=TI)
    bias, lw, lb = rnd(151, C), rnd(152, C, lo=0.25, hi=1), rnd(153, C)
    for b in (None, bias):
        for ln in (False, True):
            for act in range(5):
                ref, bound = R.upscale_shuffle(d(y), B, H, W, C, d(b), d(lw) if ln else None, d(lb) if ln else None, 1e-6, act)
                out = ops().upscale_shuffle(g(y), B, H, W, C, bias=g(b), ln_w=g(lw) if ln else None, ln_b=g(lb) if ln else None, eps=1e-6, act=act,
                                            out_dtype=TO)
                pu.check(f"upscale_shuffle[{C},{B * 4 * H * W}px,{nm(TI)}->{nm(TO)},bias={int(b is not None)},ln={int(ln)},act={act}]", out.cpu(), ref, bound)


@pytest.mark.parametrize("T", [F32, BF16])
@pytest.mark.parametrize("B,H,W,K", [(1, 1, 1, 1), (2, 5, 7, 3), (1, 16, 17, 4), (2, 3, 3, 5), (1, 2, 2, 16)])
def test_upscale_hyper(B, H, W, K, T):
    x = rnd(160, B * H * W, 64, lo=-2, hi=2, dtype=T)
    w, bias = rnd(161, 64, 32, 2, 2, lo=-0.2, hi=0.2), rnd(162, 32)
    hyper_all = g(rnd(163, B, K + 2, 32))
    hyper = hyper_all[:, 1:1 + K]                                # the strided view the decoder passes
    ref, bound = R.upscale_hyper(d(x), d(w), d(bias), d(hyper.cpu()), B, H, W)
    out = ops().upscale_hyper(g(x), g(w), g(bias), hyper, B, H, W, K)
    pu.check(f"upscale_hyper[{B},{H},{W},{K},{nm(T)}]", out.cpu(), ref, bound)


@pytest.mark.parametrize("C", [1, 32, 100])
@pytest.mark.parametrize("k_off,Ksel", [(0, 1), (1, 3), (0, 4)])
def test_iou_select(k_off, Ksel, C):
    inf = float("inf")
    iou = torch.tensor([[0.1, 0.7, 0.3, 0.9], [0.5, 0.5, 0.5, 0.5], [0.2, inf, inf, 0.1], [-inf, -inf, 0.0, -inf], [-inf, -inf, -inf, -inf],
                        [0.9, 0.2, 0.8, 0.8]], dtype=F32)
    B = iou.shape[0]
    hyper = rnd(170, B, 4, C)
    best, sel = ops().iou_select(g(iou), g(hyper), k_off, Ksel)
    want = torch.from_numpy(np.argmax(iou[:, k_off:k_off + Ksel].numpy(), axis=1))      # the first maximum
    pu.check_bitwise(f"iou_select_best[{k_off},{Ksel},{C}]", best.cpu(), want)
    pu.check_bitwise(f"iou_select_rows[{k_off},{Ksel},{C}]", sel.cpu(), hyper[torch.arange(B), k_off + want].reshape(B, 1, C))


# ====================================================================================================== postproc.hip
@pytest.mark.parametrize("HW", [1, 255, 257, 4096])
def test_mask_prob_minmax(HW):
    x = rnd(180, 3, HW, lo=-6, hi=6)
    x[1] = 0.25                                                  # a constant plane
    if HW > 2:
        x[2, 0], x[2, HW // 2] = 100.0, -100.0
    ref, bound = R.mask_prob_minmax(d(x))
    out = ops().mask_prob_minmax(g(x.reshape(3, 1, 1, HW))).cpu().reshape(3, HW)
    pu.check(f"mask_prob_minmax[{HW}]", out, ref, bound)
    assert float(out[1].abs().max()) == 0.0                      # p - min is the same expression twice: exactly 0
    if HW > 2:
        assert float(out[2].max()) == 1.0 and float(out[2].min()) == 0.0


@pytest.mark.parametrize("src,dst", SIZES + [((256, 256), (1024, 1024))])    # the last: 4096 blocks of work on a grid capped at 2048
def test_resize_binarize_and_gray(src, dst):
    B = 1 if dst[0] > 100 else 3
    p = rnd(190, B, 1, *src, lo=0, hi=1)
    v = R.bilinear(d(p), *dst)[0].reshape(B, *dst)
    for thr in (0.5, 0.25):
        out = ops().resize_binarize(g(p), *dst, threshold=thr).cpu()
        pu.check_decision(f"resize_binarize[{src}->{dst},{thr}]", out, v, R.binarize_decide(thr), R.binarize_margin(thr))
        assert set(np.unique(out.numpy()).tolist()) <= {0, 255}
    out = ops().resize_gray(g(p), *dst).cpu()
    pu.check_decision(f"resize_gray[{src}->{dst}]", out, v, R.gray_decide, R.gray_margin, slack=1)


@pytest.mark.parametrize("HW", [1, 255, 4096, 65536, 1048576])
def test_mask_metrics(HW):
    r = np.random.default_rng(200)
    soft = torch.from_numpy(r.uniform(0, 1, HW).astype(np.float32))
    gtb = torch.from_numpy((r.uniform(0, 1, HW) > 0.6).astype(np.float32))
    pred = torch.stack([soft, soft, soft, gtb])
    gt = torch.stack([gtb, torch.ones(HW), torch.zeros(HW), gtb])        # binary gt, all ones, all zeros, pred = gt hard
    ref, bound = R.mask_metrics(d(pred), d(gt))
    out = ops().mask_metrics(g(pred), g(gt)).cpu()
    pu.check(f"mask_metrics[{HW}]", out, ref, bound)


def sharp_case(hw, nbg, seed):
    """ground truth all foreground but nbg pixels, a sharp prediction: p in [0.9999, 1] on foreground, [0, 0.0001] on background"""
    r = np.random.default_rng(seed)
    gt = np.ones(hw, np.float32)
    gt[r.choice(hw, nbg, replace=False)] = 0.0
    p = np.where(gt > 0, r.uniform(0.9999, 1.0, hw), r.uniform(0.0, 0.0001, hw)).astype(np.float32)
    return torch.from_numpy(p)[None], torch.from_numpy(gt)[None]


@pytest.mark.parametrize("hw,nbg", [(256 * 256, 10), (1024 * 1024, 1000), (1024 * 1024, 10)])
def test_mask_metrics_sharp_near_full_foreground(hw, nbg):
    """With the background sums formed as n - ps - gs + pg (before the fix) mdice / miou miss this bound by orders of magnitude."""
    pred, gt = sharp_case(hw, nbg, 50)
    ref, bound = R.mask_metrics(d(pred), d(gt))
    out = ops().mask_metrics(g(pred), g(gt)).cpu()
    print(f"mask_metrics sharp hw={hw} nbg={nbg}: got {out[0].tolist()} ref {ref[0].tolist()} abs err {(d(out) - ref).abs()[0].tolist()}")
    pu.check(f"mask_metrics_sharp[{hw},{nbg}]", out, ref, bound)


# ====================================================================================================== past the grid-stride block caps
def test_past_cap_add():
    n = 4 * (4096 * 256 + 3)
    a, b = rnd(210, n, lo=-4, hi=4), rnd(211, n, lo=-4, hi=4)
    ref, bound = R.add(d(a), d(b))
    pu.check("past_cap_add", ops().add(g(a), g(b)).cpu(), ref, bound)


def test_past_cap_copy_rows():
    rows, C = 4096 * 128 + 2, 8                                  # rows * C / 4 = 4096 * 256 + 4 vectors
    src = rnd(212, rows * C, lo=-9, hi=9)
    got, want = _copy(src, C, rows, C, BF16, C)
    pu.check_bitwise("past_cap_copy_rows", got, want)


def test_past_cap_bilinear():
    x = rnd(213, 1, 3, 5, 9, lo=-1, hi=2)
    assert 3 * 840 * 840 > 8192 * 256
    ref, bound = R.bilinear(d(x), 840, 840)
    pu.check("past_cap_bilinear", ops().bilinear(g(x), 840, 840).cpu(), ref, bound)


def test_past_cap_fuse_gate():
    N, D = 2731, 768
    assert N * D > 8192 * 256
    img, txt, aI, aT = rnd(214, N, D), rnd(215, N, D), rnd(216, N, D, lo=0, hi=1), rnd(217, N, D, lo=0, hi=1)
    ref, bound = R.fuse_gate(d(img), d(txt), d(aI), d(aT))
    pu.check("past_cap_fuse_gate", ops().fuse_gate(g(img), g(txt), g(aI), g(aT)).cpu(), ref, bound)


def test_past_cap_dense_pe():
    G = torch.from_numpy(np.random.default_rng(218).standard_normal((2, 129)).astype(np.float32))
    assert 128 * 128 * 129 > 8192 * 256
    ref, bound = R.dense_pe(d(G), 128)
    pu.check("past_cap_dense_pe", ops().dense_pe(g(G), 128).cpu(), ref, bound)


def test_past_cap_dwconv7x7_vec4():
    B, H, W, C = 2, 92, 92, 496
    assert B * H * W * (C // 4) > 8192 * 256 and C % 4 == 0
    x, w_t, bias = rnd(219, B * H * W, C), rnd(220, 49, C), rnd(221, C)
    ref, bound = R.dwconv7x7(d(x), d(w_t), d(bias), B, H, W)
    pu.check("past_cap_dwconv7x7_vec4", ops().dwconv7x7(g(x), g(w_t), g(bias), B, H, W).cpu(), ref, bound)


def test_past_cap_conv3x3s2_small():
    B, Cin, Cout, H, W = 1, 1, 5, 1296, 1296
    assert B * 648 * 648 * Cout > 8192 * 256
    x, w, bias = rnd(222, B, Cin, H, W), rnd(223, Cout, Cin, 3, 3), rnd(224, Cout)
    ref, bound = R.conv3x3s2(d(x), d(w), d(bias))
    pu.check("past_cap_conv3x3s2_small", ops().conv3x3s2_small(g(x), False, g(w), g(bias), B, Cin, H, W).cpu(), ref, bound)


# ====================================================================================================== refusals (rejected by the C entry point before any launch)
def test_refusals():
    o = ops()
    z = lambda *s, dt=F32: torch.zeros(s, dtype=dt, device=DEV)     # noqa: E731
    with pytest.raises(RuntimeError):
        o.add(z(6), z(6))                                        # n % 4 != 0
    with pytest.raises(RuntimeError):
        o.layernorm(z(2, 6), z(6), z(6), 1e-6)                   # C % 4 != 0
    with pytest.raises(RuntimeError):
        o.layernorm(z(2, 2052), z(2052), z(2052), 1e-6)          # nine vectors per lane: no kernel
    with pytest.raises(RuntimeError):
        o.upscale_shuffle(z(2, 4 * 257), 1, 1, 2, 257)           # Cout > 256
    with pytest.raises(RuntimeError):
        o.upscale_hyper(z(4, 64), z(64, 32, 2, 2), z(32), z(1, 17, 32), 1, 2, 2, 17)   # Kmask > 16
    with pytest.raises(RuntimeError):
        o.iou_select(z(2, 4), z(2, 4, 8), 2, 3)                  # k_off + Ksel > Kall
    with pytest.raises(RuntimeError):
        o.adapter_pool(z(1, 4096, 4), z(1, 4096, 8), 1, 4096, 4, 8)     # (P M + P + 2M) floats > 64 KB of LDS
    with pytest.raises(RuntimeError):
        o.masked_pool(z(1, 16384, 8), z(1, 16384), 1, 16384, 8)  # (P + D + 8) floats > 64 KB of LDS
    torch.cuda.synchronize()

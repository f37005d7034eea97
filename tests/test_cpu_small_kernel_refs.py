"""CPU proof of the fp64 references, the bounds and the comparator that tests/test_gpu_small_kernels.py holds the small kernels to:
(1) every reference equals torch's own fp64 operator where one exists, (2) a plain fp32 CPU evaluation of each operation passes the
comparator under the derived bound, (3) deliberately wrong fp32 results are rejected. No kernel runs here."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import retrieval as oret, support as osup
from tests import parity_util as pu
from tests import small_kernel_refs as R

torch.set_grad_enabled(False)
F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16


def rnd(seed, *shape, lo=-1.0, hi=1.0):
    """fp32-representable values as fp64 (what a kernel and its reference both see)"""
    r = np.random.default_rng(seed)
    return torch.from_numpy(r.uniform(lo, hi, size=shape).astype(np.float32)).to(F64)


def close64(a, b, tol=1e-12):
    assert a.shape == b.shape, (a.shape, b.shape)
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max())), float((a - b).abs().max())


def f32_passes(name, fn, *args, **kw):
    """fn in fp64 = reference + bound; fn in fp32 = a plain fp32 evaluation: it must lie inside the bound."""
    ref, bound = fn(*args, **kw)
    lo = [a.to(F32) if isinstance(a, torch.Tensor) and a.is_floating_point() else a for a in args]
    got = fn(*lo, **{k: (v.to(F32) if isinstance(v, torch.Tensor) and v.is_floating_point() else v) for k, v in kw.items()})[0]
    assert got.dtype == F32
    rec = pu.check("cpu:" + name, got, ref, bound, report=False)
    bf = pu.check("cpu:" + name + ":bf16", got.to(BF16), ref, bound, report=False)      # a correctly rounded bf16 store stays inside too
    return rec, bf


def rejected(got, ref, bound, **kw):
    rec, fails = pu.compare(got, ref, bound, **kw)
    assert fails and rec["max_ratio"] > 1.0, rec


# ====================================================================================================== the comparator itself
def test_bf16_rne_equals_torch_rounding():
    r = np.random.default_rng(0)
    x = np.concatenate([r.standard_normal(20000).astype(np.float32) * np.float32(10.0) ** r.integers(-30, 30, 20000).astype(np.float32),
                        np.array([0.0, -0.0, 1.0, 1.00390625, 1.01171875, 3.3895314e38, 3.4028235e38, -3.4028235e38, 1e-40, 9.2e-41], np.float32)])
    want = torch.from_numpy(x).to(BF16).to(F64).numpy()
    np.testing.assert_array_equal(pu.bf16_rne(x.astype(np.float64)), want)
    # a tie in fp64 that fp32 would break first: 1 + 2^-8 + 2^-40 rounds UP in one step
    assert pu.bf16_rne(np.array([1.0 + 2.0 ** -8 + 2.0 ** -40]))[0] == 1.0 + 2.0 ** -7
    assert pu.bf16_rne(np.array([1.0 + 2.0 ** -8]))[0] == 1.0


def test_comparator_policies():
    ref = torch.tensor([1.0, 2.0, float("nan"), float("inf")], dtype=F64)
    b = torch.full((4,), 1e-6, dtype=F64)
    ok = torch.tensor([1.0, 2.0 + 5e-7, float("nan"), float("inf")], dtype=F32)
    pu.check("p", ok, ref, b, nonfinite="agree", report=False)
    with pytest.raises(AssertionError):
        pu.check("p", ok, ref, b, nonfinite="finite", report=False)
    for bad in ([1.0, 2.0, 0.0, float("inf")], [1.0, 2.0, float("nan"), -float("inf")], [float("nan"), 2.0, float("nan"), float("inf")],
                [1.0, 2.00001, float("nan"), float("inf")]):
        with pytest.raises(AssertionError):
            pu.check("p", torch.tensor(bad, dtype=F32), ref, b, nonfinite="agree", report=False)
    # bf16: the interval is [rne(ref - b), rne(ref + b)], not a blanket ulp
    r1, b1 = torch.tensor([1.0 + 2.0 ** -9], dtype=F64), torch.tensor([1e-9], dtype=F64)
    pu.check("b", torch.tensor([1.0], dtype=BF16), r1, b1, report=False)
    rejected(torch.tensor([1.0 + 2.0 ** -7], dtype=BF16), r1, b1)
    # bitwise: NaN by NaN-ness, zeros by sign
    pu.check_bitwise("w", torch.tensor([float("nan"), 0.0], dtype=F32), torch.tensor([float("nan"), 0.0], dtype=F32), report=False)
    assert pu.compare_bitwise(torch.tensor([0.0]), torch.tensor([-0.0]))[1]
    assert pu.compare_bitwise(torch.tensor([1.0], dtype=BF16), torch.tensor([1.0078125], dtype=BF16))[1]
    # decisions
    v = np.array([0.5 + 2e-6, 0.7, 0.2])
    assert not pu.compare_decision(np.array([0, 255, 0]), v, R.binarize_decide(0.5), R.binarize_margin(0.5))[1]
    assert pu.compare_decision(np.array([255, 0, 0]), v, R.binarize_decide(0.5), R.binarize_margin(0.5))[1]
    g = np.array([100.0004 / 255.0, 17.5 / 255.0])
    assert not pu.compare_decision(np.array([99, 17]), g, R.gray_decide, R.gray_margin, slack=1)[1]
    assert pu.compare_decision(np.array([98, 17]), g, R.gray_decide, R.gray_margin, slack=1)[1]
    assert pu.compare_decision(np.array([100, 16]), g, R.gray_decide, R.gray_margin, slack=1)[1]


# ====================================================================================================== references == torch fp64 operators
SIZES = [((1, 1), (5, 7)), ((7, 5), (3, 2)), ((24, 24), (24, 24)), ((5, 9), (64, 48))]


@pytest.mark.parametrize("src,dst", SIZES)
def test_bilinear_reference(src, dst):
    x = rnd(1, 2, 3, *src, lo=-2, hi=2)
    ref, _ = R.bilinear(x, *dst)
    close64(ref, F.interpolate(x, size=dst, mode="bilinear", align_corners=False))
    close64(ref, osup.bilinear_resize(x, *dst))
    f32_passes("bilinear", R.bilinear, x, *dst)
    f32_passes("bilinear_clamp", R.bilinear, x, *dst, clamp01=True)
    close64(R.bilinear(x, *dst, clamp01=True)[0], ref.clamp(0, 1))


@pytest.mark.parametrize("Cin,Cout,H,W", [(1, 1, 1, 1), (3, 5, 2, 7), (3, 1, 8, 8), (1, 5, 7, 2)])
def test_conv3x3s2_reference(Cin, Cout, H, W):
    x, w, b = rnd(2, 2, Cin, H, W), rnd(3, Cout, Cin, 3, 3), rnd(4, Cout)
    for bias in (b, None):
        close64(R.conv3x3s2(x, w, bias)[0], F.conv2d(x, w, bias, stride=2, padding=1).permute(0, 2, 3, 1))
        f32_passes("conv3x3s2", R.conv3x3s2, x, w, bias)


@pytest.mark.parametrize("H,W,C", [(3, 2, 4), (9, 11, 5)])
def test_dwconv7x7_reference(H, W, C):
    x, w_t, b = rnd(5, 2, H, W, C), rnd(6, 49, C), rnd(7, C)
    want = F.conv2d(x.permute(0, 3, 1, 2), w_t.t().reshape(C, 1, 7, 7), b, padding=3, groups=C).permute(0, 2, 3, 1).reshape(-1, C)
    close64(R.dwconv7x7(x, w_t, b, 2, H, W)[0], want)
    f32_passes("dwconv7x7", R.dwconv7x7, x, w_t, b, 2, H, W)


@pytest.mark.parametrize("C", [4, 260, 896, 1280, 2048])
@pytest.mark.parametrize("act", [0, 1])
def test_layernorm_reference(C, act):
    x, w, b = rnd(8, 9, C, lo=-3, hi=3), rnd(9, C), rnd(10, C)
    x[1] = x[1] + 1e3                                            # mean 1e3, spread ~1
    x[2] = 1.5                                                   # constant row: the output is b
    x = x.to(F32).to(F64)
    ref, bound = R.layernorm(x, w, b, 1e-6, act)
    want = F.layer_norm(x, (C,), w, b, 1e-6)
    close64(ref, F.gelu(want) if act else want, 1e-9)
    if act == 0:
        close64(ref[2], b, 1e-15)
    f32_passes(f"layernorm{C}", R.layernorm, x, w, b, 1e-6, act)


def test_activation_references_and_erf_as():
    y = torch.linspace(-9, 9, 4001, dtype=F64).to(F32).to(F64)
    close64(R.act_ref(y, 1), F.gelu(y))
    close64(R.act_ref(y, 4), F.gelu(y, approximate="tanh"))
    close64(R.act_ref(y, 3), torch.sigmoid(y))
    close64(R.act_ref(y, 2), F.relu(y))
    for act in (1, 2, 3, 4):
        pu.check(f"cpu:act{act}", R.act_ref(y.to(F32), act), R.act_ref(y, act), R.MARGIN * R.act_err(y, torch.zeros_like(y), act), report=False)
    # the kernels' erf (Abramowitz-Stegun 7.1.26, common.h erf_as) evaluated in fp32 stays inside the GELU bound
    x = y.to(F32).numpy()
    t = (np.float32(0.70710678118654752440) * x).astype(np.float32)
    ax = np.abs(t)
    tt = (np.float32(1) / (np.float32(0.3275911) * ax + np.float32(1))).astype(np.float32)
    p = np.float32(1.061405429) * tt + np.float32(-1.453152027)
    for c in (1.421413741, -0.284496736, 0.254829592):
        p = (p * tt + np.float32(c)).astype(np.float32)
    e = np.exp2((np.float32(-1.4426950408889634) * ax * ax).astype(np.float32)).astype(np.float32)
    erf = np.copysign((np.float32(1) - p * tt * e).astype(np.float32), t)
    g = (np.float32(0.5) * x * (np.float32(1) + erf)).astype(np.float32)
    pu.check("cpu:gelu_erf_as", torch.from_numpy(g), R.act_ref(y, 1), R.MARGIN * R.act_err(y, torch.zeros_like(y), 1), report=False)


@pytest.mark.parametrize("C", [1, 63, 64, 65, 768])
def test_l2norm_reference(C):
    x = rnd(11, 5, C, lo=-2, hi=2)
    x[1] = 0.0
    x[2] = (x[2] / x[2].norm() * 1e-13).to(F32).to(F64)
    ref, _ = R.l2norm_rows(x)
    close64(ref, F.normalize(x, dim=-1, eps=1e-12))
    assert float(ref[1].abs().max()) == 0.0
    close64(ref[2], x[2] / 1e-12)
    f32_passes("l2norm", R.l2norm_rows, x)


def test_layout_references():
    x = rnd(12, 2, 33, 31)
    assert torch.equal(R.tokens_to_nchw(x, 2, 33, 31), x.transpose(1, 2))
    assert torch.equal(R.nchw_to_tokens(x.transpose(1, 2).contiguous(), 2, 33, 31), x.reshape(66, 31))
    img = rnd(13, 2, 3, 17, 13)
    for p in (5, 6):
        gh, gw, K = 17 // p, 13 // p, 3 * p * p
        want = F.unfold(img[:, :, :gh * p, :gw * p], p, stride=p).transpose(1, 2).reshape(2 * gh * gw, K)
        got = R.patchify(img, p, K + 4 + (-K) % 4)
        assert torch.equal(got[:, :K], want) and float(got[:, K:].abs().max()) == 0.0
    t = rnd(14, 2, 1, 5, 4)                                      # [B,H,W,C]
    want = F.unfold(t.permute(0, 3, 1, 2), 3, padding=1).reshape(2, 4, 9, 5).permute(0, 3, 2, 1).reshape(10, 36)
    assert torch.equal(R.im2col3x3(t.reshape(10, 4), 2, 1, 5), want)


def test_upscale_references():
    B, H, W, C = 2, 3, 5, 7
    x, w, b = rnd(15, B, H, W, 11), rnd(16, 11, C, 2, 2), rnd(17, C)
    y = torch.einsum("bhwi,iopq->bhwpqo", x, w).reshape(B * H * W, 4 * C)                  # the GEMM output the shuffle kernel reads
    ct = F.conv_transpose2d(x.permute(0, 3, 1, 2), w, b, stride=2).permute(0, 2, 3, 1).reshape(-1, C)
    close64(R.upscale_shuffle(y, B, H, W, C, bias=b)[0], ct)
    lw, lb = rnd(18, C), rnd(19, C)
    yq = y.to(F32).to(F64)                                       # an fp32 evaluation needs fp32-representable inputs
    for act in range(5):
        want = R.act_ref(F.layer_norm(ct, (C,), lw, lb, 1e-6), act)
        close64(R.upscale_shuffle(y, B, H, W, C, b, lw, lb, 1e-6, act)[0], want, 1e-9)
        f32_passes("upscale_shuffle", R.upscale_shuffle, yq, B, H, W, C, b, lw, lb, 1e-6, act)
        f32_passes("upscale_shuffle_noln", R.upscale_shuffle, yq, B, H, W, C, None, None, None, 1e-6, act)
    x2, w2, b2, hy = rnd(20, B * H * W, 64), rnd(21, 64, 32, 2, 2, lo=-.2, hi=.2), rnd(22, 32), rnd(23, B, 3, 32)
    ct2 = F.gelu(F.conv_transpose2d(x2.reshape(B, H, W, 64).permute(0, 3, 1, 2), w2, b2, stride=2))
    close64(R.upscale_hyper(x2, w2, b2, hy, B, H, W)[0], torch.einsum("bko,bohw->bkhw", hy, ct2))
    f32_passes("upscale_hyper", R.upscale_hyper, x2, w2, b2, hy, B, H, W)


def test_pool_and_fuse_references():
    B, P, M, D = 2, 65, 3, 9
    maps, feat = rnd(24, B, P, M, lo=-30, hi=30), rnd(25, B, P, D)
    a = torch.softmax(F.logsigmoid(maps.transpose(1, 2)), dim=-1)                          # oracle/support.mask_adapter_pooling
    close64(R.adapter_pool(maps, feat)[0], (a @ feat).mean(1))
    f32_passes("adapter_pool", R.adapter_pool, maps, feat)
    mask = rnd(26, B, P, lo=-.5, hi=1.5)
    mask[1] = 0.0
    m01 = mask.clamp(0, 1)
    want = osup.masked_pooling(feat.transpose(1, 2).reshape(B, D, P, 1), m01.reshape(B, 1, P, 1))
    close64(R.masked_pool(feat, mask, clamp01=True)[0], want)
    close64(R.masked_pool(feat, mask, clamp01=True, l2norm=True)[0], F.normalize(want, dim=1))
    assert float(R.masked_pool(feat, mask, True, True)[0][1].abs().max()) == 0.0
    for l2 in (False, True):
        f32_passes("masked_pool", R.masked_pool, feat, mask, clamp01=True, l2norm=l2)
        f32_passes("masked_pool", R.masked_pool, feat, m01, clamp01=False, l2norm=l2)
    img, txt, aI, aT = rnd(27, 5, 65), rnd(28, 5, 65), rnd(29, 5, 65, lo=0, hi=1), rnd(30, 5, 65, lo=0, hi=1)
    img[3] = 0.0
    txt[3] = 0.0
    cat, _ = R.fuse_gate(img, txt, aI, aT)
    dyn = torch.tensor([0.0, 1.0, 0.3, 0.3, 0.7], dtype=F32).to(F64)
    close64(R.fuse_mix(cat, dyn)[0], F.normalize(dyn[:, None] * aI * img + (1 - dyn[:, None]) * aT * txt))
    f32_passes("fuse_gate", R.fuse_gate, img, txt, aI, aT)
    f32_passes("fuse_mix", R.fuse_mix, cat.to(F32).to(F64), dyn)
    f32_passes("add", R.add, rnd(31, 6, 8), rnd(32, 8))


def test_dense_pe_reference():
    G = rnd(33, 2, 5, lo=-3, hi=3)
    for size in (1, 3, 16):
        ref, _ = R.dense_pe(G, size)
        c = 2 * ((torch.arange(size, dtype=F64) + 0.5) / size) - 1
        yy, xx = torch.meshgrid(c, c, indexing="ij")
        ang = 2 * math.pi * (torch.stack([xx, yy], -1) @ G)                                 # PositionEmbeddingRandom: coords (x, y) @ G
        close64(ref, torch.cat([ang.sin(), ang.cos()], -1).reshape(size * size, 10))
        f32_passes("dense_pe", R.dense_pe, G, size)


def test_postproc_references():
    x = rnd(34, 3, 257, lo=-6, hi=6)
    x[1] = 0.25
    x[2, :2] = torch.tensor([100.0, -100.0], dtype=F64)
    ref, _ = R.mask_prob_minmax(x)
    want = oret.postprocess_masks(x.reshape(3, 1, 1, 257))[1].reshape(3, 257)
    close64(ref, want)
    assert float(ref[1].abs().max()) == 0.0
    f32_passes("mask_prob_minmax", R.mask_prob_minmax, x)
    p, g = rnd(35, 2, 4096, lo=0, hi=1), (rnd(36, 2, 4096, lo=0, hi=1) > 0.6).to(F64)
    close64(R.mask_metrics(p, g)[0], oret.mask_metrics(p, g).to(F64), 1e-5)                 # the oracle evaluates in fp32
    f32_passes("mask_metrics", R.mask_metrics, p, g)


# ====================================================================================================== wrong results are rejected
def test_wrong_bilinear_tap_is_rejected():
    x = rnd(40, 1, 2, 5, 9)
    ref, bound = R.bilinear(x, 64, 48)
    x0 = torch.roll(x, 1, dims=3)                                # every x tap index off by one
    rejected(R.bilinear(x0.to(F32), 64, 48)[0], ref, bound)


def test_dropped_last_element_of_a_reduction_is_rejected():
    x, w, b = rnd(41, 3, 896, lo=-3, hi=3), rnd(42, 896), rnd(43, 896)
    ref, bound = R.layernorm(x, w, b, 1e-6)
    xs = x.to(F32)
    mean = xs[:, :-1].sum(1, keepdim=True) / 896                 # the last element never enters the mean
    d = xs - mean
    bad = d / torch.sqrt((d * d).mean(1, keepdim=True) + 1e-6) * w.to(F32) + b.to(F32)
    rejected(bad, ref, bound)
    ref, bound = R.l2norm_rows(x[:, :65])
    rejected(xs[:, :65] / xs[:, :64].norm(dim=1, keepdim=True), ref, bound)
    feat, mask = rnd(44, 2, 63, 5), rnd(45, 2, 63, lo=0, hi=1)
    ref, bound = R.masked_pool(feat, mask)
    f, m = feat.to(F32), mask.to(F32)
    rejected(torch.einsum("bp,bpd->bd", m[:, :-1], f[:, :-1]) / (m.sum(1, keepdim=True) + 1e-8), ref, bound)


def test_swapped_pixel_shuffle_is_rejected():
    B, H, W, C = 1, 3, 5, 7
    y = rnd(46, B * H * W, 4 * C)
    ref, bound = R.upscale_shuffle(y, B, H, W, C)
    bad = y.to(F32).reshape(B, H, W, 2, 2, C).permute(0, 1, 4, 2, 3, 5).reshape(B * 4 * H * W, C)   # dx where dy belongs
    rejected(bad, ref, bound)
    rec, fails = pu.compare_bitwise(bad, ref.to(F32))
    assert fails


def test_missing_tail_row_is_rejected():
    a, b = rnd(47, 9, 8), rnd(48, 8)
    ref, bound = R.add(a, b)
    bad = ref.to(F32).clone()
    bad[-1] = 0.0                                                # the last row never written
    rejected(bad, ref, bound)
    x = rnd(49, 9, 6)
    bad = x.to(F32).clone()
    bad[-1] = 0.0
    assert pu.compare_bitwise(bad, x.to(F32))[1]


def sharp_case(hw, nbg, seed):
    """ground truth all foreground but nbg pixels, a sharp prediction: p in [0.9999, 1] on foreground, [0, 0.0001] on background"""
    r = np.random.default_rng(seed)
    g = np.ones(hw, np.float32)
    g[r.choice(hw, nbg, replace=False)] = 0.0
    p = np.where(g > 0, r.uniform(0.9999, 1.0, hw), r.uniform(0.0, 0.0001, hw)).astype(np.float32)
    return p, g


def emulate_mask_metrics(p, g, algebra, smooth=np.float32(1e-5)):
    """The kernel's fp32 arithmetic on one sample: 256 strided partial sums, an xor tree per wave, four waves added in order.
    algebra=True: the background sums as n - ps - gs + pg, n - ps, n - gs (before the fix); False: summed element by element."""
    f = np.float32
    hw = p.size
    pad = (-hw) % 256

    def block_sum(v):
        v = np.concatenate([v.astype(f), np.zeros(pad, f)]).reshape(-1, 256)
        acc = np.zeros(256, f)
        for row in v:
            acc = (acc + row).astype(f)
        lanes = np.arange(256)
        for o in (32, 16, 8, 4, 2, 1):
            acc = (acc + acc[lanes ^ o]).astype(f)
        return f(f(f(acc[0] + acc[64]) + acc[128]) + acc[192])

    pg, ps, gs, ad = block_sum(p * g), block_sum(p), block_sum(g), block_sum(np.abs(p - g))
    n = f(hw)
    if algebra:
        bpg, bps, bgs = f(f(f(n - ps) - gs) + pg), f(n - ps), f(n - gs)
    else:
        na, nb = (f(1) - p).astype(f), (f(1) - g).astype(f)
        bpg, bps, bgs = block_sum(na * nb), block_sum(na), block_sum(nb)
    dice = f(f(f(2) * pg + smooth) / f(f(ps + gs) + smooth))
    iou = f(f(pg + smooth) / f(f(f(ps + gs) - pg) + smooth))
    bdice = f(f(f(2) * bpg + smooth) / f(f(bps + bgs) + smooth))
    biou = f(f(bpg + smooth) / f(f(f(bps + bgs) - bpg) + smooth))
    return torch.tensor([[dice, f(ad / n), iou, f(f(0.5) * f(dice + bdice)), f(f(0.5) * f(iou + biou))]], dtype=F32)


SHARP = [(256 * 256, 10), (1024 * 1024, 1000), (1024 * 1024, 10)]


@pytest.mark.parametrize("hw,nbg", SHARP)
def test_mask_metrics_background_algebra_is_rejected_and_direct_sums_pass(hw, nbg):
    p, g = sharp_case(hw, nbg, 50)
    ref, bound = R.mask_metrics(torch.from_numpy(p).to(F64)[None], torch.from_numpy(g).to(F64)[None])
    pu.check("cpu:mask_metrics_direct", emulate_mask_metrics(p, g, algebra=False), ref, bound, report=False)
    old = emulate_mask_metrics(p, g, algebra=True)
    rec, fails = pu.compare(old, ref, bound)
    assert fails and rec["max_ratio"] > 1.0, rec
    err = (old.to(F64) - ref).abs()[0]
    assert float(err[3]) > float(bound[0, 3]) and float(err[4]) > float(bound[0, 4])       # mdice and miou are the ones that break
    pu.check("cpu:mask_metrics_fg", old[:, :3], ref[:, :3], bound[:, :3], report=False)    # dice, mae, iou never used the algebra


@pytest.mark.parametrize("hw", [1, 255, 4096])
def test_mask_metrics_emulation_benign_cases(hw):
    r = np.random.default_rng(51)
    p = r.uniform(0, 1, hw).astype(np.float32)
    for g in ((r.uniform(0, 1, hw) > 0.6).astype(np.float32), np.ones(hw, np.float32), np.zeros(hw, np.float32), (p > 0.5).astype(np.float32)):
        for pp in (p, g):
            ref, bound = R.mask_metrics(torch.from_numpy(pp).to(F64)[None], torch.from_numpy(g).to(F64)[None])
            pu.check("cpu:mask_metrics", emulate_mask_metrics(pp, g, algebra=False), ref, bound, report=False)

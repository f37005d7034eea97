"""fp64 references of the small kernels (cor_amd/csrc/rows.hip, misc.hip, postproc.hip) with their a-priori error bounds.

Every function takes torch CPU tensors and returns (ref, bound) in the dtype of its inputs: called with float64 it is the reference
and the bound the GPU tests hold a kernel to; called with float32 its first result is a plain fp32 evaluation of the same operation
(tests/test_cpu_small_kernel_refs.py passes that through the comparator to show that correct fp32 arithmetic stays inside the bound).
A bf16 kernel input is widened by the caller first: the reference sees the values the kernel sees.

The bound rule (first order, u = 2^-24, written out beside each reference):
  * an fp32 chain or tree over n terms: (n + c) u sum|term|, c the remaining roundings on the path (scaling, division, sqrt);
  * a libm call (expf, log1pf, sinf, cosf, tanhf, sqrtf): 4 ulp of its result (<= 8u relative; the HIP maxima documented for these
    are 1-2 ulp), its argument's error carried through the derivative;
  * erf_as: the 1.5e-7 of Abramowitz-Stegun 7.1.26 (common.h) plus 8u for the roundings of its fp32 evaluation (five Horner
    steps on |p| <= 1.5, a reciprocal, an exp2, the final fma on values <= 1);
  * every bound returned is TWICE the first-order worst case.
Nothing here is fitted to what a kernel returns.
"""
from __future__ import annotations

import math

import torch

U = 2.0 ** -24
TINY = 2.0 ** -126
LIBM = 8.0 * U                     # 4 ulp of a result r is at most 8u|r|
ERF_AS = 1.5e-7 + 8.0 * U
MARGIN = 2.0


# ---------------------------------------------------------------- activations (COR_ACT_*: 0 none, 1 erf GELU, 2 ReLU, 3 sigmoid, 4 tanh GELU)
def act_ref(y, act):
    if act == 0:
        return y
    if act == 1:
        return 0.5 * y * (1.0 + torch.erf(y / math.sqrt(2.0)))
    if act == 2:
        return y.clamp(min=0)
    if act == 3:
        return 1.0 / (1.0 + torch.exp(-y))
    if act == 4:
        return 0.5 * y * (1.0 + torch.tanh(0.79788456080286535588 * (y + 0.044715 * y * y * y)))
    raise ValueError(act)


def act_err(y, dy, act):
    """First-order error of apply_act on an fp32 value y that already carries the error dy."""
    if act in (0, 2):
        return dy                                                # identity / ReLU: 1-Lipschitz, no rounding
    g = act_ref(y, act)
    if act == 1:    # |gelu'| <= 1.13; erf argument: two roundings, |t erf'(t)| <= 0.5 -> u; 1 + erf: <= 2u; two products
        return 1.13 * dy + 0.5 * y.abs() * (ERF_AS + 3.0 * U) + 2.0 * U * g.abs()
    if act == 3:    # s = 1/(1+e), e = expf(-y): ds = s^2 de = 8u s(1-s); the add and the division: 2u s; s' <= 1/4
        return 0.25 * dy + LIBM * g * (1.0 - g) + 2.0 * U * g
    c = 0.79788456080286535588
    z = c * (y + 0.044715 * y * y * y)
    t = torch.tanh(z)
    dz = 5.0 * U * c * (y.abs() + 0.044715 * y.abs() ** 3)      # five roundings on the way to z
    dt = LIBM * t.abs() + (1.0 - t * t) * dz
    return 1.13 * dy + 0.5 * y.abs() * (dt + 2.0 * U) + 2.0 * U * g.abs()


# ---------------------------------------------------------------- LayerNorm over the last axis
def ln_core(v, dv, w, b, eps):
    """(y, dy) of y = (v - mean) rstd w + b for fp32 values v carrying the errors dv (first order, no margin)."""
    C = v.shape[-1]
    mean = v.sum(-1, keepdim=True) / C
    em = dv.sum(-1, keepdim=True) / C + (C + 1) * U * v.abs().sum(-1, keepdim=True) / C       # C-term sum, one division
    d = v - mean
    dd = dv + em + U * d.abs()
    var = (d * d).sum(-1, keepdim=True) / C
    evar = (2.0 * d.abs() * dd).sum(-1, keepdim=True) / C + (C + 2) * U * var                 # squares, C-term sum, division
    r = 1.0 / torch.sqrt(var + eps)
    relr = 0.5 * evar / (var + eps) + LIBM + 3.0 * U                                          # eps as fp32, the add, sqrtf, the division
    y = d * r * w + b
    dy = (w * r).abs() * dd + (d * r * w).abs() * (relr + 3.0 * U) + U * y.abs()
    return y, dy


def layernorm(x, w, b, eps, act=0):
    y, dy = ln_core(x, torch.zeros_like(x), w, b, eps)
    return act_ref(y, act), MARGIN * act_err(y, dy, act)


def l2norm_rows(x, eps=1e-12):
    C = x.shape[-1]
    n = torch.sqrt((x * x).sum(-1, keepdim=True))
    ref = x / n.clamp(min=eps)
    rel = torch.where(n > eps, torch.full_like(n, 0.5 * (C + 1) * U + LIBM), torch.full_like(n, U)) + 2.0 * U   # 1/max, the product
    return ref, MARGIN * rel * ref.abs()


def add(a, b):
    ref = (a.reshape(-1, b.numel()) + b.reshape(1, -1)).reshape(a.shape)
    return ref, MARGIN * U * ref.abs()                           # one rounding


# ---------------------------------------------------------------- pure moves (expected values, compared bitwise)
def tokens_to_nchw(x, B, HW, C):
    return x.reshape(B, HW, C).permute(0, 2, 1).contiguous()


def nchw_to_tokens(x, B, HW, C):
    return x.reshape(B, C, HW).permute(0, 2, 1).reshape(B * HW, C).contiguous()


def patchify(img, p, Kpad):
    B, C, H, W = img.shape
    gh, gw = H // p, W // p
    out = torch.zeros((B, gh, gw, Kpad), dtype=img.dtype)
    for c in range(C):
        for dy in range(p):
            for dx in range(p):
                out[:, :, :, (c * p + dy) * p + dx] = img[:, c, dy:gh * p:p, dx:gw * p:p]
    return out.reshape(B * gh * gw, Kpad)


def im2col3x3(x, B, H, W):
    C = x.shape[-1]
    xp = torch.zeros((B, H + 2, W + 2, C), dtype=x.dtype)
    xp[:, 1:H + 1, 1:W + 1] = x.reshape(B, H, W, C)
    cols = [xp[:, ky:ky + H, kx:kx + W] for ky in range(3) for kx in range(3)]
    return torch.stack(cols, dim=3).reshape(B * H * W, 9 * C)


def pixel_shuffle(y, B, H, W, C):
    """y [B*H*W, 4C], column (dy*2+dx)*C + c -> [B*2H*2W, C]"""
    return y.reshape(B, H, W, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B * 4 * H * W, C)


# ---------------------------------------------------------------- bilinear (align_corners=False, no antialias)
def _taps(n_in, n_out, dtype):
    s = ((torch.arange(n_out, dtype=dtype) + 0.5) * (n_in / n_out) - 0.5).clamp(min=0)
    i0 = s.floor().long().clamp(max=n_in - 1)
    i1 = (i0 + 1).clamp(max=n_in - 1)
    # the kernel forms s in fp32 (a division, a product, a subtraction): |ds| <= 4u (s + 1). Where that moves floor(s) across an
    # integer the taps change but the value does not jump: the interpolant is continuous with slope <= the largest neighbour difference.
    return i0, i1, s - i0.to(dtype), 4.0 * U * (s + 1.0)


def bilinear(x, OH, OW, clamp01=False):
    B, C, H, W = x.shape
    y0, y1, wy, dsy = _taps(H, OH, x.dtype)
    x0, x1, wx, dsx = _taps(W, OW, x.dtype)
    r0, r1 = x[:, :, y0], x[:, :, y1]
    a, b, c, d = r0[:, :, :, x0], r0[:, :, :, x1], r1[:, :, :, x0], r1[:, :, :, x1]
    wyc = wy[:, None]
    ref = (a * (1 - wx) + b * wx) * (1 - wyc) + (c * (1 - wx) + d * wx) * wyc
    mag = (a.abs() * (1 - wx) + b.abs() * wx) * (1 - wyc) + (c.abs() * (1 - wx) + d.abs() * wx) * wyc
    zero = torch.zeros((B, C, 1, 1), dtype=x.dtype)
    Dx = (x[:, :, :, 1:] - x[:, :, :, :-1]).abs().amax((2, 3), keepdim=True) if W > 1 else zero
    Dy = (x[:, :, 1:] - x[:, :, :-1]).abs().amax((2, 3), keepdim=True) if H > 1 else zero
    err = dsx[None, None, None, :] * Dx + dsy[None, None, :, None] * Dy + 8.0 * U * mag       # 1-w, two products and an add, twice
    if clamp01:
        ref = ref.clamp(0, 1)                                    # 1-Lipschitz, exact
    return ref, MARGIN * err


# ---------------------------------------------------------------- convolutions
def conv3x3s2(x_nchw, w, bias):
    """3x3 stride 2 pad 1; x [B,Cin,H,W], w [Cout,Cin,3,3] -> [B,OH,OW,Cout]. One fma per tap on the bias: <= 9 Cin + 1 roundings."""
    B, Cin, H, W = x_nchw.shape
    Cout = w.shape[0]
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = torch.zeros((B, Cin, 2 * OH + 1, 2 * OW + 1), dtype=x_nchw.dtype)
    xp[:, :, 1:H + 1, 1:W + 1] = x_nchw
    acc = torch.zeros((B, OH, OW, Cout), dtype=x_nchw.dtype)
    mag = torch.zeros_like(acc)
    if bias is not None:
        acc = acc + bias
        mag = mag + bias.abs()
    for ky in range(3):
        for kx in range(3):
            xs = xp[:, :, ky:ky + 2 * OH:2, kx:kx + 2 * OW:2]
            acc = acc + torch.einsum("bchw,oc->bhwo", xs, w[:, :, ky, kx])
            mag = mag + torch.einsum("bchw,oc->bhwo", xs.abs(), w[:, :, ky, kx].abs())
    return acc, MARGIN * (9 * Cin + 1) * U * mag


def dwconv7x7(x, w_t, bias, B, H, W):
    """depthwise 7x7 pad 3, channels-last x [B,H,W,C], w_t [49,C] -> [B*H*W, C]. 49 fmas on the bias: <= 50 roundings."""
    C = x.shape[-1]
    xp = torch.zeros((B, H + 6, W + 6, C), dtype=x.dtype)
    xp[:, 3:H + 3, 3:W + 3] = x.reshape(B, H, W, C)
    xa, wa = xp.abs(), w_t.abs()
    acc = bias.expand(B, H, W, C).clone()
    mag = bias.abs().expand(B, H, W, C).clone()
    for ky in range(7):
        for kx in range(7):
            acc.addcmul_(xp[:, ky:ky + H, kx:kx + W], w_t[ky * 7 + kx])
            mag.addcmul_(xa[:, ky:ky + H, kx:kx + W], wa[ky * 7 + kx])
    return acc.reshape(B * H * W, C), (MARGIN * 50 * U * mag).reshape(B * H * W, C)


# ---------------------------------------------------------------- pooling
def adapter_pool(maps, feat):
    """oracle/support.mask_adapter_pooling's tail: a = softmax over positions of logsigmoid(maps); out = mean over maps of a @ feat.
    maps [B,P,M], feat [B,P,D] -> [B,D]."""
    B, P, M = maps.shape
    e = torch.exp(-maps.abs())
    l1 = torch.log1p(e)
    ls = maps.clamp(max=0) - l1
    els = LIBM * e + LIBM * l1 + U * ls.abs()                    # expf (log1p' <= 1), log1pf, the subtraction
    mx, arg = ls.max(dim=1, keepdim=True)
    z = ls - mx
    dz = els + torch.gather(els, 1, arg) + U * z.abs()
    ex = torch.exp(z)
    rel_e = LIBM + dz
    s = ex.sum(1, keepdim=True)
    t = ex / s
    rel_t = rel_e + rel_e.amax(1, keepdim=True) + (P + 3) * U    # the P-term sum, 1/s, the product
    wgt = t.mean(2)
    dw = (t * rel_t).sum(2) / M + (M + 1) * U * wgt              # M-term sum, the division by M
    ref = torch.einsum("bp,bpd->bd", wgt, feat)
    err = torch.einsum("bp,bpd->bd", dw, feat.abs()) + P * U * torch.einsum("bp,bpd->bd", wgt, feat.abs())
    return ref, MARGIN * err


def masked_pool(feat, mask, clamp01=False, l2norm=False):
    """feat [B,P,D] channels-last (the NCHW form is permuted by the caller), mask [B,P] -> [B,D]"""
    B, P, D = feat.shape
    mk = mask.clamp(0, 1) if clamp01 else mask
    denom = mk.sum(1, keepdim=True) + 1e-8
    rd = (P + 1) * U * mk.abs().sum(1, keepdim=True) / denom.abs() + U                        # P-term sum, + 1e-8 (itself rounded)
    acc = torch.einsum("bp,bpd->bd", mk, feat)
    mag = torch.einsum("bp,bpd->bd", mk.abs(), feat.abs())
    res = acc / denom
    dres = P * U * mag / denom.abs() + res.abs() * (rd + U)
    if not l2norm:
        return res, MARGIN * dres
    n = res.norm(dim=1, keepdim=True)
    dn = dres.norm(dim=1, keepdim=True) + n * (0.5 * (D + 1) * U + LIBM)
    den = n.clamp(min=1e-12)
    out = res / den
    return out, MARGIN * (dres / den + out.abs() * (dn / den + 2.0 * U))


# ---------------------------------------------------------------- gated fusion
def fuse_gate(img, txt, aI, aT):
    ref = torch.cat([aI * img, aT * txt], dim=1)
    return ref, MARGIN * U * ref.abs()


def fuse_mix(cat, dyn):
    D = cat.shape[1] // 2
    a = dyn.reshape(-1, 1)
    p0, p1 = a * cat[:, :D], (1.0 - a) * cat[:, D:]
    v = p0 + p1
    dv = 4.0 * U * (p0.abs() + p1.abs())                         # 1 - a, two products, an add
    n = v.norm(dim=1, keepdim=True)
    dn = dv.norm(dim=1, keepdim=True) + n * (0.5 * (D + 1) * U + LIBM)
    den = n.clamp(min=1e-12)
    out = v / den
    return out, MARGIN * (dv / den + out.abs() * (dn / den + 2.0 * U))


# ---------------------------------------------------------------- dense random-Fourier positional encoding
def dense_pe(G, size):
    F = G.shape[1]
    c = 2.0 * ((torch.arange(size, dtype=G.dtype) + 0.5) / size) - 1.0                        # |c| <= 1, a division and a subtraction
    dc = 3.0 * U
    cx, cy = c.reshape(1, size, 1), c.reshape(size, 1, 1)
    tx, ty = cx * G[0], cy * G[1]
    arg = tx + ty
    darg = dc * (G[0].abs() + G[1].abs()) + 3.0 * U * (tx.abs() + ty.abs())
    ang = 2.0 * math.pi * arg
    dang = 2.0 * math.pi * darg + 2.0 * U * ang.abs()                                         # 2 pi as fp32, the product
    s, co = torch.sin(ang), torch.cos(ang)
    ref = torch.cat([s, co], dim=2).reshape(size * size, 2 * F)
    err = torch.cat([dang + LIBM * s.abs(), dang + LIBM * co.abs()], dim=2).reshape(size * size, 2 * F)
    return ref, MARGIN * err


# ---------------------------------------------------------------- mask decoder upscaling
def upscale_shuffle(y, B, H, W, C, bias=None, ln_w=None, ln_b=None, eps=1e-6, act=0):
    v = pixel_shuffle(y, B, H, W, C)
    dv = torch.zeros_like(v)
    if bias is not None:
        v = v + bias
        dv = U * v.abs()
    if ln_w is not None:
        v, dv = ln_core(v, dv, ln_w, ln_b, eps)
    return act_ref(v, act), MARGIN * act_err(v, dv, act)


def upscale_hyper(x, w, bias, hyper, B, H, W):
    """ConvTranspose2d(64 -> 32, 2x2, stride 2) -> erf GELU -> dot with hyper [B,K,32]; x [B*H*W, 64] -> [B,K,2H,2W]"""
    K = hyper.shape[1]
    xv = x.reshape(B, H, W, 64)
    a = torch.einsum("bhwi,iopq->bhwpqo", xv, w) + bias
    da = 65.0 * U * (torch.einsum("bhwi,iopq->bhwpqo", xv.abs(), w.abs()) + bias.abs())      # 64 fmas on the bias
    g = act_ref(a, 1)
    dg = act_err(a, da, 1)
    ref = torch.einsum("bko,bhwpqo->bkhpwq", hyper, g).reshape(B, K, 2 * H, 2 * W)
    err = torch.einsum("bko,bhwpqo->bkhpwq", hyper.abs(), dg) + 32.0 * U * torch.einsum("bko,bhwpqo->bkhpwq", hyper.abs(), g.abs())
    return ref, MARGIN * err.reshape(B, K, 2 * H, 2 * W)


# ---------------------------------------------------------------- post-processing
def mask_prob_minmax(x):
    """x [B,HW] logits -> (sigmoid - min) / (max - min + 1e-8) per sample"""
    p = 1.0 / (1.0 + torch.exp(-x))
    dp = LIBM * p * (1.0 - p) + 2.0 * U * p + TINY               # expf, the add and the division; TINY: 1/(1+inf) = 0 for x = -100
    mx, mn = p.amax(1, keepdim=True), p.amin(1, keepdim=True)
    dpm = dp.amax(1, keepdim=True)
    d = mx - mn + 1e-8
    dd = 2.0 * dpm + 2.0 * U * d
    o = (p - mn) / d
    err = (dp + dpm + U * (p - mn).abs()) / d + o.abs() * (dd / d + 2.0 * U)
    return o, MARGIN * err


def mask_metrics(pred, gt, smooth=1e-5):
    """[B,HW] x2 -> [B,5] = dice, mae, iou, mdice, miou, every background sum taken element by element (utils/trainer_v3_g.py:381-443).
    Every sum has non-negative terms, so each carries a relative error gamma = (HW/256 + 8) u (the per-thread chain, the wave tree, the
    four waves); the only subtraction left is ps + gs - pg >= (ps + gs) / 2. All five outputs: relative error <= 8 gamma."""
    HW = pred.shape[1]

    def dice(a, b):
        return (2.0 * (a * b).sum(1) + smooth) / (a.sum(1) + b.sum(1) + smooth)

    def iou(a, b):
        inter = (a * b).sum(1)
        return (inter + smooth) / (a.sum(1) + b.sum(1) - inter + smooth)

    na, nb = 1.0 - pred, 1.0 - gt
    ref = torch.stack([dice(pred, gt), (pred - gt).abs().sum(1) / HW, iou(pred, gt), 0.5 * (dice(pred, gt) + dice(na, nb)),
                       0.5 * (iou(pred, gt) + iou(na, nb))], dim=1)
    gamma = (HW / 256.0 + 8.0) * U
    return ref, 8.0 * gamma * ref.abs()


THR_DELTA, GRAY_DELTA = 1e-5, 1e-3


def binarize_decide(thr):
    return lambda v: 255.0 * (v > thr)


def binarize_margin(thr):
    return lambda v: abs(v - thr) / THR_DELTA


def gray_decide(v):
    import numpy as np
    return np.floor(np.clip(255.0 * v, 0.0, 255.0))


def gray_margin(v):
    import numpy as np
    t = 255.0 * v
    return np.abs(t - np.rint(t)) / GRAY_DELTA

"""Exact-query mode on the MI355X: x3 split producers, the x3 GEMM, flash_fwd_f32, and the model with query_dtype = torch.float32
beside a bf16 SAM (golden anchor, full-depth SigLIP-B with a 100k-row search, captured graphs, unchanged defaults)."""
import numpy as np
import pytest
import torch

from oracle import config as ocfg
from tests.golden_util import load, make_inputs

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, BF16 = torch.float32, torch.bfloat16


def _ops():
    from cor_amd import ops
    return ops


def _split_ref(x):
    hi = x.to(BF16)
    lo = (x - hi.float()).to(BF16)
    return torch.cat([lo, hi, hi], dim=1)


def _x3_weight(w):
    return _ops().split_weight_x3(w)


# ---------------------------------------------------------------------------------------------------------------- split producers
@pytest.mark.parametrize("rows,C,ld_in", [(1, 4, 4), (7, 3, 5), (33, 768, 768), (129, 1536, 1600), (5, 250, 251), (2048, 3072, 3072)])
def test_split_kernel_bitwise(rows, C, ld_in):
    ops = _ops()
    g = torch.Generator(device=DEV).manual_seed(rows * 7 + C)
    big = torch.randn((rows, ld_in), generator=g, device=DEV) * torch.logspace(-4, 4, ld_in, device=DEV)
    x = big[:, :C]                                                   # strided view when ld_in > C
    got = ops.split_x3(x)
    assert torch.equal(got, _split_ref(x.contiguous()))
    # a split row with a wider segment stride (cat of two blocks, as the fusion gates' input)
    out = torch.full((rows, 6 * C), 7.0, dtype=BF16, device=DEV)
    ops.split_x3(x, out[:, C:], seg=2 * C)
    ref = _split_ref(x.contiguous())
    for s in range(3):
        assert torch.equal(out[:, (2 * s + 1) * C:(2 * s + 2) * C], ref[:, s * C:(s + 1) * C])
        assert bool((out[:, 2 * s * C:(2 * s + 1) * C] == 7.0).all())           # untouched columns stay untouched


@pytest.mark.parametrize("C", [256, 768, 1152, 96])
@pytest.mark.parametrize("act", [0, 1])
def test_layernorm_split_output_equals_split_of_fp32_output(C, act):
    ops = _ops()
    g = torch.Generator(device=DEV).manual_seed(C + act)
    x = torch.randn((1000, C), generator=g, device=DEV) * 3 + 1
    w, b = torch.randn(C, generator=g, device=DEV), torch.randn(C, generator=g, device=DEV)
    y32 = ops.layernorm(x, w, b, 1e-6, out_dtype=F32, act=act)
    y3 = ops.layernorm(x, w, b, 1e-6, out_dtype=ops.X3, act=act)
    assert torch.equal(y3, _split_ref(y32))
    assert torch.equal(ops.layernorm(x, w, b, 1e-6, out_dtype=ops.X3, act=act, reverse=True), y3)


def test_gemm_split_output_equals_split_of_fp32_output():
    ops = _ops()
    g = torch.Generator(device=DEV).manual_seed(11)
    a, w = torch.randn((300, 768), generator=g, device=DEV), torch.randn((3072, 768), generator=g, device=DEV) * 0.03
    bias = torch.randn(3072, generator=g, device=DEV)
    A3, W3 = ops.split_x3(a), _x3_weight(w)
    y32 = ops.gemm(A3, W3, out_dtype=F32, bias=bias, act=ops.ACT_GELU_ERF, x3=True)
    y3 = ops.gemm(A3, W3, out_dtype=ops.X3, bias=bias, act=ops.ACT_GELU_ERF, x3=True)
    assert torch.equal(y3, _split_ref(y32))


def test_patchify_split_output():
    ops = _ops()
    img = torch.randn((2, 3, 384, 384), device=DEV)
    assert torch.equal(ops.patchify(img, 16, 768, ops.X3), _split_ref(ops.patchify(img, 16, 768, F32)))


# ---------------------------------------------------------------------------------------------------------------- x3 GEMM
def _ref_gemm(a, w, bias=None, act=0, residual=None, col_scale=None):
    """fp64 result and the error scale sum|a.b| (+ |bias|, |residual| as the kernels add them in fp32)."""
    y = a.double() @ w.double().T
    scale = a.double().abs() @ w.double().abs().T
    if bias is not None:
        y = y + bias.double()
        scale = scale + bias.double().abs()
    if act == 1:
        y = 0.5 * y * (1 + torch.erf(y / 2 ** 0.5))
    elif act == 4:
        y = 0.5 * y * (1 + torch.tanh(0.7978845608028654 * (y + 0.044715 * y ** 3)))
    elif act == 2:
        y = y.clamp_min(0)
    elif act == 3:
        y = torch.sigmoid(y)
    if col_scale is not None:
        y = y * col_scale.double()
        scale = scale * col_scale.double().abs()
    if residual is not None:
        y = y + residual.double()
        scale = scale + residual.double().abs()
    return y, scale


# (M, N, K): the support branch's GEMMs at batch 32 (towers: 18 432 / 2 048 rows; adapter / fusion / dim_proj: down to M = 1)
SHAPES = [(18432, 2304, 768), (18432, 768, 3072), (2048, 3072, 768), (2048, 768, 768), (64, 768, 1536), (6, 256, 768), (1, 1536, 1536),
          (1, 256, 768), (576, 8, 256), (18432, 768, 768)]


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_x3_gemm_accuracy_every_shape(M, N, K):
    ops = _ops()
    g = torch.Generator(device=DEV).manual_seed(M + N + K)
    a = torch.randn((M, K), generator=g, device=DEV)
    w = torch.randn((N, K), generator=g, device=DEV) / K ** 0.5
    bias = torch.randn(N, generator=g, device=DEV)
    y = ops.gemm(ops.split_x3(a), _x3_weight(w), out_dtype=F32, bias=bias, x3=True)
    ref, scale = _ref_gemm(a, w, bias)
    err = ((y.double() - ref).abs() / scale).max().item()
    assert err <= 2e-6, err


@pytest.mark.parametrize("act", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("extra", ["none", "residual", "col_scale"])
@pytest.mark.parametrize("cfg", [0, 1, 2, 3, 4, 9, 13])
def test_x3_gemm_epilogues_and_configs(act, extra, cfg):
    ops = _ops()
    M, N, K = (2048, 768, 768) if cfg in (0, 13) else (300, 256, 768)
    g = torch.Generator(device=DEV).manual_seed(act * 10 + cfg)
    a = torch.randn((M, K), generator=g, device=DEV)
    w = torch.randn((N, K), generator=g, device=DEV) / K ** 0.5
    bias = torch.randn(N, generator=g, device=DEV) * 0.1
    res = torch.randn((M, N), generator=g, device=DEV) if extra == "residual" else None
    cs = torch.rand(N, generator=g, device=DEV) + 0.5 if extra == "col_scale" else None
    A3, W3 = ops.split_x3(a), _x3_weight(w)
    kw = dict(out_dtype=F32, bias=bias, act=act, residual=res, col_scale=cs, cfg=cfg, x3=True)
    y = ops.gemm(A3, W3, **kw)
    ref, scale = _ref_gemm(a, w, bias, act, res, cs)
    # epilogue functions are fp32 (erf / tanh / exp: a few fp32 ulps of their value on top of the product's error)
    err = ((y.double() - ref).abs() - 1e-6 * ref.abs()).clamp_min(0) / scale
    assert err.max().item() <= 2.5e-6, err.max().item()
    assert torch.equal(ops.gemm(A3, W3, **kw), y)                                     # run to run
    assert torch.equal(ops.gemm(A3, W3, **kw, reverse=True), y)                      # COR_ORDER_REVERSE


def test_x3_gemm_configs_agree_and_batch_invariance():
    ops = _ops()
    g = torch.Generator(device=DEV).manual_seed(99)
    K, N = 768, 768
    a = torch.randn((18432, K), generator=g, device=DEV)
    w = torch.randn((N, K), generator=g, device=DEV) / K ** 0.5
    bias = torch.randn(N, generator=g, device=DEV)
    A3, W3 = ops.split_x3(a), _x3_weight(w)
    full = ops.gemm(A3, W3, out_dtype=F32, bias=bias, x3=True)                        # persistent kernel (cfg 13 by dispatch)
    for r0 in (0, 576 * 17, 18432 - 576):
        part = ops.gemm(A3[r0:r0 + 576], W3, out_dtype=F32, bias=bias, x3=True)      # 128x128 / LDS-DMA kernels
        assert torch.equal(part, full[r0:r0 + 576]), r0
    one = ops.gemm(A3[5:6], W3, out_dtype=F32, bias=bias, x3=True)
    assert torch.equal(one, full[5:6])


# ---------------------------------------------------------------------------------------------------------------- flash_fwd_f32
def _attn_ref(q, k, v, N, H, T, hd):
    qd, kd, vd = (t.double().view(N, T, H, hd).transpose(1, 2) for t in (q, k, v))
    s = (qd @ kd.transpose(-1, -2)) * hd ** -0.5
    return (torch.softmax(s, -1) @ vd).transpose(1, 2).reshape(N * T, H * hd)


@pytest.mark.parametrize("hd,H", [(64, 12), (72, 16), (80, 4)])
@pytest.mark.parametrize("T,N", [(64, 32), (576, 8), (729, 4), (1024, 2), (77, 3)])
@pytest.mark.parametrize("amp", [0.05, 1.0, 6.0])
def test_flash_fwd_f32_vs_fp64_and_rowlane(hd, H, T, N, amp):
    ops = _ops()
    D = H * hd
    g = torch.Generator(device=DEV).manual_seed(hd * T + N)
    qkv = torch.randn((N * T, 3 * D), generator=g, device=DEV) * amp
    q, k, v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
    ref = _attn_ref(q, k, v, N, H, T, hd)
    got = ops.attention_f32(q, k, v, N, H, T, T, hd, hd ** -0.5)
    rl = ops.attention(q, k, v, N, H, T, T, hd, hd ** -0.5, out_dtype=F32)           # fp32 mode's row-per-lane kernel
    scale = ref.abs().max().item()
    e_new = (got.double() - ref).abs().max().item() / scale
    e_rl = (rl.double() - ref).abs().max().item() / scale
    assert e_new <= 2 * e_rl, (e_new, e_rl)
    x3 = ops.attention_f32(q, k, v, N, H, T, T, hd, hd ** -0.5, out_dtype=ops.X3)
    assert torch.equal(x3, _split_ref(got))
    assert torch.equal(ops.attention_f32(q, k, v, N, H, T, T, hd, hd ** -0.5), got)


# ---------------------------------------------------------------------------------------------------------------- the model
def _golden_model(pooling):
    from cor_amd import config
    from tests.test_gpu_parity import _build
    g = load(f"toplevel_{pooling}")
    gcfg = dict(config.siglip_cfg("ViT-B-16-SigLIP-384"), depth=2, t_depth=2, vocab=512)
    model = _build(12, (2, 5, 8, 11), gcfg, pooling)
    spec = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    sd = ocfg.random_state({k: v for k, v in spec.items() if "attn_pool" not in k}, int(g["seed_params"]))
    model.load_state_dict(sd, strict=False)
    model = model.to(DEV).eval()
    inp = make_inputs(int(g["seed_inputs"]), q=(1, 3, 1024, 1024), s=(1, 3, 384, 384), text=("tokens", 1, 64, 512), mask=("mask", 1, 384))
    kw = dict(query_image_inputs=inp["q"].to(DEV), support_image_inputs=inp["s"].to(DEV), change_text_inputs=inp["text"].to(DEV),
              support_mask_inputs=inp["mask"].to(DEV))
    return model, kw, g


@pytest.mark.parametrize("pooling", ["MaskAdapterPooling", "MaskedPooling"])
def test_golden_anchor_exact_query_beside_bf16_sam(pooling):
    model, kw, g = _golden_model(pooling)
    model.compute_dtype = BF16
    _, emb_bf16, feat_bf16 = model(**kw, multimask_output=True)
    model.query_dtype = F32
    masks, emb, feat = model(**kw, multimask_output=True)
    ref = torch.from_numpy(g["feat"]).reshape(feat.shape)
    err = (feat.cpu() - ref).abs().max().item()
    err_bf16 = (feat_bf16.cpu() - ref).abs().max().item()
    print(f"feat vs golden: exact-query {err:.3e}, bf16 mode {err_bf16:.3e}")
    assert err <= 1e-5, err
    assert torch.equal(emb, emb_bf16)                                                 # the SAM side is untouched
    assert (BF16, _ops().X3) in model._packed and BF16 in model._packed
    # the same under autocast(bf16) with compute_dtype float32
    model.compute_dtype = F32
    with torch.autocast("cuda", dtype=BF16):
        _, emb_ac, feat_ac = model(**kw, multimask_output=True)
    assert torch.equal(feat_ac, feat) and torch.equal(emb_ac, emb_bf16)


def test_defaults_unchanged_and_fp32_exact_query_is_the_fp32_path():
    model, kw, _ = _golden_model("MaskAdapterPooling")
    for T in (F32, BF16):
        model.compute_dtype = T
        base = model(**kw, multimask_output=True)
        model.query_dtype = None
        again = model(**kw, multimask_output=True)
        for a, b in zip(base, again):
            assert torch.equal(a, b)
    model.compute_dtype = F32
    base = model(**kw, multimask_output=True)
    model.query_dtype = F32
    exact = model(**kw, multimask_output=True)
    for a, b in zip(base, exact):
        assert torch.equal(a, b)
    assert set(k for k in model._packed if k != "fp") == {F32, BF16}                 # no extra pack for fp32 + fp32


def _small_model(B, seed=5):
    from cor_amd import config, utils
    from tests.test_gpu_parity import _build
    gcfg = dict(config.siglip_cfg("ViT-B-16-SigLIP-384"), depth=2, t_depth=2, vocab=512)
    model = _build(2, (1,), gcfg, "MaskAdapterPooling")
    model.load_state_dict(ocfg.random_state({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed), strict=True)
    model = model.to(DEV).eval()
    batch = utils.synthetic_batch(B, torch.device(DEV), seed=seed, vocab=512)
    return model, batch


def test_capture_and_pipeline_replays_equal_eager_exact_query():
    model, b = _small_model(2)
    model.compute_dtype, model.query_dtype = BF16, F32
    eager = model(**b, multimask_output=True)
    torch.cuda.synchronize()
    g = model.capture(**b, multimask_output=True)
    for a, e in zip(g(**b, clone=True), eager):
        assert torch.equal(a, e)
    for stagger in (False, True):
        pipe = model.capture_pipeline(**b, multimask_output=True, depth=2, stagger=stagger)
        outs = [pipe.submit(tuple(b.values()), then=lambda o: tuple(t.clone() for t in o))[1] for _ in range(3)]
        torch.cuda.synchronize()
        for out in outs:
            for a, e in zip(out, eager):
                assert torch.equal(a, e), stagger
    # engine.forward_support on two streams (text tower on its own chain) computes the same feature
    from cor_amd import engine
    W = model.packed(BF16)
    args = (W, model.support_branch.siglip.cfg, model.support_branch.mask_pooling_name, _ops().X3,
            b["support_image_inputs"], b["change_text_inputs"], b["support_mask_inputs"])
    f2 = engine.forward_support(*args, two_chains=True)
    f1 = engine.forward_support(*args, two_chains=False)
    torch.cuda.synchronize()
    assert torch.equal(f1, f2) and torch.equal(f1.view(eager[2].shape), eager[2])


# ---------------------------------------------------------------------------------------------------------------- full depth
def test_full_depth_siglip_b_feat_and_top10():
    """Real SigLIP-B/16-384 (12 + 12 layers) at batch 32: the exact-query feature against the fp32 mode's, then a 100k-row search."""
    from cor_amd import config, engine, utils
    from tests.test_gpu_parity import _build
    ops = _ops()
    gcfg = dict(config.siglip_cfg("ViT-B-16-SigLIP-384"))
    model = _build(1, (0,), gcfg, "MaskAdapterPooling")
    model.load_state_dict(ocfg.random_state({k: tuple(v.shape) for k, v in model.state_dict().items()}, 17), strict=True)
    utils.zero_support_head_biases(model)                  # distinct features per sample (see the helper), as bench.py does
    model = model.to(DEV).eval()
    b = utils.synthetic_batch(32, torch.device(DEV), seed=3, vocab=gcfg["vocab"], structured=True)
    sb = (b["support_image_inputs"], b["change_text_inputs"], b["support_mask_inputs"])
    scfg, pool = model.support_branch.siglip.cfg, model.support_branch.mask_pooling_name
    with torch.no_grad():
        f32 = engine.forward_support(model.packed(F32), scfg, pool, F32, *sb, two_chains=False)
        model.compute_dtype, model.query_dtype = BF16, F32
        fx3 = engine.forward_support(model.packed(BF16), scfg, pool, ops.X3, *sb, two_chains=False)
        model.query_dtype = None
        fbf = engine.forward_support(model.packed(BF16), scfg, pool, BF16, *sb, two_chains=False)
    torch.cuda.synchronize()
    d = (fx3 - f32).abs().max().item()
    print(f"full depth feat: exact-query vs fp32 {d:.3e}, bf16 mode vs fp32 {(fbf - f32).abs().max().item():.3e}")
    assert d <= 1e-5, d

    # 100k-row bf16 gallery: indices agree wherever the fp32 mode's margins exceed 4x the largest score difference
    gen = torch.Generator(device=DEV).manual_seed(8)
    G = torch.nn.functional.normalize(torch.randn((100_000, 256), generator=gen, device=DEV), dim=1).to(BF16).contiguous()
    s32, i32 = ops.similarity_topk(f32, G, 10)
    sx3, ix3 = ops.similarity_topk(fx3, G, 10)
    # score difference on the SAME rows: every gallery row's score moves by at most this much between the two queries
    full32, fullx3 = f32.double() @ G.double().T, fx3.double() @ G.double().T
    delta = (full32 - fullx3).abs().max().item()
    s11, _ = torch.topk(full32, 11, dim=1)
    gaps_hi = torch.cat([torch.full((32, 1), float("inf"), device=DEV, dtype=torch.float64), s11[:, :10] - s11[:, 1:11]], 1)[:, :10]
    gaps_lo = s11[:, :10] - s11[:, 1:11]
    safe = (torch.minimum(gaps_hi, gaps_lo) > 4 * delta).cpu()
    agree = (i32 == ix3).cpu()
    n_unsafe = int((~safe).sum())
    print(f"top-10: max score difference {delta:.3e}; {int(safe.sum())} entries past the margin rule, {n_unsafe} within it "
          f"({int((~agree & ~safe).sum())} of those differ)")
    assert bool(agree[safe].all())

    # planted rows at cosine margins >= 1e-4: identical indices at every rank
    rows = []
    gp = torch.Generator(device=DEV).manual_seed(9)
    base = torch.nn.functional.normalize(torch.randn((100_000, 256), generator=gp, device=DEV), dim=1) * 0.05
    for qi in range(32):
        q = f32[qi].double()
        for r in range(10):
            cos = 0.99 - 2e-4 * r
            noise = torch.randn(256, generator=gp, device=DEV, dtype=torch.float64)
            noise = noise - (noise @ q) * q
            rows.append(cos * q + (1 - cos ** 2) ** 0.5 * noise / noise.norm())
    plant = torch.stack(rows).float()
    Gp = base.clone()
    Gp[torch.arange(320, device=DEV) * 311 % 100_000] = plant
    Gp = Gp.contiguous()
    sp32, p32 = ops.similarity_topk(f32, Gp, 10)
    _, px3 = ops.similarity_topk(fx3, Gp, 10)
    assert float((sp32[:, :-1] - sp32[:, 1:]).min()) >= 1e-4                        # the planted margins hold in the fp32 mode
    assert torch.equal(p32, px3)

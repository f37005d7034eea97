"""Exact-query mode, host side (no GPU): the public switch `query_dtype`, the packed-cache key, the x3 weight split and the C ABI
of the new kernels (cor_split_x3, cor_attention_f32, COR_BF16X3)."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _small_model():
    from tests.test_gpu_parity import _build
    from cor_amd import config
    gcfg = dict(config.siglip_cfg("ViT-B-16-SigLIP-384"), depth=1, t_depth=1, vocab=64)
    return _build(1, (0,), gcfg, "MaskedPooling")


def test_query_dtype_defaults_to_none_and_accepts_float32():
    m = _small_model()
    assert m.query_dtype is None
    m.query_dtype = torch.float32
    assert m.query_dtype is torch.float32
    m.query_dtype = None
    assert m.query_dtype is None


@pytest.mark.parametrize("bad", [torch.bfloat16, torch.float16, torch.float64, "float32", "fp32", 32, True])
def test_query_dtype_rejects_everything_else(bad):
    m = _small_model()
    with pytest.raises(ValueError):
        m.query_dtype = bad
    assert m.query_dtype is None                                      # a refused value leaves the mode as it was


def test_branch_mode_and_pack_key():
    from cor_amd import ops
    m = _small_model()
    F32, BF16 = torch.float32, torch.bfloat16
    assert m._query_mode(F32) is F32 and m._query_mode(BF16) is BF16
    m.query_dtype = F32
    assert m._query_mode(F32) is F32                                  # fp32 compute: the exact-query branch IS the fp32 path
    assert m._query_mode(BF16) == ops.X3                              # bf16 SAM: the branch on x3 split products
    # the default keys of the packed cache are the plain dtypes (as before); exact-query beside bf16 has a key of its own
    assert m._pack_key(BF16, BF16) is BF16 and m._pack_key(F32, F32) is F32
    assert m._pack_key(BF16, ops.X3) == (BF16, ops.X3) != BF16


def test_split_weight_x3_layout_and_exactness():
    from cor_amd import ops
    g = torch.Generator().manual_seed(3)
    w = torch.randn(7, 40, generator=g) * torch.logspace(-3, 3, 40)
    s = ops.split_weight_x3(w)
    assert s.dtype == torch.bfloat16 and s.shape == (7, 120) and s.is_contiguous()
    hi, lo, hi2 = s[:, :40], s[:, 40:80], s[:, 80:]
    assert torch.equal(hi, w.to(torch.bfloat16)) and torch.equal(hi2, hi)
    assert torch.equal(lo, (w - hi.float()).to(torch.bfloat16))
    # hi + lo carries ~16 significant bits: relative error <= 2^-16 per element (bf16 alone: 2^-8)
    rel = ((hi.double() + lo.double()) - w.double()).abs() / w.double().abs()
    assert rel.max().item() <= 2.0 ** -16


def test_x3_emulation_accuracy_on_cpu():
    """The numerics the kernels implement, emulated in fp32 on the host: A_lo.W_hi + A_hi.W_lo + A_hi.W_hi with bf16 operands
    (exact products) and fp32 sums is within 2e-6 of sum|a.b| of the fp64 result; plain bf16 operands are ~100x further off."""
    g = torch.Generator().manual_seed(5)
    a, w = torch.randn(64, 768, generator=g), torch.randn(48, 768, generator=g)
    ref = a.double() @ w.double().T
    scale = a.double().abs() @ w.double().abs().T
    ah, wh = a.to(torch.bfloat16).float(), w.to(torch.bfloat16).float()
    al, wl = (a - ah).to(torch.bfloat16).float(), (w - wh).to(torch.bfloat16).float()
    x3 = torch.cat([al, ah, ah], 1) @ torch.cat([wh, wl, wh], 1).T
    err_x3 = ((x3.double() - ref).abs() / scale).max().item()
    err_bf16 = (((ah @ wh.T).double() - ref).abs() / scale).max().item()
    assert err_x3 <= 2e-6, err_x3
    assert err_bf16 > 50 * err_x3, (err_bf16, err_x3)


def test_header_declares_the_exact_query_abi():
    from cor_amd import _native
    hdr = open(os.path.join(ROOT, "include", "cor_amd.h")).read()
    declared = set(re.findall(r"^(?:int|long)\s+(cor_\w+)\s*\(", hdr, flags=re.M))
    for name in ("cor_split_x3", "cor_attention_f32"):
        assert name in declared and name in _native.SIGNATURES, name
    assert re.search(r"COR_BF16X3\s*=\s*3\b", hdr) and _native.BF16X3 == 3
    # argument counts of the two new entry points match their prototypes
    for name in ("cor_split_x3", "cor_attention_f32"):
        proto = re.search(rf"^int\s+{name}\s*\(([^;]*)\);", hdr, flags=re.M | re.S).group(1)
        assert len(proto.split(",")) == len(_native.SIGNATURES[name]), name


def test_exact_query_kernels_are_in_the_library():
    lib_path = os.path.join(ROOT, "cor_amd", "csrc", "libcor_amd.so")
    if not os.path.exists(lib_path):
        import __graft_entry__ as g
        g.build()
    from cor_amd import _native
    lib = _native.load()
    assert hasattr(lib, "cor_split_x3") and hasattr(lib, "cor_attention_f32")

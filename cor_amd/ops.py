"""Torch-tensor front end of the C ABI (include/cor_amd.h).

torch is used here only for device memory and the current HIP stream; every function enqueues one hand-written
gfx950 kernel through libcor_amd.so. Operand shapes are validated on the host BEFORE the launch (a faulting
kernel can reset the GPU). There is no CPU path: CPU tensors raise.
"""
from __future__ import annotations

import math

import torch

from . import _native as nat
from ._native import ACT_NONE, ACT_GELU_ERF, ACT_RELU, ACT_SIGMOID, ACT_GELU_TANH, F32, BF16, F16  # noqa: F401

_DT = {torch.float32: F32, torch.bfloat16: BF16, torch.float16: F16}

# Operand mode of the support branch in exact-query mode (model.query_dtype = torch.float32 beside a bf16 SAM): "x3 split rows". A
# logical fp32 [rows, C] activation is carried as a bf16 tensor [rows, 3C] = [lo | hi | hi] (hi = bf16(x), lo = bf16(x - hi)), a
# weight [N, K] as bf16 [N, 3K] = [hi | lo | hi]; their bf16 GEMM over 3K is A_lo.W_hi + A_hi.W_lo + A_hi.W_hi (include/cor_amd.h).
# Functions below that take an `out_dtype` accept X3 where noted.
X3 = "bf16x3"

# bench.py sets this to a list to time every GEMM launch with HIP events recorded on the launch stream:
# entries are (start_event, end_event, algorithmic_flops, ab_dtype, algorithmic_bytes). None = no instrumentation.
GEMM_PROFILE = None


def _lib():
    return nat.load()


def _dt(t: torch.Tensor) -> int:
    return _DT[t.dtype]


def _s():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return 0 if t is None else t.data_ptr()


def _dev(*ts):
    """Host-side guard run BEFORE every launch: the kernels take raw pointers and are enqueued on the CURRENT device's
    current stream, so (1) no CPU tensor, (2) all operands on ONE GPU, (3) that GPU is the current HIP device (otherwise
    the launch would dereference another device's memory: a GPU fault). Callers holding a model on another device wrap
    the call in `with torch.cuda.device(model.device)` (CirSegModelWithQuerySupportFeat.forward does)."""
    dev = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("cor_amd ops run on the GPU only (no CPU fallback): got a CPU tensor")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError(f"cor_amd ops: operands live on different devices ({dev} and {t.device})")
    if dev is not None and dev.index != torch.cuda.current_device():
        raise RuntimeError(f"cor_amd ops: operands live on {dev} but the current device is cuda:{torch.cuda.current_device()}; "
                           f"wrap the call in `with torch.cuda.device({dev.index})`")
    return dev


def _rows(t: torch.Tensor):
    """(rows, cols, ld) of a 2-D tensor whose last dim is contiguous."""
    assert t.dim() == 2 and t.stride(1) == 1, f"expected 2-D row-major view, got {tuple(t.shape)} / {t.stride()}"
    return t.shape[0], t.shape[1], t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])


def _f32vec(t, n, name):
    if t is None:
        return
    assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n, f"{name}: need contiguous fp32[{n}]"


def split_weight_x3(w):
    """fp32 weight [N, K] -> x3 split weight rows bf16 [N, 3K] = [hi | lo | hi] (host-side torch: runs once, at pack time)."""
    w = w.detach().to(torch.float32)
    hi = w.to(torch.bfloat16)
    lo = (w - hi.to(torch.float32)).to(torch.bfloat16)
    return torch.cat([hi, lo, hi], dim=1).contiguous()


def gemm(a, w, out_dtype=None, bias=None, act=ACT_NONE, col_scale=None, residual=None, res_row_mod=0, out=None, cfg=0, reverse=False,
         x3=False):
    """out[M,N] = residual + col_scale * act(a[M,K] @ w[N,K]^T + bias). cfg: per-call kernel choice (0 = automatic).
    reverse: walk the tiles from the last row panel to the first (same result; see ORDER_REVERSE).
    x3: a [M, 3K] / w [N, 3K] are x3 split rows (see X3); out_dtype X3 writes the result as split rows [M, 3N] (an fp32 result, then
    cor_split_x3)."""
    if out_dtype == X3:
        assert out is None and x3
        y = gemm(a, w, torch.float32, bias, act, col_scale, residual, res_row_mod, None, cfg, reverse, x3)
        return split_x3(y)
    _dev(a, w, bias, col_scale, residual, out)
    M, K, lda = _rows(a)
    N, K2, ldw = _rows(w)
    assert K == K2 and a.dtype == w.dtype, (a.shape, w.shape, a.dtype, w.dtype)
    if x3:
        assert a.dtype == torch.bfloat16 and K % 3 == 0, (a.shape, a.dtype)
        K //= 3
    if out is None:
        out = torch.empty((M, N), dtype=out_dtype or a.dtype, device=a.device)
    Mo, No, ldc = _rows(out)
    assert (Mo, No) == (M, N)
    _f32vec(bias, N, "bias")
    _f32vec(col_scale, N, "col_scale")
    ldr = 0
    if residual is not None:
        Mr, Nr, ldr = _rows(residual)
        assert residual.dtype == torch.float32 and Nr == N and Mr == (res_row_mod if res_row_mod > 0 else M)
    prof = GEMM_PROFILE
    if prof is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    nat.check(_lib().cor_gemm(a.data_ptr(), lda, w.data_ptr(), ldw, nat.BF16X3 if x3 else _dt(a), out.data_ptr(), ldc, _dt(out), M, N, K,
                              _p(bias), act, _p(col_scale), _p(residual), ldr, res_row_mod, int(cfg) | (nat.ORDER_REVERSE if reverse else 0), _s()), "cor_gemm")
    if prof is not None:
        e1.record()
        k_run = 3 * K if x3 else K
        nbytes = (M * k_run + N * k_run) * a.element_size() + M * N * out.element_size() + (M * N * 4 if residual is not None else 0)
        prof.append((e0, e1, 2.0 * M * N * k_run, a.dtype, float(nbytes)))
    return out


def layernorm(x, w, b, eps, out_dtype=None, act=ACT_NONE, out=None, reverse=False):
    """out_dtype X3 (fp32 x): the normalised rows as x3 split rows [rows, 3C]."""
    _dev(x, w, b, out)
    assert x.is_contiguous() and x.dim() == 2
    rows, C = x.shape
    _f32vec(w, C, "ln.weight")
    _f32vec(b, C, "ln.bias")
    if out_dtype == X3:
        assert out is None and x.dtype == torch.float32
        out = torch.empty((rows, 3 * C), dtype=torch.bfloat16, device=x.device)
        y_dt = nat.BF16X3
    else:
        if out is None:
            out = torch.empty((rows, C), dtype=out_dtype or x.dtype, device=x.device)
        assert out.is_contiguous() and out.shape == x.shape
        y_dt = _dt(out)
    nat.check(_lib().cor_layernorm(x.data_ptr(), _dt(x), out.data_ptr(), y_dt, w.data_ptr(), b.data_ptr(), rows, C,
                                   float(eps), act | (nat.ORDER_REVERSE if reverse else 0), _s()), "cor_layernorm")
    return out


def _attn_out(out, rows, cols, dtype, device, strided):
    """The output of an attention call: a fresh [rows, cols] tensor, or the caller's `out` held to the same shape and dtype. strided:
    the entry point takes a row stride (any stride(0) >= cols); otherwise `out` must be contiguous like the allocation it replaces."""
    if out is None:
        return torch.empty((rows, cols), dtype=dtype, device=device)
    assert out.is_cuda and out.device == device and out.dtype == dtype and out.dim() == 2 and tuple(out.shape) == (rows, cols), \
        (out.shape, out.dtype, out.device, rows, cols, dtype)
    if strided:
        assert out.stride(1) == 1 and (rows == 1 or out.stride(0) >= cols), out.stride()
    else:
        assert out.is_contiguous(), out.stride()
    return out


def attention(q, k, v, B, H, Tq, Tk, hd, scale, out_dtype=None, out=None):
    """q [B*Tq, >=H*hd] / k,v [B*Tk, ...] row-major 2-D views (e.g. column slices of a fused qkv activation).
    out: optional [B*Tq, H*hd] row-major view to write into (its row stride is passed on), of dtype out_dtype (default: q's)."""
    _dev(q, k, v, out)
    assert q.dtype == k.dtype == v.dtype
    for t, T in ((q, Tq), (k, Tk), (v, Tk)):
        assert t.dim() == 2 and t.stride(1) == 1 and t.shape[0] == B * T and t.shape[1] == H * hd, (t.shape, B, T, H, hd)
    out = _attn_out(out, B * Tq, H * hd, out_dtype or q.dtype, q.device, True)
    ld = out.stride(0) if B * Tq > 1 else max(out.stride(0), H * hd)
    nat.check(_lib().cor_attention(q.data_ptr(), Tq * q.stride(0), q.stride(0), k.data_ptr(), Tk * k.stride(0), k.stride(0),
                                   v.data_ptr(), Tk * v.stride(0), v.stride(0), _dt(q), out.data_ptr(), Tq * ld, ld,
                                   _dt(out), B, H, Tq, Tk, hd, float(scale), _s()), "cor_attention")
    return out


def attention_f32(q, k, v, B, H, Tq, Tk, hd, scale, out_dtype=torch.float32, out=None):
    """flash_fwd_f32 (cor_attention_f32): exact-fp32 MHA on the f32 matrix cores. q [B*Tq, >=H*hd] / k,v [B*Tk, ...] fp32 row-major 2-D
    views (e.g. column slices of an fp32 qkv activation) -> fp32 [B*Tq, H*hd] or, out_dtype X3, split rows [B*Tq, 3*H*hd].
    out: optional row-major view of that shape and type to write into (its row stride is passed on)."""
    _dev(q, k, v, out)
    for t, T in ((q, Tq), (k, Tk), (v, Tk)):
        assert t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1 and t.shape[0] == B * T and t.shape[1] == H * hd, (t.shape, B, T, H, hd)
    if out_dtype == X3:
        out = _attn_out(out, B * Tq, 3 * H * hd, torch.bfloat16, q.device, True)
        o_dt = nat.BF16X3
    else:
        assert out_dtype == torch.float32
        out = _attn_out(out, B * Tq, H * hd, torch.float32, q.device, True)
        o_dt = F32
    ld = out.stride(0) if B * Tq > 1 else max(out.stride(0), out.shape[1])
    nat.check(_lib().cor_attention_f32(q.data_ptr(), Tq * q.stride(0), q.stride(0), k.data_ptr(), Tk * k.stride(0), k.stride(0),
                                       v.data_ptr(), Tk * v.stride(0), v.stride(0), out.data_ptr(), Tq * ld, ld, o_dt,
                                       B, H, Tq, Tk, hd, float(scale), _s()), "cor_attention_f32")
    return out


def sam_attention(qkv, pad_row, rel_h, rel_w, B, H, grid, window, out_dtype=None, variant=0, q_prescale=1.0, reverse=False, out=None):
    """out: optional contiguous [B*grid*grid, H*hd] tensor to write into, of dtype out_dtype (default: qkv's)."""
    _dev(qkv, pad_row, rel_h, rel_w, out)
    hd = rel_h.shape[1]
    d = H * hd
    assert qkv.is_contiguous() and qkv.shape == (B * grid * grid, 3 * d), qkv.shape
    S = window if window > 0 else grid
    for r in (rel_h, rel_w):
        assert r.dtype == torch.float32 and r.is_contiguous() and r.shape == (2 * S - 1, hd), r.shape
    if window > 0:
        assert pad_row is not None and pad_row.dtype == qkv.dtype and pad_row.is_contiguous() and pad_row.numel() == 3 * d
    out = _attn_out(out, B * grid * grid, d, out_dtype or qkv.dtype, qkv.device, False)
    nat.check(_lib().cor_sam_attention(qkv.data_ptr(), _dt(qkv), out.data_ptr(), _dt(out), _p(pad_row), rel_h.data_ptr(),
                                       rel_w.data_ptr(), B, H, hd, grid, window, float(q_prescale), int(variant) | (nat.ORDER_REVERSE if reverse else 0), _s()), "cor_sam_attention")
    return out


def patchify(img, p, Kpad, out_dtype):
    if out_dtype == X3:
        return split_x3(patchify(img, p, Kpad, torch.float32))
    _dev(img)
    assert img.dtype == torch.float32 and img.is_contiguous() and img.dim() == 4
    B, C, H, W = img.shape
    out = torch.empty((B * (H // p) * (W // p), Kpad), dtype=out_dtype, device=img.device)
    nat.check(_lib().cor_patchify(img.data_ptr(), out.data_ptr(), _dt(out), B, C, H, W, p, Kpad, _s()), "cor_patchify")
    return out


def im2col3x3(x, B, H, W):
    _dev(x)
    C = x.shape[-1]
    assert x.is_contiguous() and x.numel() == B * H * W * C
    out = torch.empty((B * H * W, 9 * C), dtype=x.dtype, device=x.device)
    nat.check(_lib().cor_im2col3x3(x.data_ptr(), _dt(x), out.data_ptr(), B, H, W, C, _s()), "cor_im2col3x3")
    return out


def add(a, b, out_dtype=None, out=None):
    """a + b, b broadcast periodically over the flattened a (b.numel() must divide a.numel())."""
    _dev(a, b, out)
    assert a.is_contiguous() and b.is_contiguous() and a.numel() % b.numel() == 0
    if out is None:
        out = torch.empty(a.shape, dtype=out_dtype or a.dtype, device=a.device)
    assert out.is_contiguous() and out.numel() == a.numel()
    nat.check(_lib().cor_add(a.data_ptr(), _dt(a), b.data_ptr(), _dt(b), out.data_ptr(), _dt(out), a.numel(), b.numel(), _s()),
              "cor_add")
    return out


def copy_rows(src_ptr_tensor, ld_in, rows, C, out, ld_out=None, src_offset=0):
    """out[r, :C] = src[src_offset + r*ld_in : ... + C]; casts between fp32/bf16. ld_in == 0 broadcasts one row."""
    _dev(src_ptr_tensor, out)
    src = src_ptr_tensor
    assert src.is_contiguous()
    need = src_offset + (rows - 1) * ld_in + C
    assert need <= src.numel(), (need, src.numel())
    if ld_out is None:
        ld_out = out.stride(0) if out.dim() == 2 else C
    assert out.stride(-1) == 1
    nat.check(_lib().cor_copy_rows(src.data_ptr() + src_offset * src.element_size(), ld_in, _dt(src), out.data_ptr(), ld_out,
                                   _dt(out), rows, C, _s()), "cor_copy_rows")
    return out


def split_x3(x, out=None, seg=None):
    """fp32 rows x [rows, C] (row-major 2-D view) -> x3 split rows (cor_split_x3): lo at out[:, 0:C], hi at out[:, seg:seg+C] and
    out[:, 2seg:2seg+C]. out: a bf16 2-D view whose row stride holds 2*seg + C (default: new [rows, 3C], seg = C)."""
    _dev(x, out)
    rows, C, ld_in = _rows(x)
    assert x.dtype == torch.float32
    seg = C if seg is None else seg
    if out is None:
        out = torch.empty((rows, 3 * C), dtype=torch.bfloat16, device=x.device)
    assert out.dtype == torch.bfloat16 and out.dim() == 2 and out.stride(1) == 1 and out.shape[0] == rows
    ld_out = out.stride(0) if rows > 1 else out.shape[1]
    assert 2 * seg + C <= out.shape[1] and seg >= C, (seg, C, out.shape)
    nat.check(_lib().cor_split_x3(x.data_ptr(), ld_in, out.data_ptr(), ld_out, seg, rows, C, _s()), "cor_split_x3")
    return out


def cast(x, dtype):
    """Contiguous dtype conversion through cor_copy_rows (no-op when already `dtype`); dtype X3: fp32 -> x3 split rows."""
    if dtype == X3:
        assert x.dim() == 2 and x.is_contiguous()
        return split_x3(x)
    if x.dtype == dtype:
        return x
    assert x.is_contiguous()
    C = x.shape[-1]
    rows = x.numel() // C
    out = torch.empty(x.shape, dtype=dtype, device=x.device)
    return copy_rows(x, C, rows, C, out, ld_out=C)


def tokens_to_nchw(x, B, HW, C):
    _dev(x)
    assert x.is_contiguous() and x.numel() == B * HW * C
    out = torch.empty((B, C, HW), dtype=torch.float32, device=x.device)
    nat.check(_lib().cor_tokens_to_nchw(x.data_ptr(), _dt(x), out.data_ptr(), B, HW, C, _s()), "cor_tokens_to_nchw")
    return out


def nchw_to_tokens(x, out_dtype):
    _dev(x)
    assert x.dtype == torch.float32 and x.is_contiguous()
    B, C = x.shape[:2]
    HW = x.numel() // (B * C)
    out = torch.empty((B * HW, C), dtype=out_dtype, device=x.device)
    nat.check(_lib().cor_nchw_to_tokens(x.data_ptr(), out.data_ptr(), _dt(out), B, HW, C, _s()), "cor_nchw_to_tokens")
    return out


def l2norm_rows(x, eps=1e-12, out_dtype=None):
    _dev(x)
    assert x.is_contiguous() and x.dim() == 2
    out = torch.empty(x.shape, dtype=out_dtype or x.dtype, device=x.device)
    nat.check(_lib().cor_l2norm_rows(x.data_ptr(), _dt(x), out.data_ptr(), _dt(out), x.shape[0], x.shape[1], float(eps), _s()),
              "cor_l2norm_rows")
    return out


def embed_tokens(ids, table, pos):
    _dev(ids, table, pos)
    assert ids.dtype == torch.int64 and ids.is_contiguous() and ids.dim() == 2
    N, ctx = ids.shape
    vocab, D = table.shape
    assert table.dtype == torch.float32 and table.is_contiguous() and pos.dtype == torch.float32 and pos.is_contiguous()
    assert pos.shape[0] >= ctx and pos.shape[1] == D
    out = torch.empty((N * ctx, D), dtype=torch.float32, device=ids.device)
    nat.check(_lib().cor_embed_tokens(ids.data_ptr(), table.data_ptr(), pos.data_ptr(), out.data_ptr(), N * ctx, ctx, D, vocab, _s()),
              "cor_embed_tokens")
    return out


def bilinear(x, OH, OW, clamp01=False):
    _dev(x)
    assert x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 4
    B, C, H, W = x.shape
    out = torch.empty((B, C, OH, OW), dtype=torch.float32, device=x.device)
    nat.check(_lib().cor_bilinear(x.data_ptr(), out.data_ptr(), B * C, H, W, OH, OW, int(clamp01), _s()), "cor_bilinear")
    return out


def conv3x3s2_small(x, channels_last, w, bias, B, Cin, H, W):
    _dev(x, w, bias)
    Cout = w.shape[0]
    assert x.dtype == torch.float32 and x.is_contiguous() and x.numel() == B * Cin * H * W
    assert w.dtype == torch.float32 and w.is_contiguous() and w.shape == (Cout, Cin, 3, 3)
    _f32vec(bias, Cout, "conv.bias")
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    out = torch.empty((B, OH, OW, Cout), dtype=torch.float32, device=x.device)
    nat.check(_lib().cor_conv3x3s2_small(x.data_ptr(), int(channels_last), w.data_ptr(), _p(bias), out.data_ptr(), B, Cin, Cout, H, W,
                                         _s()), "cor_conv3x3s2_small")
    return out


def dwconv7x7(x, w_t, bias, B, H, W, out_dtype=torch.float32):
    _dev(x, w_t, bias)
    C = x.shape[-1]
    assert x.dtype == torch.float32 and x.is_contiguous() and x.numel() == B * H * W * C
    assert w_t.dtype == torch.float32 and w_t.is_contiguous() and w_t.shape == (49, C)
    _f32vec(bias, C, "dwconv.bias")
    out = torch.empty((B * H * W, C), dtype=out_dtype, device=x.device)
    nat.check(_lib().cor_dwconv7x7(x.data_ptr(), w_t.data_ptr(), bias.data_ptr(), out.data_ptr(), _dt(out), B, H, W, C, _s()),
              "cor_dwconv7x7")
    return out


def adapter_pool(maps, feat, B, P, M, D):
    _dev(maps, feat)
    assert maps.dtype == torch.float32 and maps.is_contiguous() and maps.numel() == B * P * M
    assert feat.dtype == torch.float32 and feat.is_contiguous() and feat.numel() == B * P * D
    out = torch.empty((B, D), dtype=torch.float32, device=maps.device)
    nat.check(_lib().cor_adapter_pool(maps.data_ptr(), feat.data_ptr(), out.data_ptr(), B, P, M, D, _s()), "cor_adapter_pool")
    return out


def masked_pool(feat, mask, B, P, D, feat_nchw=False, clamp01=False, l2norm=False):
    _dev(feat, mask)
    assert feat.dtype == torch.float32 and feat.is_contiguous() and feat.numel() == B * P * D
    assert mask.dtype == torch.float32 and mask.is_contiguous() and mask.numel() == B * P
    out = torch.empty((B, D), dtype=torch.float32, device=feat.device)
    nat.check(_lib().cor_masked_pool(feat.data_ptr(), int(feat_nchw), mask.data_ptr(), out.data_ptr(), B, P, D, int(clamp01),
                                     int(l2norm), _s()), "cor_masked_pool")
    return out


def region_pool(tokens, masks, region_offsets, B, P, D, out_dtype=torch.float32, clamp01=False, l2norm=False):
    """R masks pooled against the tokens of B images, every image's tokens read once per tile of regions (cor_region_pool).
    tokens f32 [B,P,D] channels-last, masks f32 [R,P], region_offsets int32 [B+1] on the device (CSR: regions [off[b], off[b+1]) belong
    to image b) -> [R,D] in out_dtype (float32 / bfloat16 / float16). An f32 row has the bits masked_pool gives for that mask alone."""
    _dev(tokens, masks, region_offsets)
    assert tokens.dtype == torch.float32 and tokens.is_contiguous() and tokens.numel() == B * P * D
    assert masks.dtype == torch.float32 and masks.is_contiguous() and masks.numel() % P == 0
    assert region_offsets.dtype == torch.int32 and region_offsets.is_contiguous() and region_offsets.numel() == B + 1
    assert out_dtype in _DT, f"region_pool: out_dtype {out_dtype}"
    R = masks.numel() // P
    out = torch.empty((R, D), dtype=out_dtype, device=tokens.device)
    if R == 0 or B == 0:
        return out
    nat.check(_lib().cor_region_pool(tokens.data_ptr(), masks.data_ptr(), region_offsets.data_ptr(), out.data_ptr(), _DT[out_dtype],
                                     B, R, P, D, int(clamp01), int(l2norm), _s()), "cor_region_pool")
    return out


def fuse_gate(img, txt, aI, aT):
    _dev(img, txt, aI, aT)
    N, D = img.shape
    for t in (img, txt, aI, aT):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.shape == (N, D)
    cat = torch.empty((N, 2 * D), dtype=torch.float32, device=img.device)
    nat.check(_lib().cor_fuse_gate(img.data_ptr(), txt.data_ptr(), aI.data_ptr(), aT.data_ptr(), cat.data_ptr(), N, D, _s()),
              "cor_fuse_gate")
    return cat


def fuse_mix(cat, dyn):
    _dev(cat, dyn)
    N, D2 = cat.shape
    assert cat.dtype == torch.float32 and cat.is_contiguous() and dyn.dtype == torch.float32 and dyn.is_contiguous() and dyn.numel() == N
    out = torch.empty((N, D2 // 2), dtype=torch.float32, device=cat.device)
    nat.check(_lib().cor_fuse_mix(cat.data_ptr(), dyn.data_ptr(), out.data_ptr(), N, D2 // 2, _s()), "cor_fuse_mix")
    return out


def dense_pe(gauss, size):
    _dev(gauss)
    assert gauss.dtype == torch.float32 and gauss.is_contiguous() and gauss.dim() == 2 and gauss.shape[0] == 2
    F = gauss.shape[1]
    out = torch.empty((size * size, 2 * F), dtype=torch.float32, device=gauss.device)
    nat.check(_lib().cor_dense_pe(gauss.data_ptr(), out.data_ptr(), size, F, _s()), "cor_dense_pe")
    return out


def upscale_shuffle(y, B, H, W, Cout, bias=None, ln_w=None, ln_b=None, eps=1e-6, act=ACT_NONE, out_dtype=None):
    _dev(y, bias, ln_w, ln_b)
    assert y.is_contiguous() and y.shape == (B * H * W, 4 * Cout)
    _f32vec(bias, Cout, "bias")
    _f32vec(ln_w, Cout, "ln_w")
    _f32vec(ln_b, Cout, "ln_b")
    out = torch.empty((B * 4 * H * W, Cout), dtype=out_dtype or y.dtype, device=y.device)
    nat.check(_lib().cor_upscale_shuffle(y.data_ptr(), _dt(y), _p(bias), _p(ln_w), _p(ln_b), float(eps), act, out.data_ptr(), _dt(out),
                                         B, H, W, Cout, _s()), "cor_upscale_shuffle")
    return out


def upscale_hyper(x, w, bias, hyper, B, H, W, Kmask):
    """x [B*H*W, 64] -> masks [B, Kmask, 2H, 2W]; hyper [B, Kmask, 32] fp32 (may be a strided view over dim 0)."""
    _dev(x, w, bias, hyper)
    assert x.is_contiguous() and x.shape == (B * H * W, 64)
    assert w.dtype == torch.float32 and w.is_contiguous() and w.shape == (64, 32, 2, 2)
    _f32vec(bias, 32, "bias")
    assert hyper.dtype == torch.float32 and hyper.shape == (B, Kmask, 32) and hyper.stride(2) == 1 and hyper.stride(1) == 32
    masks = torch.empty((B, Kmask, 2 * H, 2 * W), dtype=torch.float32, device=x.device)
    nat.check(_lib().cor_upscale_hyper(x.data_ptr(), _dt(x), w.data_ptr(), bias.data_ptr(), hyper.data_ptr(),
                                       hyper.stride(0) if B > 1 else Kmask * 32, masks.data_ptr(), B, H, W, 64, 32, Kmask, _s()),
              "cor_upscale_hyper")
    return masks


def iou_select(iou, hyper, k_off, Ksel):
    _dev(iou, hyper)
    B, Kall = iou.shape
    C = hyper.shape[-1]
    assert iou.dtype == torch.float32 and iou.is_contiguous() and hyper.dtype == torch.float32 and hyper.is_contiguous()
    assert hyper.shape == (B, Kall, C)
    best = torch.empty((B,), dtype=torch.int64, device=iou.device)
    sel = torch.empty((B, 1, C), dtype=torch.float32, device=iou.device)
    nat.check(_lib().cor_iou_select(iou.data_ptr(), hyper.data_ptr(), B, Kall, k_off, Ksel, C, best.data_ptr(), sel.data_ptr(), _s()),
              "cor_iou_select")
    return best, sel


_FILTER_MODES = {"eq": nat.FILTER_EQ, "ne": nat.FILTER_NE}


def _topk_front(who, Q, G, k, mode="eq", labels=None):
    """The argument checks the similarity_topk* wrappers share, before anything touches the device: k, the filter mode, the label pair
    (both or neither), then device, dtype and shapes. Returns (Bq, Ng, C)."""
    if not 1 <= int(k) <= nat.TOPK_KMAX:
        raise ValueError(f"{who}: k must be in [1, {nat.TOPK_KMAX}], got {k}")
    if mode not in _FILTER_MODES:
        raise ValueError(f"{who}: mode must be 'eq' or 'ne', got {mode!r}")
    if labels is not None and (labels[0] is None) != (labels[1] is None):
        raise ValueError(f"{who}: row_labels and query_labels go together (both or neither)")
    _dev(Q, G)
    assert Q.dtype == torch.float32 and Q.is_contiguous() and G.is_contiguous() and Q.dim() == 2 and G.dim() == 2
    Bq, Cq = Q.shape
    Ng, Cg = G.shape
    assert Cq == Cg
    return Bq, Ng, Cq


def _topk_buffers(bytes_fn, Q, Bq, Ng, k):
    """(workspace, scores f32[Bq,k], idx i64[Bq,k]) of one search; bytes_fn names the route's cor_topk*_workspace_bytes."""
    nbytes = getattr(_lib(), bytes_fn)(Bq, Ng, k)
    if nbytes < 0:
        nat.check(int(nbytes), bytes_fn)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=Q.device)          # torch's allocator returns >= 256-B aligned blocks
    scores = torch.empty((Bq, k), dtype=torch.float32, device=Q.device)
    idx = torch.empty((Bq, k), dtype=torch.int64, device=Q.device)
    return ws, scores, idx


def similarity_topk(Q, G, k, g_offset=0, flags=0):
    """Top-k gallery rows per query by dot product; (score desc, index asc). Q fp32 [Bq,C]; G [Ng,C] fp32/bf16/fp16;
    1 <= k <= nat.TOPK_KMAX (256); Ng < k: the tail is (-inf, -1).
    k <= 32: fp32 galleries and 16-bit galleries with C = 256 are bit-identical to the CPU fmaf-chain oracle
    (oracle/c/sim_chain.c), scores and indices. 33 <= k <= 256 (the wide route: Recall@50/100, two-stage re-ranking): every
    gallery dtype and every C is bit-identical to that oracle. A candidate overflow (pathological score distributions) is
    repaired ON THE DEVICE: no host synchronisation here. flags: nat.TOPK_FORCE_LISTS | nat.TOPK_NO_FALLBACK (tests);
    TOPK_FORCE_LISTS and TOPK_WAVE_FINAL need k <= 32."""
    Bq, Ng, C = _topk_front("similarity_topk", Q, G, k)
    ws, scores, idx = _topk_buffers("cor_topk_workspace_bytes", Q, Bq, Ng, k)
    nat.check(_lib().cor_similarity_topk(Q.data_ptr(), G.data_ptr(), _dt(G), Bq, Ng, C, k, int(g_offset), scores.data_ptr(),
                                         idx.data_ptr(), ws.data_ptr(), int(flags), _s()), "cor_similarity_topk")
    return scores, idx


def _label_vec(t, n, name, who):
    """The shape and dtype checks of a label vector (nothing moves)."""
    t = torch.as_tensor(t)
    if t.dim() != 1 or t.shape[0] != n:
        raise ValueError(f"{who}: {name} must be a vector of {n} labels, got shape {tuple(t.shape)}")
    if t.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{who}: {name} must be int32 (int64 is converted), got {t.dtype}")
    return t


def _labels(t, n, name, device, who="similarity_topk_filtered"):
    t = _label_vec(t, n, name, who).to(device=device, dtype=torch.int32).contiguous()
    if t.data_ptr() % 16:                                     # the kernels read row labels 16 B at a time (a view into a larger tensor)
        t = t.clone()
    return t


def similarity_topk_filtered(Q, G, k, row_labels, query_labels, mode="eq", g_offset=0, flags=0):
    """similarity_topk over the ALLOWED rows only: row g is allowed for query b if query_labels[b] < 0 (unrestricted) or, for
    mode "eq", row_labels[g] == query_labels[b] (restrict to a class / subset), for mode "ne", row_labels[g] != query_labels[b]
    (exclude a source, e.g. the query's own image). row_labels int32[Ng], query_labels int32[Bq] (int64 is converted). 1 <= k <= 256
    for every gallery dtype and C; bit-identical to the chain oracle on the allowed rows; fewer than k allowed rows: the tail is
    (-inf, -1). No host synchronisation when the labels already live on the device. flags: nat.TOPK_NO_FALLBACK (tests)."""
    Bq, Ng, C = _topk_front("similarity_topk_filtered", Q, G, k, mode)
    rl = _labels(row_labels, Ng, "row_labels", Q.device)
    qlab = _labels(query_labels, Bq, "query_labels", Q.device)
    ws, scores, idx = _topk_buffers("cor_topk_filtered_workspace_bytes", Q, Bq, Ng, k)
    nat.check(_lib().cor_similarity_topk_filtered(Q.data_ptr(), G.data_ptr(), _dt(G), Bq, Ng, C, k, int(g_offset), rl.data_ptr(),
                                                  qlab.data_ptr(), _FILTER_MODES[mode], scores.data_ptr(), idx.data_ptr(), ws.data_ptr(),
                                                  int(flags), _s()), "cor_similarity_topk_filtered")
    return scores, idx


def _range_floors(thresholds, Bq, who):
    """The shape and dtype checks of the floors of a range search (nothing moves): a Python number, or an f32 tensor [Bq]."""
    if isinstance(thresholds, (int, float)) and not isinstance(thresholds, bool):
        return float(thresholds)
    if not isinstance(thresholds, torch.Tensor):
        raise ValueError(f"{who}: thresholds must be a float or an f32 tensor [{Bq}], got {type(thresholds).__name__}")
    if thresholds.dim() != 1 or thresholds.shape[0] != Bq:
        raise ValueError(f"{who}: thresholds must have shape ({Bq},), got {tuple(thresholds.shape)}")
    if thresholds.dtype != torch.float32:
        raise ValueError(f"{who}: thresholds must be float32, got {thresholds.dtype}")
    return thresholds


def _range_front(who, Q, G, thresholds, k, mode="eq"):
    """The argument checks the range wrappers share, before anything touches the device (k, the floors, then _topk_front), and the floors
    as a device vector: (Bq, Ng, C, thr f32 [Bq])."""
    if not 1 <= int(k) <= nat.TOPK_KMAX:
        raise ValueError(f"{who}: k must be in [1, {nat.TOPK_KMAX}], got {k}")
    if isinstance(Q, torch.Tensor) and Q.dim() == 2:
        thresholds = _range_floors(thresholds, Q.shape[0], who)
    Bq, Ng, C = _topk_front(who, Q, G, k, mode)
    if isinstance(thresholds, float):
        thr = torch.full((Bq,), thresholds, dtype=torch.float32, device=Q.device)
    else:
        _dev(thresholds)
        thr = thresholds.contiguous()
    return Bq, Ng, C, thr


def similarity_range(Q, G, thresholds, k, g_offset=0, flags=0):
    """Threshold search: per query b the rows whose score is at least thresholds[b], and how many there are.
    Returns (scores f32[Bq,k], idx i64[Bq,k], count i32[Bq]). The score is similarity_topk's fmaf-chain score (oracle/c/sim_chain.c; 16-bit
    rows widened exactly, the query rounded to the gallery dtype); membership is the IEEE `score >= floor` (a NaN floor: no row; -inf:
    every row; +0.0 and -0.0 are one floor). count[b] is the EXACT number of members for any gallery size; the lists hold the first k
    members by (score desc, index asc) and then the (-inf, -1) tail, i.e. similarity_topk's lists with every entry below the floor
    turned into tail. Scores, indices and counts are bit-identical to that definition on the CPU for fp32 / bf16 / fp16 rows, every C
    and 1 <= k <= 256.
    thresholds: a Python float (broadcast by a device fill, no host scalar assignment) or an f32 tensor [Bq] on Q's device.
    Route (include/cor_amd.h): the wide route's sample and threshold, then one full scan that appends the list candidates, counts the
    rows at least delta_q above the floor in registers and appends the rows within delta_q of it for the chain to decide; delta_q is
    twice the bound of |scan score - chain score|, so neither decision can differ from the chain's. No allocation inside the call, no
    host synchronisation, capturable in a graph. A candidate overflow is repaired on the device by a chain pass that ranks and counts.
    flags: nat.TOPK_NO_FALLBACK (tests: an overflowed query carries index -2 in every slot and count -2)."""
    Bq, Ng, C, thr = _range_front("similarity_range", Q, G, thresholds, k)
    ws, scores, idx = _topk_buffers("cor_range_workspace_bytes", Q, Bq, Ng, k)
    count = torch.empty((Bq,), dtype=torch.int32, device=Q.device)
    nat.check(_lib().cor_similarity_range(Q.data_ptr(), G.data_ptr(), _dt(G), Bq, Ng, C, thr.data_ptr(), k, int(g_offset), scores.data_ptr(),
                                          idx.data_ptr(), count.data_ptr(), ws.data_ptr(), int(flags), _s()), "cor_similarity_range")
    return scores, idx, count


def similarity_range_filtered(Q, G, thresholds, k, row_labels, query_labels, mode="eq", g_offset=0, flags=0):
    """similarity_range over the ALLOWED rows only (the rule of similarity_topk_filtered: query_labels[b] < 0 is unrestricted, mode "eq"
    keeps the rows that carry the query's label, "ne" the rows that do not). Returns (scores f32[Bq,k], idx i64[Bq,k], count i32[Bq]):
    count[b] is the EXACT number of allowed rows whose chain score is at least thresholds[b]; the lists are similarity_topk_filtered's
    with every entry below the floor turned into (-inf, -1) tail; a query with no allowed row gets count 0 and only the tail. Bit-identical
    to that definition for fp32 / bf16 / fp16 rows, every C and 1 <= k <= 256. Typical use: mode "ne" with the query's own image id asks
    "does this region already exist in ANOTHER image" (count > 0). thresholds as in similarity_range; labels as in
    similarity_topk_filtered (int32, int64 is converted). No allocation inside the call, no host synchronisation when floors and labels
    already live on the device, capturable in a graph. flags: nat.TOPK_NO_FALLBACK (tests: index -2 in every slot and count -2)."""
    who = "similarity_range_filtered"
    Bq, Ng, C, thr = _range_front(who, Q, G, thresholds, k, mode)
    rl = _labels(row_labels, Ng, "row_labels", Q.device, who)
    qlab = _labels(query_labels, Bq, "query_labels", Q.device, who)
    ws, scores, idx = _topk_buffers("cor_range_filtered_workspace_bytes", Q, Bq, Ng, k)
    count = torch.empty((Bq,), dtype=torch.int32, device=Q.device)
    nat.check(_lib().cor_similarity_range_filtered(Q.data_ptr(), G.data_ptr(), _dt(G), Bq, Ng, C, thr.data_ptr(), k, int(g_offset), rl.data_ptr(),
                                                   qlab.data_ptr(), _FILTER_MODES[mode], scores.data_ptr(), idx.data_ptr(), count.data_ptr(),
                                                   ws.data_ptr(), int(flags), _s()), "cor_similarity_range_filtered")
    return scores, idx, count


def similarity_topk_distinct(Q, G, k, row_groups, row_labels=None, query_labels=None, mode="eq", g_offset=0, flags=0):
    """Top-k DISTINCT groups: row_groups int32[Ng] gives every gallery row a group id (the source image of a region; a negative id
    makes the row a group of its own). Per query, each group's representative is its best allowed row by (chain score desc, index
    asc); the result is the k best representatives in that order: scores f32[Bq,k], idx i64[Bq,k] (global ROW ids, no group twice;
    fewer than k groups: the (-inf, -1) tail). row_labels / query_labels / mode: the optional filter of similarity_topk_filtered
    (both or neither; labels and group ids are separate vectors and may be the same tensor), e.g. mode "ne" with the query's own
    image id. 1 <= k <= 256 for every gallery dtype and C; bit-identical to "chain-rank the allowed rows, keep the first row of each
    group, keep the first k". No host synchronisation when the vectors already live on the device. flags: nat.TOPK_NO_FALLBACK."""
    who = "similarity_topk_distinct"
    Bq, Ng, C = _topk_front(who, Q, G, k, mode, (row_labels, query_labels))
    rg = _labels(row_groups, Ng, "row_groups", Q.device, who)
    rl = _labels(row_labels, Ng, "row_labels", Q.device, who) if row_labels is not None else None
    qlab = _labels(query_labels, Bq, "query_labels", Q.device, who) if query_labels is not None else None
    ws, scores, idx = _topk_buffers("cor_topk_distinct_workspace_bytes", Q, Bq, Ng, k)
    nat.check(_lib().cor_similarity_topk_distinct(Q.data_ptr(), G.data_ptr(), _dt(G), Bq, Ng, C, k, int(g_offset), rg.data_ptr(),
                                                  rl.data_ptr() if rl is not None else None, qlab.data_ptr() if qlab is not None else None,
                                                  _FILTER_MODES[mode], scores.data_ptr(), idx.data_ptr(), ws.data_ptr(), int(flags), _s()),
              "cor_similarity_topk_distinct")
    return scores, idx


def quantize_rows_i8(X):
    """Per-row scalar quantisation: X [n,C] fp32 / bf16 / fp16 (finite values) -> (q int8 [n,C], scale f32 [n]) on the GPU, X untouched.
    Per row amax = max|x| in fp32; amax == 0: scale 0 and q 0; else q = clamp(rint(x * (127 / amax)), -127, 127) (half to even) and
    scale = amax / 127, every step one rounded fp32 operation (include/cor_amd.h). C % 16 == 0, C <= 256."""
    if X.dim() != 2 or X.dtype not in _DT:
        raise ValueError(f"quantize_rows_i8: X must be [n, C] in float32 / bfloat16 / float16, got {X.dtype} {tuple(X.shape)}")
    n, C = X.shape
    if C < 16 or C > 256 or C % 16:
        raise ValueError(f"quantize_rows_i8: C must be a multiple of 16 up to 256, got {C}")
    _dev(X)
    X = X.contiguous()
    if X.data_ptr() % 16:                                     # a view into a larger tensor: the kernel loads 16 B at a time
        X = X.clone()
    q = torch.empty((n, C), dtype=torch.int8, device=X.device)
    scale = torch.empty((n,), dtype=torch.float32, device=X.device)
    nat.check(_lib().cor_quantize_rows_i8(X.data_ptr(), _dt(X), n, C, q.data_ptr(), scale.data_ptr(), _s()), "cor_quantize_rows_i8")
    return q, scale


def dequantize_rows_i8(q, scale, out_dtype=torch.float32, out=None):
    """The way back from quantize_rows_i8 (cor_dequantize_rows_i8): q int8 [n,C], scale f32 [n] -> X [n,C] in out_dtype on the GPU,
    x = float(q) * scale[row], ONE rounded fp32 multiply, stored as float32 or rounded again (nearest even) to bfloat16 / float16 (what
    .to(dtype) of the fp32 result gives). C % 16 == 0, C <= 256. out: an optional contiguous [n,C] tensor of out_dtype to write into.
    No host synchronisation; capturable in a graph."""
    if q.dim() != 2 or q.dtype != torch.int8:
        raise ValueError(f"dequantize_rows_i8: q must be int8 [n, C], got {q.dtype} {tuple(q.shape)}")
    n, C = q.shape
    if scale.dtype != torch.float32 or scale.dim() != 1 or scale.shape[0] != n:
        raise ValueError(f"dequantize_rows_i8: scale must be float32 [{n}], got {scale.dtype} {tuple(scale.shape)}")
    if C < 16 or C > 256 or C % 16:
        raise ValueError(f"dequantize_rows_i8: C must be a multiple of 16 up to 256, got {C}")
    if out_dtype not in _DT:
        raise ValueError(f"dequantize_rows_i8: out_dtype must be float32 / bfloat16 / float16, got {out_dtype}")
    if out is not None and (out.shape != (n, C) or out.dtype != out_dtype or not out.is_contiguous()):
        raise ValueError(f"dequantize_rows_i8: out must be a contiguous {out_dtype} [{n}, {C}] tensor")
    dev = _dev(q, scale, out)
    q, scale = q.contiguous(), scale.contiguous()
    if q.data_ptr() % 16:                                     # a view into a larger tensor: the kernel loads 16 B at a time
        q = q.clone()
    dst = out if out is not None and out.data_ptr() % 16 == 0 else torch.empty((n, C), dtype=out_dtype, device=dev)
    if n:                                                     # (no rows: empty tensors have no address to pass)
        nat.check(_lib().cor_dequantize_rows_i8(q.data_ptr(), scale.data_ptr(), n, C, dst.data_ptr(), _DT[out_dtype], _s()),
                  "cor_dequantize_rows_i8")
    if out is not None and dst is not out:
        out.copy_(dst)
        dst = out
    return dst


def _i8_front(who, Q, Gq, gscale, k, flags, mode="eq"):
    """The checks the int8 searches share, before anything touches the device. Returns (Bq, Ng, C, gscale as the scan reads it)."""
    if Gq.dtype != torch.int8:
        raise ValueError(f"{who}: Gq must be int8 rows (ops.quantize_rows_i8), got {Gq.dtype}")
    if gscale.dtype != torch.float32 or gscale.dim() != 1 or Gq.dim() != 2 or gscale.shape[0] != Gq.shape[0]:
        raise ValueError(f"{who}: gscale must be float32 [Ng] for Gq [Ng, C], got {gscale.dtype} {tuple(gscale.shape)} for {tuple(Gq.shape)}")
    if int(flags) & ~nat.TOPK_NO_FALLBACK:
        raise ValueError(f"{who}: flags must be 0 or TOPK_NO_FALLBACK, got {flags}")
    Bq, Ng, C = _topk_front(who, Q, Gq, k, mode)
    _dev(Q, gscale)
    gscale = gscale.contiguous()
    if gscale.data_ptr() % 16:                                # a view into a larger tensor: the scan loads four scales at a time
        gscale = gscale.clone()
    return Bq, Ng, C, gscale


def similarity_topk_i8(Q, Gq, gscale, k, g_offset=0, flags=0):
    """similarity_topk over an int8 gallery: Q fp32 [Bq,C]; Gq int8 [Ng,C] and gscale f32 [Ng] as quantize_rows_i8 returns them. The query
    is quantised the same way inside the call; score = ((float)(int32 dot) * qscale) * gscale, exact in any summation order, ranked by
    (score key desc, index asc): bit-identical to tests/i8_refs.py, scores and indices. 1 <= k <= 256, C % 16 == 0, C <= 256; Ng < k:
    the tail is (-inf, -1). One route for every k; a candidate overflow is repaired on the device. flags: 0 or nat.TOPK_NO_FALLBACK."""
    Bq, Ng, C, gscale = _i8_front("similarity_topk_i8", Q, Gq, gscale, k, flags)
    ws, scores, idx = _topk_buffers("cor_topk_i8_workspace_bytes", Q, Bq, Ng, k)
    nat.check(_lib().cor_similarity_topk_i8(Q.data_ptr(), Gq.data_ptr(), gscale.data_ptr(), Bq, Ng, C, k, int(g_offset), scores.data_ptr(),
                                            idx.data_ptr(), ws.data_ptr(), int(flags), _s()), "cor_similarity_topk_i8")
    return scores, idx


def similarity_topk_i8_filtered(Q, Gq, gscale, k, row_labels, query_labels, mode="eq", g_offset=0, flags=0):
    """similarity_topk_i8 over the ALLOWED rows only: the score and order of similarity_topk_i8, the allowed rows of
    similarity_topk_filtered (query_labels[b] < 0: unrestricted; mode "eq": row_labels[g] == query_labels[b]; mode "ne": !=).
    row_labels int32[Ng], query_labels int32[Bq] (int64 is converted, a misaligned view is realigned). Bit-identical to
    tests/i8_filtered_refs.py, scores and indices; fewer than k allowed rows: those, then the (-inf, -1) tail. One route for every k, the
    filter inside the int8 scan; an overflowed query is ranked over its allowed rows on the device. No host synchronisation when the
    labels already live on the device. flags: 0 or nat.TOPK_NO_FALLBACK."""
    who = "similarity_topk_i8_filtered"
    if Gq.dim() == 2 and Q.dim() == 2:                        # the label checks raise before anything touches the device
        _label_vec(row_labels, Gq.shape[0], "row_labels", who)
        _label_vec(query_labels, Q.shape[0], "query_labels", who)
    Bq, Ng, C, gscale = _i8_front(who, Q, Gq, gscale, k, flags, mode)
    rl = _labels(row_labels, Ng, "row_labels", Q.device, who)
    qlab = _labels(query_labels, Bq, "query_labels", Q.device, who)
    ws, scores, idx = _topk_buffers("cor_topk_i8_filtered_workspace_bytes", Q, Bq, Ng, k)
    nat.check(_lib().cor_similarity_topk_i8_filtered(Q.data_ptr(), Gq.data_ptr(), gscale.data_ptr(), Bq, Ng, C, k, int(g_offset), rl.data_ptr(),
                                                     qlab.data_ptr(), _FILTER_MODES[mode], scores.data_ptr(), idx.data_ptr(), ws.data_ptr(),
                                                     int(flags), _s()), "cor_similarity_topk_i8_filtered")
    return scores, idx


def similarity_topk_i8_distinct(Q, Gq, gscale, k, row_groups, row_labels=None, query_labels=None, mode="eq", g_offset=0, flags=0):
    """Top-k DISTINCT groups of an int8 gallery: the score and order of similarity_topk_i8, the groups and allowed rows of
    similarity_topk_distinct. row_groups int32[Ng] (a negative id: a group of its own); per query, a group's representative is its first
    allowed row by (score key desc, index asc) and the result is the k best representatives in that order: scores f32[Bq,k], idx
    i64[Bq,k] (global ROW ids, no group twice; fewer than k groups: the (-inf, -1) tail). row_labels / query_labels / mode: the optional
    filter (both or neither; may be the group tensor itself, e.g. mode "ne" with the query's own image id). int64 ids are converted, a
    misaligned view is realigned. Bit-identical to tests/i8_distinct_refs.py, scores and indices. One route for every k; an overflowed
    query is ranked on the device. No host synchronisation when the vectors already live on the device. flags: 0 or
    nat.TOPK_NO_FALLBACK."""
    who = "similarity_topk_i8_distinct"
    if (row_labels is None) != (query_labels is None):
        raise ValueError(f"{who}: row_labels and query_labels go together (both or neither)")
    if Gq.dim() == 2 and Q.dim() == 2:                        # the id checks raise before anything touches the device
        _label_vec(row_groups, Gq.shape[0], "row_groups", who)
        if row_labels is not None:
            _label_vec(row_labels, Gq.shape[0], "row_labels", who)
            _label_vec(query_labels, Q.shape[0], "query_labels", who)
    Bq, Ng, C, gscale = _i8_front(who, Q, Gq, gscale, k, flags, mode)
    rg = _labels(row_groups, Ng, "row_groups", Q.device, who)
    rl = _labels(row_labels, Ng, "row_labels", Q.device, who) if row_labels is not None else None
    qlab = _labels(query_labels, Bq, "query_labels", Q.device, who) if query_labels is not None else None
    ws, scores, idx = _topk_buffers("cor_topk_i8_distinct_workspace_bytes", Q, Bq, Ng, k)
    nat.check(_lib().cor_similarity_topk_i8_distinct(Q.data_ptr(), Gq.data_ptr(), gscale.data_ptr(), Bq, Ng, C, k, int(g_offset), rg.data_ptr(),
                                                     rl.data_ptr() if rl is not None else None, qlab.data_ptr() if qlab is not None else None,
                                                     _FILTER_MODES[mode], scores.data_ptr(), idx.data_ptr(), ws.data_ptr(), int(flags), _s()),
              "cor_similarity_topk_i8_distinct")
    return scores, idx


def _list_front(who, scores, idx):
    """The checks of a (scores f32, idx i64) [Bq,kin] list as a search, the merge or the re-scoring return it. Returns (Bq, kin)."""
    if scores.dim() != 2 or scores.shape[1] < 1 or scores.dtype != torch.float32:
        raise ValueError(f"{who}: scores must be float32 [Bq, kin] with kin >= 1, got {scores.dtype} {tuple(scores.shape)}")
    if idx.shape != scores.shape or idx.dtype != torch.int64:
        raise ValueError(f"{who}: idx must be int64 {tuple(scores.shape)}, got {idx.dtype} {tuple(idx.shape)}")
    return scores.shape


def _disjoint_spans(who, segments):
    """ValueError if the id ranges of two non-empty segments [(rows-like, .., offset)] overlap."""
    spans = sorted((seg[-1], seg[-1] + seg[0].shape[0]) for seg in segments if seg[0].shape[0])
    for (_, hi), (lo, _) in zip(spans, spans[1:]):
        if lo < hi:
            raise ValueError(f"{who}: the segments' id ranges overlap")


def _seg_arrays(offsets, *tensors):
    """The ctypes segment table of a call, never zero-length: one pointer array per list of tensors (NULL for an empty tensor), the offsets,
    the row counts of the first list."""
    c, n = nat.C, max(len(offsets), 1)
    ptrs = [(c.c_void_p * n)(*[t.data_ptr() or None for t in ts]) for ts in tensors]
    return (*ptrs, (c.c_longlong * n)(*offsets), (c.c_int * n)(*[t.shape[0] for t in tensors[0]]))


def _list_outputs(Bq, k, dev, third, missing=False):
    """(scores f32, idx i64, third i32 or None), each [Bq,k]: a list kernel's outputs; missing: the (-inf, -1, -1) lists instead of empty tensors."""
    new = (lambda v, dt: torch.full((Bq, k), v, dtype=dt, device=dev)) if missing else (lambda v, dt: torch.empty((Bq, k), dtype=dt, device=dev))
    return new(float("-inf"), torch.float32), new(-1, torch.int64), new(-1, torch.int32) if third else None


def merge_topk(scores, idx, k, groups=None):
    """Merge P top-k lists per query on the device (cor_merge_topk): scores f32 [P,B,kin], idx i64 [P,B,kin] (global row ids; < 0 =
    missing, ranked after every present entry), as P searches return them, stacked -> (scores f32[B,k], idx i64[B,k]) ordered by
    (score desc, index asc) with the (-inf, -1) tail. groups i32 [P,B,kin] (one id per entry): the distinct merge, the best entry
    per non-negative group id, and a third result, the survivors' group ids i32[B,k] (-1 in the tail), so that a merged list can be
    merged again. Bitwise equal to retrieval.merge_topk_host / merge_topk_distinct_host on the same lists. 1 <= k <= 256;
    P * kin <= nat.MERGE_NMAX (4096) entries per query in one launch, beyond that NativeError (retrieval.merge_topk_device merges
    in rounds). No host synchronisation."""
    if not 1 <= int(k) <= nat.TOPK_KMAX:
        raise ValueError(f"merge_topk: k must be in [1, {nat.TOPK_KMAX}], got {k}")
    if scores.dim() != 3 or scores.shape[0] < 1 or scores.shape[2] < 1:
        raise ValueError(f"merge_topk: scores must be [P, B, kin] with P, kin >= 1, got {tuple(scores.shape)}")
    for name, t, dt in (("idx", idx, torch.int64), ("groups", groups, torch.int32)):
        if t is not None and (t.shape != scores.shape or t.dtype != dt):
            raise ValueError(f"merge_topk: {name} must be {dt} of shape {tuple(scores.shape)}, got {t.dtype} {tuple(t.shape)}")
    if scores.dtype != torch.float32:
        raise ValueError(f"merge_topk: scores must be float32, got {scores.dtype}")
    _dev(scores, idx, groups)
    scores, idx = scores.contiguous(), idx.contiguous()
    groups = groups.contiguous() if groups is not None else None
    P, B, kin = scores.shape
    lib = _lib()
    nbytes = lib.cor_merge_topk_workspace_bytes(P, B, kin, k)
    if nbytes < 0:
        nat.check(int(nbytes), "cor_merge_topk_workspace_bytes")
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=scores.device) if nbytes else None
    out_s, out_i, out_g = _list_outputs(B, k, scores.device, groups is not None)
    if B:                                                     # (no queries: empty tensors have no address to pass)
        nat.check(lib.cor_merge_topk(scores.data_ptr(), idx.data_ptr(), _p(groups) or None, P, B, kin, k, out_s.data_ptr(), out_i.data_ptr(),
                                     _p(out_g) or None, _p(ws) or None, _s()), "cor_merge_topk")
    return (out_s, out_i) if groups is None else (out_s, out_i, out_g)


def rescore_topk(Q, G, cand, k, g_offset=0, return_pos=False):
    """Re-score candidate lists on the device (cor_rescore_topk), the second stage of a two-stage search: Q f32 [Bq,C], G [Ng,C]
    fp32/bf16/fp16 (the rows with global ids [g_offset, g_offset + Ng)), cand i64 [Bq,kin] global row ids -> (scores f32[Bq,k],
    idx i64[Bq,k]) ordered by (score desc, id asc), and with return_pos a third tensor pos i32[Bq,k], each entry's position in its
    input list (of a repeated id: the first occurrence). An id outside the shard (negative, another shard's, any 64-bit value) or
    seen earlier in the same list is dropped; fewer than k left: the (-inf, -1, -1) tail. Scores are the fmaf-chain scores of
    similarity_topk (16-bit galleries: the query rounded to the gallery dtype), so the list a search returned comes back bitwise.
    1 <= k <= 256, 1 <= kin <= nat.MERGE_NMAX (4096; beyond that NativeError), C <= 256 and C % 16 == 0. No host synchronisation."""
    if not 1 <= int(k) <= nat.TOPK_KMAX:
        raise ValueError(f"rescore_topk: k must be in [1, {nat.TOPK_KMAX}], got {k}")
    if Q.dim() != 2 or G.dim() != 2 or Q.shape[1] != G.shape[1]:
        raise ValueError(f"rescore_topk: Q must be [Bq, C] and G [Ng, C], got {tuple(Q.shape)} and {tuple(G.shape)}")
    if Q.dtype != torch.float32 or G.dtype not in _DT:
        raise ValueError(f"rescore_topk: Q must be float32 and G float32 / bfloat16 / float16, got {Q.dtype} and {G.dtype}")
    if cand.dim() != 2 or cand.shape[0] != Q.shape[0] or cand.shape[1] < 1 or cand.dtype != torch.int64:
        raise ValueError(f"rescore_topk: cand must be int64 [{Q.shape[0]}, kin] with kin >= 1, got {cand.dtype} {tuple(cand.shape)}")
    _dev(Q, G, cand)
    Q, G, cand = Q.contiguous(), G.contiguous(), cand.contiguous()
    (Bq, C), Ng, kin = Q.shape, G.shape[0], cand.shape[1]
    lib = _lib()
    nbytes = lib.cor_rescore_workspace_bytes(Bq, kin, k)
    if nbytes < 0:
        nat.check(int(nbytes), "cor_rescore_workspace_bytes")
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=Q.device) if nbytes else None
    out_s, out_i, out_p = _list_outputs(Bq, k, Q.device, return_pos, missing=Ng == 0)
    if Bq and Ng:                                             # (no queries / no rows: empty tensors have no address to pass)
        nat.check(lib.cor_rescore_topk(Q.data_ptr(), G.data_ptr(), _dt(G), Bq, Ng, C, int(g_offset), cand.data_ptr(), kin, k, out_s.data_ptr(),
                                       out_i.data_ptr(), _p(out_p) or None, _p(ws) or None, _s()), "cor_rescore_topk")
    return (out_s, out_i, out_p) if return_pos else (out_s, out_i)


def rescore_topk_i8(Q, Gq, gscale, cand, k, g_offset=0, return_pos=False):
    """rescore_topk over an int8 shard (cor_rescore_topk_i8): Q f32 [Bq,C]; Gq int8 [Ng,C] and gscale f32 [Ng] as quantize_rows_i8 returns
    them (the rows with global ids [g_offset, g_offset + Ng)); cand i64 [Bq,kin] global row ids -> (scores f32[Bq,k], idx i64[Bq,k]) ordered
    by (score desc, id asc), and with return_pos a third tensor pos i32[Bq,k]. The PRESENT / MISSING rule, the first occurrence per id and
    the (-inf, -1, -1) tail are rescore_topk's; the score is similarity_topk_i8's (the query is quantised inside the call, score =
    ((float)(int32 dot) * qscale) * gscale), so the list an int8 search returned comes back bitwise (one exception: a list holding both
    +0.0 and -0.0 scores, where this call lets the id decide; include/cor_amd.h). Bit-identical to tests/i8_list_refs.py.
    1 <= k <= 256, 1 <= kin <= nat.MERGE_NMAX (4096; beyond that NativeError), C <= 256 and C % 16 == 0. No host synchronisation."""
    who = "rescore_topk_i8"
    if not 1 <= int(k) <= nat.TOPK_KMAX:
        raise ValueError(f"{who}: k must be in [1, {nat.TOPK_KMAX}], got {k}")
    if Q.dim() != 2 or Gq.dim() != 2 or Q.shape[1] != Gq.shape[1]:
        raise ValueError(f"{who}: Q must be [Bq, C] and Gq [Ng, C], got {tuple(Q.shape)} and {tuple(Gq.shape)}")
    if Q.dtype != torch.float32:
        raise ValueError(f"{who}: Q must be float32, got {Q.dtype}")
    if Q.shape[1] < 16 or Q.shape[1] > 256 or Q.shape[1] % 16:
        raise ValueError(f"{who}: the width must be a multiple of 16 up to 256, got {Q.shape[1]}")
    if cand.dim() != 2 or cand.shape[0] != Q.shape[0] or cand.shape[1] < 1 or cand.dtype != torch.int64:
        raise ValueError(f"{who}: cand must be int64 [{Q.shape[0]}, kin] with kin >= 1, got {cand.dtype} {tuple(cand.shape)}")
    Q, Gq = Q.contiguous(), Gq.contiguous()
    if Q.data_ptr() % 16:                                     # a view into a larger tensor: the kernel loads 16 B at a time
        Q = Q.clone()
    if Gq.data_ptr() % 16:
        Gq = Gq.clone()
    Bq, Ng, C, gscale = _i8_front(who, Q, Gq, gscale, k, 0)
    _dev(Q, cand)
    cand, kin = cand.contiguous(), cand.shape[1]
    lib = _lib()
    nbytes = lib.cor_rescore_i8_workspace_bytes(Bq, kin, k)
    if nbytes < 0:
        nat.check(int(nbytes), "cor_rescore_i8_workspace_bytes")
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=Q.device) if nbytes else None
    out_s, out_i, out_p = _list_outputs(Bq, k, Q.device, return_pos, missing=Ng == 0)
    if Bq and Ng:                                             # (no queries / no rows: empty tensors have no address to pass)
        nat.check(lib.cor_rescore_topk_i8(Q.data_ptr(), Gq.data_ptr(), gscale.data_ptr(), Bq, Ng, C, int(g_offset), cand.data_ptr(), kin, k,
                                          out_s.data_ptr(), out_i.data_ptr(), _p(out_p) or None, _p(ws) or None, _s()), "cor_rescore_topk_i8")
    return (out_s, out_i, out_p) if return_pos else (out_s, out_i)


def expand_queries(Q, segments, scores, idx, m, alpha=3, query_weight=1.0, normalize=True, out_dtype=torch.float32, out=None):
    """Query expansion on the device (cor_expand_queries; AQE / alpha-QE, and with query_weight = 0 over gallery rows: DBA).
    Q f32 [Bq,C] (None is allowed when query_weight == 0), segments a list of (rows, offset): rows [n,C] fp32 / bf16 / fp16 holding the
    global ids [offset, offset + n), or of (rows_i8, scales, offset): int8 rows with their f32 [n] row scales as quantize_rows_i8 returns
    them, whose value is float(q) * scale, one rounded multiply (with such a segment the call is cor_expand_queries_sq, without one it
    is cor_expand_queries exactly as before); at most nat.EXPAND_SEGMAX (16) of them, pairwise disjoint, dtypes free to differ; scores f32
    [Bq,kin] and idx i64 [Bq,kin] as a search, the merge or the re-scoring return them -> [Bq,C] in out_dtype:
    v = query_weight * Q; for j < m in list order, if idx[b,j] lies in a segment: v += max(scores[b,j], +0)^alpha * row; then
    v / max(|v|, 1e-12) if normalize. Every step is one separately rounded fp32 operation in a fixed order (include/cor_amd.h has the
    definition to the bit), so the result does not depend on how the rows are cut into segments. An id of no segment (-1, another
    shard's, any 64-bit value) contributes nothing and its score is not read. 1 <= m <= min(kin, 256), 0 <= alpha <= 8, C <= 256 and
    C % 16 == 0. out: an optional contiguous [Bq,C] tensor of out_dtype to write into. No host synchronisation; capturable in a graph."""
    segments = _row_segments("expand_queries", segments, nat.EXPAND_SEGMAX)
    Bq, kin = _list_front("expand_queries", scores, idx)
    if not 1 <= int(m) <= min(kin, nat.TOPK_KMAX):
        raise ValueError(f"expand_queries: m must be in [1, min(kin, {nat.TOPK_KMAX})] (kin = {kin}), got {m}")
    if int(alpha) != alpha or not 0 <= int(alpha) <= 8:
        raise ValueError(f"expand_queries: alpha must be an integer in [0, 8], got {alpha}")
    query_weight = float(query_weight)
    if Q is None and query_weight != 0.0:
        raise ValueError("expand_queries: Q may only be None with query_weight == 0")
    if Q is None and not segments:
        raise ValueError("expand_queries: neither queries nor segments: the width is unknown")
    C = Q.shape[-1] if Q is not None else segments[0][0].shape[-1]
    if Q is not None and (Q.dim() != 2 or Q.shape[0] != Bq or Q.dtype != torch.float32):
        raise ValueError(f"expand_queries: Q must be float32 [{Bq}, C], got {Q.dtype} {tuple(Q.shape)}")
    if C < 16 or C > 256 or C % 16 != 0:
        raise ValueError(f"expand_queries: the width must be a multiple of 16 up to 256, got {C}")
    if out_dtype not in _DT:
        raise ValueError(f"expand_queries: out_dtype must be float32 / bfloat16 / float16, got {out_dtype}")
    _row_segment_tensors("expand_queries", segments, C)
    _disjoint_spans("expand_queries", segments)
    if out is not None and (out.shape != (Bq, C) or out.dtype != out_dtype or not out.is_contiguous()):
        raise ValueError(f"expand_queries: out must be a contiguous {out_dtype} [{Bq}, {C}] tensor")
    dev = _dev(Q, scores, idx, out, *[t for seg in segments for t in seg[:-1]])
    Q = Q.contiguous() if Q is not None else None
    scores, idx = scores.contiguous(), idx.contiguous()
    rows = [seg[0].contiguous() for seg in segments]
    if out is None:
        out = torch.empty((Bq, C), dtype=out_dtype, device=dev)
    n = len(segments)
    if any(len(seg) == 3 for seg in segments):                # an int8 segment: the table with row scales
        scales = [seg[1].contiguous() if len(seg) == 3 else None for seg in segments]
        seg_rows, seg_off, seg_n = _seg_arrays([seg[-1] for seg in segments], rows)
        seg_sc = (nat.C.c_void_p * n)(*[_p(t) or None for t in scales])
        seg_dt = (nat.C.c_int * n)(*[nat.I8 if len(seg) == 3 else _dt(r) for seg, r in zip(segments, rows)])
        if Bq:
            nat.check(_lib().cor_expand_queries_sq(_p(Q) or None, query_weight, seg_rows, seg_sc, seg_off, seg_n, seg_dt, n, scores.data_ptr(),
                                                   idx.data_ptr(), Bq, kin, int(m), C, int(alpha), int(bool(normalize)), out.data_ptr(),
                                                   _DT[out_dtype], _s()), "cor_expand_queries_sq")
        return out
    seg_rows, seg_off, seg_n = _seg_arrays([seg[-1] for seg in segments], rows)
    seg_dt = (nat.C.c_int * max(n, 1))(*[_dt(r) for r in rows])
    if Bq:                                                    # (no queries: empty tensors have no address to pass)
        nat.check(_lib().cor_expand_queries(_p(Q) or None, query_weight, seg_rows, seg_off, seg_n, seg_dt, n, scores.data_ptr(), idx.data_ptr(),
                                            Bq, kin, int(m), C, int(alpha), int(bool(normalize)), out.data_ptr(), _DT[out_dtype], _s()),
                  "cor_expand_queries")
    return out


def _graph_spans(who, segments):
    """Shared check of a graph's segment list [(…, offset)] whose first tensor has one row per gallery row: count and disjoint ranges."""
    if len(segments) > nat.RERANK_SEGMAX:
        raise ValueError(f"{who}: {len(segments)} segments, one call reads at most {nat.RERANK_SEGMAX}")
    _disjoint_spans(who, segments)


def knn_reciprocal(segments, seg, out=None):
    """Reciprocal pruning of one segment of a neighbour graph on the device (cor_knn_reciprocal). segments: a list of (nbr, offset), nbr
    i64 [n, k1] the global ids of the k1 nearest rows of each of the rows [offset, offset + n), as a search returns them (-1 = none); at
    most nat.RERANK_SEGMAX (16) segments, pairwise disjoint, one width k1 <= 256. -> i64 [n, k1] for segment number `seg`: the id h where
    h lies in some segment and h's own list names the row, else -1. Written to a new tensor (or `out`, which must not be an input): never
    in place. Ids are range-tested before they index anything. No host synchronisation."""
    segments = [(t, int(o)) for t, o in segments]
    if not segments or not 0 <= int(seg) < len(segments):
        raise ValueError(f"knn_reciprocal: segment number {seg} of {len(segments)} segments")
    k1 = segments[0][0].shape[-1]
    for t, _ in segments:
        if t.dim() != 2 or t.dtype != torch.int64 or t.shape[1] != k1 or t.shape[0] >= 2 ** 31:
            raise ValueError(f"knn_reciprocal: a segment's lists must be int64 [n < 2^31, {k1}], got {t.dtype} {tuple(t.shape)}")
    if not 1 <= k1 <= nat.TOPK_KMAX:
        raise ValueError(f"knn_reciprocal: the lists' width must be in [1, {nat.TOPK_KMAX}], got {k1}")
    _graph_spans("knn_reciprocal", segments)
    mine = segments[int(seg)][0]
    if out is not None and (out.shape != mine.shape or out.dtype != torch.int64 or not out.is_contiguous()
                            or any(out.data_ptr() == t.data_ptr() for t, _ in segments if t.numel())):
        raise ValueError(f"knn_reciprocal: out must be a contiguous int64 {tuple(mine.shape)} tensor that is none of the inputs")
    dev = _dev(out, *[t for t, _ in segments])
    lists = [t.contiguous() for t, _ in segments]
    if out is None:
        out = torch.empty(mine.shape, dtype=torch.int64, device=dev)
    seg_nbr, seg_off, seg_n = _seg_arrays([o for _, o in segments], lists)
    if mine.shape[0]:                                         # (no rows: empty tensors have no address to pass)
        nat.check(_lib().cor_knn_reciprocal(seg_nbr, seg_off, seg_n, len(segments), k1, int(seg), out.data_ptr(), _s()), "cor_knn_reciprocal")
    return out


def rerank_reciprocal(scores, idx, segments, k1, lam, k, return_pos=False):
    """k-reciprocal re-ranking of lists on the device, set form (cor_rerank_reciprocal). scores f32 [Bq,kin] and idx i64 [Bq,kin] as a
    search, the merge or the re-scoring return them; segments: a list of (rnbr, kth, offset), the graph of the rows [offset, offset + n):
    rnbr i64 [n,kg] the reciprocal neighbour lists (knn_reciprocal), kth f32 [n] the score of each row's k1-th neighbour; at most
    nat.RERANK_SEGMAX (16), pairwise disjoint, one width kg <= 256. -> (scores f32[Bq,k], idx i64[Bq,k]) and with return_pos pos i32[Bq,k]:
    A = the ids of the first k1 entries with score >= kth[id]; every entry whose id lies in a segment gets
    f = lam * score + (1 - lam) * |A n B| / |A u B|, B its row's non-negative rnbr ids, and the entries are ranked by (f desc, id asc);
    an id of no segment (-1, another shard's, any 64-bit value) is dropped and its score is not read; fewer than k left: the
    (-inf, -1, -1) tail. include/cor_amd.h has the definition to the bit. 1 <= k1 <= min(kin, 256), 1 <= k <= 256, kin <= nat.MERGE_NMAX
    (4096; beyond that NativeError), lam finite. No host synchronisation; capturable in a graph."""
    segments = [(r, t, int(o)) for r, t, o in segments]
    Bq, kin = _list_front("rerank_reciprocal", scores, idx)
    if not 1 <= int(k) <= nat.TOPK_KMAX:
        raise ValueError(f"rerank_reciprocal: k must be in [1, {nat.TOPK_KMAX}], got {k}")
    if not 1 <= int(k1) <= min(kin, nat.TOPK_KMAX):
        raise ValueError(f"rerank_reciprocal: k1 must be in [1, min(kin, {nat.TOPK_KMAX})] (kin = {kin}), got {k1}")
    lam = float(lam)
    if lam != lam or lam in (float("inf"), float("-inf")):
        raise ValueError(f"rerank_reciprocal: lam must be finite, got {lam}")
    kg = segments[0][0].shape[-1] if segments else 1
    for r, t, _ in segments:
        if r.dim() != 2 or r.dtype != torch.int64 or r.shape[1] != kg or r.shape[0] >= 2 ** 31:
            raise ValueError(f"rerank_reciprocal: a segment's lists must be int64 [n < 2^31, {kg}], got {r.dtype} {tuple(r.shape)}")
        if t.dim() != 1 or t.dtype != torch.float32 or t.shape[0] != r.shape[0]:
            raise ValueError(f"rerank_reciprocal: a segment's kth must be float32 [{r.shape[0]}], got {t.dtype} {tuple(t.shape)}")
    if not 1 <= kg <= nat.TOPK_KMAX:
        raise ValueError(f"rerank_reciprocal: the graph's width must be in [1, {nat.TOPK_KMAX}], got {kg}")
    _graph_spans("rerank_reciprocal", segments)
    dev = _dev(scores, idx, *[x for r, t, _ in segments for x in (r, t)])
    scores, idx = scores.contiguous(), idx.contiguous()
    lists, kths = [r.contiguous() for r, _, _ in segments], [t.contiguous() for _, t, _ in segments]
    out_s, out_i, out_p = _list_outputs(Bq, k, dev, return_pos)
    seg_rnbr, seg_kth, seg_off, seg_n = _seg_arrays([o for _, _, o in segments], lists, kths)
    if Bq:                                                    # (no queries: empty tensors have no address to pass)
        nat.check(_lib().cor_rerank_reciprocal(scores.data_ptr(), idx.data_ptr(), seg_rnbr, seg_kth, seg_off, seg_n, len(segments), Bq, kin, kg, int(k1), lam,
                                               int(k), out_s.data_ptr(), out_i.data_ptr(), _p(out_p) or None, _s()), "cor_rerank_reciprocal")
    return (out_s, out_i, out_p) if return_pos else (out_s, out_i)


def _row_segments(who, segments, segmax):
    """The gallery-row segments of a call that reads rows through a segment table, offsets as ints: each (rows, offset) or (rows_i8, scales, offset), at most segmax."""
    segments = [tuple(seg[:-1]) + (int(seg[-1]),) for seg in segments]
    if any(len(seg) not in (2, 3) for seg in segments):
        raise ValueError(f"{who}: a segment is (rows, offset) or (rows_i8, scales, offset)")
    if len(segments) > segmax:
        raise ValueError(f"{who}: {len(segments)} segments, one call reads at most {segmax}")
    return segments


def _row_segment_tensors(who, segments, C):
    """The checks of each such segment's tensors: rows [n < 2^31, C] of a storage dtype, or int8 rows with float32 [n] scales."""
    for seg in segments:
        r = seg[0]
        if len(seg) == 3:
            if r.dim() != 2 or r.shape[1] != C or r.dtype != torch.int8 or r.shape[0] >= 2 ** 31:
                raise ValueError(f"{who}: a segment with scales must be int8 [n < 2^31, {C}], got {r.dtype} {tuple(r.shape)}")
            if seg[1].dtype != torch.float32 or seg[1].dim() != 1 or seg[1].shape[0] != r.shape[0]:
                raise ValueError(f"{who}: scales must be float32 [{r.shape[0]}], got {seg[1].dtype} {tuple(seg[1].shape)}")
        elif r.dim() != 2 or r.shape[1] != C or r.dtype not in _DT or r.shape[0] >= 2 ** 31:
            raise ValueError(f"{who}: a segment must be float32 / bfloat16 / float16 [n < 2^31, {C}], got {r.dtype} {tuple(r.shape)}")


def _row_segments_width(who, segments):
    """The checks of such segments' tensors (one width C, a multiple of 16 up to 256; dtypes; scales; disjoint id ranges) -> C."""
    C = segments[0][0].shape[-1] if segments and segments[0][0].dim() == 2 else 16    # (no segment: every entry is missing, any width will do)
    if C < 16 or C > 256 or C % 16 != 0:
        raise ValueError(f"{who}: the width must be a multiple of 16 up to 256, got {C}")
    _row_segment_tensors(who, segments, C)
    _disjoint_spans(who, segments)
    return C


def _row_table(segments):
    """Checked segments on the device -> ((seg_rows, seg_scale, seg_offset, seg_n, seg_dtype) as ctypes arrays, nseg, the tensors they point to)."""
    rows = [seg[0].contiguous() for seg in segments]
    rows = [r.clone() if r.data_ptr() % 16 else r for r in rows]   # a view into a larger tensor: the kernel loads 16 B at a time
    scales = [seg[1].contiguous() if len(seg) == 3 else None for seg in segments]
    n = len(segments)
    seg_rows, seg_off, seg_n = _seg_arrays([seg[-1] for seg in segments], rows)
    seg_sc = (nat.C.c_void_p * max(n, 1))(*[_p(t) or None for t in scales])
    seg_dt = (nat.C.c_int * max(n, 1))(*[nat.I8 if len(seg) == 3 else _dt(r) for seg, r in zip(segments, rows)])
    return (seg_rows, seg_sc, seg_off, seg_n, seg_dt), n, (rows, scales)


def diversify_mmr(segments, scores, idx, k, lam=0.5, max_sim=None, return_pos=False, return_value=False):
    """Diversified lists on the device (cor_diversify_mmr): greedy maximal marginal relevance with optional near-duplicate suppression.
    segments as expand_queries takes them: a list of (rows, offset), rows [n,C] fp32 / bf16 / fp16 holding the global ids
    [offset, offset + n), or of (rows_i8, scales, offset), int8 rows with their f32 [n] row scales whose value is float(q) * scale; at most
    nat.DIVERSIFY_SEGMAX (16), pairwise disjoint, dtypes free to differ. scores f32 [Bq,kin] and idx i64 [Bq,kin] as a search, the merge
    or the re-scoring return them -> (scores f32[Bq,k], idx i64[Bq,k][, pos i32[Bq,k]][, value f32[Bq,k]]). Per query, k times: among
    the entries still alive the one with the greatest f = lam * score - (1 - lam) * (its largest similarity to an entry already chosen,
    at least 0) goes out, by (f desc, id asc, position asc), with its INPUT score (value: f itself; pos: its position in the input list);
    then every alive entry whose similarity to it is >= max_sim leaves for good (max_sim None: no suppression). The similarity is the
    fmaf chain of the searches over the rows' fp32 values, so neither the segmentation nor the storage dtype of equal values changes
    a bit; include/cor_amd.h has the definition to the bit. An id of no segment (-1, another shard's, any 64-bit value) is dropped and its
    score is not read; a repeated id is an entry of its own. Fewer than k chosen: the (-inf, -1, -1, -inf) tail. lam = 1 without max_sim
    returns the present entries by (score desc, id asc); lam = 1 with max_sim is plain near-duplicate suppression. 0 <= lam <= 1,
    1 <= k <= 256, kin <= nat.MERGE_NMAX (4096; beyond that NativeError), C <= 256 and C % 16 == 0. No host synchronisation; capturable
    in a graph."""
    who = "diversify_mmr"
    segments = _row_segments(who, segments, nat.DIVERSIFY_SEGMAX)
    Bq, kin = _list_front(who, scores, idx)
    if not 1 <= int(k) <= nat.TOPK_KMAX:
        raise ValueError(f"{who}: k must be in [1, {nat.TOPK_KMAX}], got {k}")
    lam = float(lam)
    if not 0.0 <= lam <= 1.0:
        raise ValueError(f"{who}: lam must be in [0, 1], got {lam}")
    max_sim = float("inf") if max_sim is None else float(max_sim)
    if max_sim != max_sim:
        raise ValueError(f"{who}: max_sim must not be NaN")
    C = _row_segments_width(who, segments)
    dev = _dev(scores, idx, *[t for seg in segments for t in seg[:-1]])
    scores, idx = scores.contiguous(), idx.contiguous()
    table, n, _keep = _row_table(segments)
    out_s, out_i, out_p = _list_outputs(Bq, int(k), dev, return_pos)
    out_v = torch.empty((Bq, int(k)), dtype=torch.float32, device=dev) if return_value else None
    if Bq:                                                    # (no queries: empty tensors have no address to pass)
        nat.check(_lib().cor_diversify_mmr(*table, n, scores.data_ptr(), idx.data_ptr(), Bq, kin, C, lam, max_sim,
                                           int(k), out_s.data_ptr(), out_i.data_ptr(), _p(out_p) or None, _p(out_v) or None, _s()),
                  "cor_diversify_mmr")
    return (out_s, out_i) + ((out_p,) if return_pos else ()) + ((out_v,) if return_value else ())


def rerank_diffusion(segments, scores, idx, k, kd=8, kq=None, gamma=3, alpha=0.9, iters=20, return_pos=False):
    """Diffusion re-ranking of lists on the device (cor_rerank_diffusion): manifold ranking on the mutual kd-nearest-neighbour graph of
    each query's candidates. segments as diversify_mmr takes them: a list of (rows, offset), rows [n,C] fp32 / bf16 / fp16 holding the
    global ids [offset, offset + n), or of (rows_i8, scales, offset); at most nat.DIFFUSE_SEGMAX (16), pairwise disjoint, dtypes free to
    differ. scores f32 [Bq,kin] and idx i64 [Bq,kin] as a search, the merge or the re-scoring return them, kin <= nat.DIFFUSE_NMAX (256;
    beyond that NativeError) -> (scores f32[Bq,k], idx i64[Bq,k][, pos i32[Bq,k]]). Per query: the affinity of two present entries is
    their chain similarity (that of diversify_mmr), clipped at 0, to the power gamma; every entry keeps its kd best neighbours and an
    edge stays if both ends keep each other; the edges are scaled by 1 / sqrt(degree) of both ends; y holds score ** gamma for the kq
    first present entries (kq None: all) and 0 for the rest; f starts as y and `iters` times becomes alpha * S f + (1 - alpha) * y; the
    present entries go out ranked by (f desc, id asc, position asc) with f as their score. include/cor_amd.h has the definition to the
    bit. An id of no segment (-1, another shard's, any 64-bit value) is dropped and its score is not read; a repeated id is an entry of
    its own. Fewer than k present: the (-inf, -1, -1) tail. alpha = 0 returns y. 1 <= k <= 256, 1 <= kd <= nat.DIFFUSE_KDMAX (32),
    kq >= 1, 1 <= gamma <= 4, 0 <= alpha < 1, 1 <= iters <= 64, C <= 256 and C % 16 == 0. No host synchronisation; capturable in a graph."""
    who = "rerank_diffusion"
    segments = _row_segments(who, segments, nat.DIFFUSE_SEGMAX)
    Bq, kin = _list_front(who, scores, idx)
    if not 1 <= int(k) <= nat.TOPK_KMAX:
        raise ValueError(f"{who}: k must be in [1, {nat.TOPK_KMAX}], got {k}")
    kq = nat.DIFFUSE_NMAX if kq is None else kq
    if not 1 <= int(kd) <= nat.DIFFUSE_KDMAX or int(kq) < 1:
        raise ValueError(f"{who}: kd must be in [1, {nat.DIFFUSE_KDMAX}] and kq at least 1, got kd={kd}, kq={kq}")
    if not 1 <= int(gamma) <= 4 or not 1 <= int(iters) <= 64:
        raise ValueError(f"{who}: gamma must be in [1, 4] and iters in [1, 64], got gamma={gamma}, iters={iters}")
    alpha = float(alpha)
    if not 0.0 <= alpha < 1.0:
        raise ValueError(f"{who}: alpha must be in [0, 1), got {alpha}")
    C = _row_segments_width(who, segments)
    dev = _dev(scores, idx, *[t for seg in segments for t in seg[:-1]])
    scores, idx = scores.contiguous(), idx.contiguous()
    table, n, _keep = _row_table(segments)
    out_s, out_i, out_p = _list_outputs(Bq, int(k), dev, return_pos)
    if Bq:                                                    # (no queries: empty tensors have no address to pass)
        nat.check(_lib().cor_rerank_diffusion(*table, n, scores.data_ptr(), idx.data_ptr(), Bq, kin, C, int(kd), min(int(kq), 2 ** 31 - 1),
                                              int(gamma), alpha, int(iters), int(k), out_s.data_ptr(), out_i.data_ptr(), _p(out_p) or None,
                                              _s()), "cor_rerank_diffusion")
    return (out_s, out_i, out_p) if return_pos else (out_s, out_i)


def _kmeans_front(who, segments, K):
    """The checks kmeans_seed and kmeans_update share -> (segments with int offsets, C, n_total); nothing touches the device."""
    segments = _row_segments(who, segments, nat.CLUSTER_SEGMAX)
    if not 1 <= int(K) <= nat.KMEANS_KMAX:
        raise ValueError(f"{who}: K must be in [1, {nat.KMEANS_KMAX}], got {K}")
    C = _row_segments_width(who, segments)
    n = sum(seg[0].shape[0] for seg in segments)
    if n >= 2 ** 31:
        raise ValueError(f"{who}: {n} rows, one call takes fewer than 2^31")
    return segments, C, n


def _kmeans_workspace(n, K, C, dev):
    nbytes = _lib().cor_kmeans_workspace_bytes(n, int(K), C)
    if nbytes < 0:
        nat.check(int(nbytes), "cor_kmeans_workspace_bytes")
    return torch.empty((nbytes,), dtype=torch.uint8, device=dev)


def kmeans_seed(segments, K, first_id=None):
    """Farthest-point ("max-min") seeding on the device (cor_kmeans_seed): K rows that are far from each other, deterministic, no random
    numbers. segments as diversify_mmr takes them: a list of (rows, offset), rows [n,C] fp32 / bf16 / fp16 holding the global ids
    [offset, offset + n), or of (rows_i8, scales, offset); at most nat.CLUSTER_SEGMAX (16), pairwise disjoint, dtypes free to differ.
    -> (ids i64[K], centroids f32[K,C]): the chosen rows' global ids in the order they were chosen and their values. The first is
    first_id (None: the smallest id present); then K - 1 times the row whose largest chain similarity to the rows chosen so far is
    smallest, ties to the smallest id. The similarity is the fmaf chain of the searches over the rows' fp32 values, so neither the
    segmentation nor the storage dtype of equal values changes a bit; include/cor_amd.h has the definition to the bit. 1 <= K <=
    min(nat.KMEANS_KMAX, the number of rows), C <= 256 and C % 16 == 0. 2K launches, no host synchronisation; capturable in a graph."""
    who = "kmeans_seed"
    segments, C, n = _kmeans_front(who, segments, K)
    if int(K) > n:
        raise ValueError(f"{who}: K = {K} but the segments hold {n} rows")
    live = [seg for seg in segments if seg[0].shape[0]]
    first_id = min(seg[-1] for seg in live) if first_id is None else int(first_id)
    if not any(seg[-1] <= first_id < seg[-1] + seg[0].shape[0] for seg in live):
        raise ValueError(f"{who}: no segment holds first_id = {first_id}")
    dev = _dev(*[t for seg in segments for t in seg[:-1]])
    table, nseg, _keep = _row_table(segments)
    ids = torch.empty((int(K),), dtype=torch.int64, device=dev)
    cent = torch.empty((int(K), C), dtype=torch.float32, device=dev)
    ws = _kmeans_workspace(n, K, C, dev)
    nat.check(_lib().cor_kmeans_seed(*table, nseg, C, int(K), first_id, ids.data_ptr(), cent.data_ptr(), ws.data_ptr(), _s()), "cor_kmeans_seed")
    return ids, cent


def kmeans_update(segments, assigns, K, scores=None, prev=None, out=None):
    """The centre step of spherical k-means on the device (cor_kmeans_update). segments as kmeans_seed takes them; assigns: one int32 [n]
    tensor per segment, the cluster of each row (a value outside [0, K), e.g. -1: the row belongs to no cluster); scores: None, or one
    f32 [n] tensor per segment, each row's score to its centre; prev: None or f32 [K,C], the centres an empty cluster keeps (None: a zero
    row); out: None or f32 [K,C] to write into (not prev). -> (centroids f32[K,C], counts i32[K], score_sums f32[K] or None). A centre is
    the sum of its members' values, taken in ascending global id in chunks of 256 members whose partial sums are then added up, divided by
    its Euclidean norm (the norm tree of expand_queries); score_sums is the same two-level sum over the members' scores. Every step is
    one rounded fp32 operation in an order include/cor_amd.h fixes, so the result does not depend on the segmentation, on the storage
    dtype of equal values or on how skewed the clusters are. 1 <= K <= nat.KMEANS_KMAX (16384), C <= 256 and C % 16 == 0. Six launches,
    no host synchronisation; capturable in a graph."""
    who = "kmeans_update"
    segments, C, n = _kmeans_front(who, segments, K)
    K = int(K)

    def per_segment(ts, dtype, name):
        ts = list(ts)
        if len(ts) != len(segments):
            raise ValueError(f"{who}: {len(ts)} {name} tensors for {len(segments)} segments")
        for t, seg in zip(ts, segments):
            if t.dtype != dtype or t.dim() != 1 or t.shape[0] != seg[0].shape[0]:
                raise ValueError(f"{who}: {name} must be {dtype} [{seg[0].shape[0]}] per segment, got {t.dtype} {tuple(t.shape)}")
        return ts

    assigns = per_segment(assigns, torch.int32, "assigns")
    scores = None if scores is None else per_segment(scores, torch.float32, "scores")
    for t, name in ((prev, "prev"), (out, "out")):
        if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != (K, C) or not t.is_contiguous()):
            raise ValueError(f"{who}: {name} must be contiguous float32 [{K}, {C}], got {t.dtype} {tuple(t.shape)}")
    if out is not None and prev is not None and out.data_ptr() == prev.data_ptr():
        raise ValueError(f"{who}: out must not be prev")
    dev = _dev(prev, out, *assigns, *(scores or ()), *[t for seg in segments for t in seg[:-1]])
    if dev is None:
        raise ValueError(f"{who}: no tensor names a device (no segments and neither prev nor out)")
    table, nseg, _keep = _row_table(segments)
    assigns = [a.contiguous() for a in assigns]
    scores = None if scores is None else [s.contiguous() for s in scores]
    m = max(nseg, 1)
    seg_a = (nat.C.c_void_p * m)(*[a.data_ptr() or None for a in assigns])
    seg_s = None if scores is None else (nat.C.c_void_p * m)(*[s.data_ptr() or None for s in scores])
    cent = torch.empty((K, C), dtype=torch.float32, device=dev) if out is None else out
    counts = torch.empty((K,), dtype=torch.int32, device=dev)
    sums = None if scores is None else torch.empty((K,), dtype=torch.float32, device=dev)
    ws = _kmeans_workspace(n, K, C, dev)
    nat.check(_lib().cor_kmeans_update(*table, nseg, seg_a, seg_s, C, K, _p(prev) or None, cent.data_ptr(), counts.data_ptr(), _p(sums) or None,
                                       ws.data_ptr(), _s()), "cor_kmeans_update")
    return cent, counts, sums


def ivf_build(segments, assigns, K):
    """Cell-contiguous storage of a clustered gallery on the device (cor_ivf_build). segments as kmeans_update takes them, but of ONE
    dtype (float32 / bfloat16 / float16 rows, or int8 rows with their scales): rows are copied bit for bit, never converted; assigns: one
    int32 [n] tensor per segment, the cell of each row (a value outside [0, K): the row is not indexed).
    -> (rows [n_total,C] in the segments' dtype, scales f32[n_total] or None, ids i64[n_total], cell_start i32[K+1]). Cell c owns the
    slots [cell_start[c], cell_start[c+1]), its rows in ascending global id; cell_start[K] is the number of indexed rows and the slots
    behind it are left unwritten. The result does not depend on the segmentation. 1 <= K <= nat.KMEANS_KMAX, C <= 256 and C % 16 == 0.
    Five launches, no host synchronisation; capturable in a graph."""
    who = "ivf_build"
    segments, C, n = _kmeans_front(who, segments, K)
    K = int(K)
    if not segments:
        raise ValueError(f"{who}: no segment names a dtype and a device")
    i8 = len(segments[0]) == 3
    dtype = segments[0][0].dtype
    if any((len(seg) == 3) != i8 or seg[0].dtype != dtype for seg in segments):
        raise ValueError(f"{who}: the segments must share one dtype (rows are copied, never converted)")
    assigns = list(assigns)
    if len(assigns) != len(segments):
        raise ValueError(f"{who}: {len(assigns)} assigns tensors for {len(segments)} segments")
    for t, seg in zip(assigns, segments):
        if t.dtype != torch.int32 or t.dim() != 1 or t.shape[0] != seg[0].shape[0]:
            raise ValueError(f"{who}: assigns must be {torch.int32} [{seg[0].shape[0]}] per segment, got {t.dtype} {tuple(t.shape)}")
    dev = _dev(*assigns, *[t for seg in segments for t in seg[:-1]])
    table, nseg, _keep = _row_table(segments)
    assigns = [a.contiguous() for a in assigns]
    seg_a = (nat.C.c_void_p * max(nseg, 1))(*[a.data_ptr() or None for a in assigns])
    rows = torch.empty((n, C), dtype=dtype, device=dev)
    scales = torch.empty((n,), dtype=torch.float32, device=dev) if i8 else None
    ids = torch.empty((n,), dtype=torch.int64, device=dev)
    cell_start = torch.empty((K + 1,), dtype=torch.int32, device=dev)
    nbytes = _lib().cor_ivf_build_workspace_bytes(n, K, C)
    if nbytes < 0:
        nat.check(int(nbytes), "cor_ivf_build_workspace_bytes")
    ws = torch.empty((max(int(nbytes), 256),), dtype=torch.uint8, device=dev)
    # an empty tensor has no address: the library wants non-null outputs even when it writes nothing into them
    hold = torch.empty((16,), dtype=torch.uint8, device=dev) if n == 0 else None
    nat.check(_lib().cor_ivf_build(*table, nseg, seg_a, C, K, nat.I8 if i8 else _DT[dtype], _p(rows) or _p(hold), _p(scales) or _p(hold),
                                   _p(ids) or _p(hold), cell_start.data_ptr(), ws.data_ptr(), _s()), "cor_ivf_build")
    return rows, scales, ids, cell_start


def ivf_search(Q, rows, scales, ids, cell_start, probes, k, max_cell, split=0, return_scanned=False):
    """Exact top-k over the rows of the probed cells (cor_ivf_search). Q f32 [Bq,C]; rows, scales, ids, cell_start: what ivf_build
    returned (scales None for float rows); probes i64 [Bq,nprobe], what a search over the centres returns: every value outside [0, K)
    and every repeat is ignored; 1 <= nprobe <= nat.IVF_NPROBE_MAX, 1 <= k <= 256. max_cell: the largest cell's size (a hint >= 1) and
    split (0: automatic, else that many partial lists per query, split * k <= nat.MERGE_NMAX) only deal the work out: the result's bits
    do not depend on them. -> (scores f32[Bq,k], idx i64[Bq,k][, scanned i32[Bq]]): the lists of the exact search of that dtype over
    the candidate rows alone, idx being global ids, then the (-inf, -1) tail; scanned: the number of candidate rows of each query.
    Two launches, no host synchronisation; capturable in a graph."""
    who = "ivf_search"
    k, max_cell, split = int(k), int(max_cell), int(split)
    if Q.dim() != 2 or Q.dtype != torch.float32:
        raise ValueError(f"{who}: Q must be float32 [Bq, C], got {Q.dtype} {tuple(Q.shape)}")
    Bq, C = Q.shape
    if C < 16 or C > 256 or C % 16 != 0:
        raise ValueError(f"{who}: the width must be a multiple of 16 up to 256, got {C}")
    i8 = rows.dtype == torch.int8
    if rows.dim() != 2 or rows.shape[1] != C or (not i8 and rows.dtype not in _DT) or rows.shape[0] >= 2 ** 31:
        raise ValueError(f"{who}: rows must be float32 / bfloat16 / float16 / int8 [n < 2^31, {C}], got {rows.dtype} {tuple(rows.shape)}")
    n = rows.shape[0]
    if i8 != (scales is not None):
        raise ValueError(f"{who}: scales go with int8 rows and with int8 rows only")
    if i8 and (scales.dtype != torch.float32 or scales.dim() != 1 or scales.shape[0] != n):
        raise ValueError(f"{who}: scales must be float32 [{n}], got {scales.dtype} {tuple(scales.shape)}")
    if ids.dtype != torch.int64 or ids.dim() != 1 or ids.shape[0] != n:
        raise ValueError(f"{who}: ids must be int64 [{n}], got {ids.dtype} {tuple(ids.shape)}")
    if cell_start.dtype != torch.int32 or cell_start.dim() != 1 or not 2 <= cell_start.shape[0] <= nat.KMEANS_KMAX + 1:
        raise ValueError(f"{who}: cell_start must be int32 [K + 1] with 1 <= K <= {nat.KMEANS_KMAX}, got {cell_start.dtype} {tuple(cell_start.shape)}")
    K = cell_start.shape[0] - 1
    if probes.dtype != torch.int64 or probes.dim() != 2 or probes.shape[0] != Bq or not 1 <= probes.shape[1] <= nat.IVF_NPROBE_MAX:
        raise ValueError(f"{who}: probes must be int64 [{Bq}, 1..{nat.IVF_NPROBE_MAX}], got {probes.dtype} {tuple(probes.shape)}")
    nprobe = probes.shape[1]
    if not 1 <= k <= nat.TOPK_KMAX:
        raise ValueError(f"{who}: k must be in [1, {nat.TOPK_KMAX}], got {k}")
    if max_cell < 1:
        raise ValueError(f"{who}: max_cell must be at least 1, got {max_cell}")
    if split < 0 or split * k > nat.MERGE_NMAX:
        raise ValueError(f"{who}: split must be 0 (automatic) or give split * k <= {nat.MERGE_NMAX}, got split={split}, k={k}")
    dev = _dev(Q, rows, scales, ids, cell_start, probes)
    out_s = torch.empty((Bq, k), dtype=torch.float32, device=dev)
    out_i = torch.empty((Bq, k), dtype=torch.int64, device=dev)
    scanned = torch.empty((Bq,), dtype=torch.int32, device=dev) if return_scanned else None
    if Bq > 0:
        Q, rows, ids, cell_start, probes = Q.contiguous(), rows.contiguous(), ids.contiguous(), cell_start.contiguous(), probes.contiguous()
        scales = None if scales is None else scales.contiguous()
        Q = Q.clone() if Q.data_ptr() % 16 else Q
        nbytes = _lib().cor_ivf_search_workspace_bytes(Bq, K, C, nprobe, k, split)
        if nbytes < 0:
            nat.check(int(nbytes), "cor_ivf_search_workspace_bytes")
        ws = torch.empty((max(int(nbytes), 256),), dtype=torch.uint8, device=dev)
        hold = torch.empty((16,), dtype=torch.uint8, device=dev) if n == 0 else None   # an index without rows: every list is the tail
        nat.check(_lib().cor_ivf_search(Q.data_ptr(), _p(rows) or _p(hold), (_p(scales) or _p(hold)) if i8 else None, nat.I8 if i8 else _DT[rows.dtype],
                                        _p(ids) or _p(hold), cell_start.data_ptr(), K, C, Bq, probes.data_ptr(), nprobe, k, max_cell, split,
                                        out_s.data_ptr(), out_i.data_ptr(), _p(scanned) or None, ws.data_ptr(), _s()), "cor_ivf_search")
    return (out_s, out_i, scanned) if return_scanned else (out_s, out_i)


_FUSE_MODES ={"rrf": nat.FUSE_RRF, "sum": nat.FUSE_SUM, "max": nat.FUSE_MAX}
_FUSE_NORMS = {"none": nat.FUSE_NORM_NONE, "minmax": nat.FUSE_NORM_MINMAX}
_FUSE_MISSING = {"zero": nat.FUSE_MISSING_ZERO, "floor": nat.FUSE_MISSING_FLOOR}


def fuse_args(who, P, k, weights=None, mode="rrf", rrf_c=60.0, normalize="none", missing="zero"):
    """The checks of a fusion's host arguments (everything cor_fuse_lists refuses that does not depend on the lists), before anything touches
    the device -> (weights as P floats, mode, normalize, missing as the C constants, rrf_c)."""
    if not 1 <= int(k) <= nat.TOPK_KMAX:
        raise ValueError(f"{who}: k must be in [1, {nat.TOPK_KMAX}], got {k}")
    if not 1 <= int(P) <= nat.FUSE_PMAX:
        raise ValueError(f"{who}: {P} lists, one call fuses 1 to {nat.FUSE_PMAX}")
    if mode not in _FUSE_MODES or normalize not in _FUSE_NORMS or missing not in _FUSE_MISSING:
        raise ValueError(f"{who}: mode is one of {sorted(_FUSE_MODES)}, normalize of {sorted(_FUSE_NORMS)}, missing of {sorted(_FUSE_MISSING)}; "
                         f"got {mode!r}, {normalize!r}, {missing!r}")
    if mode == "rrf" and (normalize != "none" or missing != "zero"):
        raise ValueError(f"{who}: reciprocal-rank fusion uses ranks alone: normalize and missing must be 'none' and 'zero'")
    if mode == "max" and missing != "zero":
        raise ValueError(f"{who}: mode 'max' ignores the lists that do not hold an id: missing must be 'zero'")
    if isinstance(weights, torch.Tensor) and weights.device.type != "cpu":
        raise ValueError(f"{who}: weights are host floats (they travel in the kernel arguments), not a device tensor")
    w = [1.0] * int(P) if weights is None else [float(x) for x in weights]
    if len(w) != int(P):
        raise ValueError(f"{who}: {len(w)} weights for {P} lists")
    w = [nat.C.c_float(x).value for x in w]                   # as the kernel receives them
    if not all(math.isfinite(x) for x in w):
        raise ValueError(f"{who}: the weights must be finite as float32, got {w}")
    rrf_c = float(rrf_c)
    if mode == "rrf" and not (math.isfinite(nat.C.c_float(rrf_c).value) and rrf_c >= 0.0):
        raise ValueError(f"{who}: rrf_c must be finite and >= 0, got {rrf_c}")
    return w, _FUSE_MODES[mode], _FUSE_NORMS[normalize], _FUSE_MISSING[missing], rrf_c


def fuse_lists(scores, idx, k, weights=None, mode="rrf", rrf_c=60.0, normalize="none", missing="zero", return_count=False):
    """Fuse P ranked lists per query on the device (cor_fuse_lists): scores f32 [P,Bq,kin], idx i64 [P,Bq,kin], P rankings of the same Bq
    requests over the same global ids, stacked -> (scores f32[Bq,k], idx i64[Bq,k][, count i32[Bq,k]]): one entry per distinct id, ranked by
    (fused score desc, id asc), then the (-inf, -1, -1) tail; count is the number of lists that hold the id. mode "rrf": the sum over the
    lists that hold the id of w_p / (rrf_c + rank), rank = position + 1; "sum" (CombSUM): the sum of w_p * value; "max" (CombMAX): the
    greatest w_p * value. normalize "minmax": a list's values are (s - min) / (max - min) over its valid entries (1 where they are all
    equal) instead of the scores. missing "floor" (sum only): a list that does not hold the id contributes w_p * its least valid score (0
    under minmax) instead of nothing. weights: a host sequence of P floats (default all 1), never a device tensor. An entry with idx < 0 or
    a non-finite score is a hole; of an id repeated inside a list only the lowest position counts. include/cor_amd.h has the definition to
    the bit. 1 <= P <= nat.FUSE_PMAX (16), P * kin <= nat.MERGE_NMAX (4096), 1 <= k <= 256, else ValueError. No host synchronisation;
    capturable in a graph."""
    who = "fuse_lists"
    if not isinstance(scores, torch.Tensor) or not isinstance(idx, torch.Tensor) or scores.dim() != 3 or scores.shape[0] < 1 or scores.shape[2] < 1:
        raise ValueError(f"{who}: scores must be a tensor [P, Bq, kin] with P, kin >= 1, got {tuple(getattr(scores, 'shape', ()))}")
    if scores.dtype != torch.float32:
        raise ValueError(f"{who}: scores must be float32, got {scores.dtype}")
    if idx.shape != scores.shape or idx.dtype != torch.int64:
        raise ValueError(f"{who}: idx must be int64 of shape {tuple(scores.shape)}, got {idx.dtype} {tuple(idx.shape)}")
    P, Bq, kin = scores.shape
    w, c_mode, c_norm, c_missing, rrf_c = fuse_args(who, P, k, weights, mode, rrf_c, normalize, missing)
    if P * kin > nat.MERGE_NMAX:
        raise ValueError(f"{who}: {P} lists of {kin} are {P * kin} entries per query, one call fuses at most {nat.MERGE_NMAX}")
    dev = _dev(scores, idx)
    scores, idx = scores.contiguous(), idx.contiguous()
    out_s, out_i, out_c = _list_outputs(Bq, int(k), dev, return_count)
    if Bq:                                                    # (no queries: empty tensors have no address to pass)
        nat.check(_lib().cor_fuse_lists(scores.data_ptr(), idx.data_ptr(), P, Bq, kin, (nat.C.c_float * P)(*w), c_mode, c_norm, c_missing, rrf_c,
                                        int(k), out_s.data_ptr(), out_i.data_ptr(), _p(out_c) or None, None, _s()), "cor_fuse_lists")
    return (out_s, out_i, out_c) if return_count else (out_s, out_i)


def decoder_heads(hs, w01, b01, w2, b2):
    """The mask decoder's five output MLPs in one launch (cor_decoder_heads). hs [B*6,256] in the weights' dtype ->
    (hyper f32 [B,4,32], iou f32 [B,4])."""
    _dev(hs, w01, b01, w2, b2)
    assert hs.is_contiguous() and hs.dim() == 2 and hs.shape[1] == 256 and hs.shape[0] % 6 == 0 and hs.dtype == w01.dtype == w2.dtype
    assert tuple(w01.shape) == (5, 2, 256, 256) and tuple(b01.shape) == (5, 2, 256) and tuple(w2.shape) == (132, 256) and tuple(b2.shape) == (132,)
    assert w01.is_contiguous() and w2.is_contiguous() and b01.is_contiguous() and b2.is_contiguous() and b01.dtype == b2.dtype == torch.float32
    B = hs.shape[0] // 6
    hyper = torch.empty((B, 4, 32), dtype=torch.float32, device=hs.device)
    iou = torch.empty((B, 4), dtype=torch.float32, device=hs.device)
    nat.check(_lib().cor_decoder_heads(hs.data_ptr(), w01.data_ptr(), b01.data_ptr(), w2.data_ptr(), b2.data_ptr(), _dt(hs), hyper.data_ptr(),
                                       iou.data_ptr(), B, _s()), "cor_decoder_heads")
    return hyper, iou


def mask_prob_minmax(logits):
    """sigmoid + per-sample min-max normalisation of mask logits [B,1,H,W] (utils/vailder.py:426-430)."""
    _dev(logits)
    x = logits.to(torch.float32).contiguous()
    B = x.shape[0]
    out = torch.empty_like(x)
    nat.check(_lib().cor_mask_prob_minmax(x.data_ptr(), out.data_ptr(), B, x.numel() // B, _s()), "cor_mask_prob_minmax")
    return out


def resize_binarize(prob, OH, OW, threshold=0.5):
    """[B,1,H,W] probabilities -> uint8 {0,255} [B,OH,OW] (cv2.INTER_LINEAR semantics, utils/vailder.py:459-473)."""
    _dev(prob)
    assert prob.dtype == torch.float32 and prob.is_contiguous()
    B, H, W = prob.shape[0], prob.shape[-2], prob.shape[-1]
    assert prob.numel() == B * H * W
    out = torch.empty((B, OH, OW), dtype=torch.uint8, device=prob.device)
    nat.check(_lib().cor_resize_binarize(prob.data_ptr(), out.data_ptr(), B, H, W, OH, OW, float(threshold), _s()), "cor_resize_binarize")
    return out


def resize_gray(prob, OH, OW):
    """[B,1,H,W] probabilities -> uint8 [B,OH,OW] = (resized * 255) truncated (cv2.INTER_LINEAR semantics, utils/vailder.py:615-621)."""
    _dev(prob)
    assert prob.dtype == torch.float32 and prob.is_contiguous()
    B, H, W = prob.shape[0], prob.shape[-2], prob.shape[-1]
    assert prob.numel() == B * H * W
    out = torch.empty((B, OH, OW), dtype=torch.uint8, device=prob.device)
    nat.check(_lib().cor_resize_gray(prob.data_ptr(), out.data_ptr(), B, H, W, OH, OW, _s()), "cor_resize_gray")
    return out


def mask_metrics(pred, gt, smooth=1e-5):
    """per-sample [dice, mae, iou, mdice, miou] (utils/trainer_v3_g.py:381-443). pred, gt: [B,...] fp32 of equal shape."""
    _dev(pred, gt)
    assert pred.shape == gt.shape, f"Shape mismatch: pred {tuple(pred.shape)} vs gt {tuple(gt.shape)}"
    p, g = pred.to(torch.float32).contiguous(), gt.to(torch.float32).contiguous()
    B = p.shape[0]
    out = torch.empty((B, 5), dtype=torch.float32, device=p.device)
    nat.check(_lib().cor_mask_metrics(p.data_ptr(), g.data_ptr(), out.data_ptr(), B, p.numel() // B, float(smooth), _s()), "cor_mask_metrics")
    return out

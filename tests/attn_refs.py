"""fp64 references, a-priori per-element bounds, arithmetic emulations, planted errors and the case tables of the attention parity
suite (tests/test_cpu_attn_refs.py proves the bounds on the CPU, tests/test_gpu_attn_kernels.py holds every kernel to them).

REFERENCE. softmax(q.k^T * scale + bias) @ v in fp64 on the operands exactly as the kernel receives them (bf16 operands widen exactly):
plain multi-head attention with Tq != Tk (plain_eval) and SAM attention, global or windowed (sam_eval: partition, bottom/right padding
by pad_row, un-partition; decomposed relative-position bias from the UNSCALED q with index q - k + S - 1, oracle/sam.py:47-58). With
q_prescale = c the caller passes q_given = bf16(q * c); the reference takes q_given and undoes c in fp64 (q = q_given / c).

BOUND. A kernel computes weights w_j (1 + e_j) / sum_k w_k (1 + e'_k) with |e_j|, |e'_j| <= E_j, hence
    |out - ref| <= ((w E) @ |v| + |ref| sum(w E)) / (1 - sum(w E))  +  (Tk + hd) u (w @ |v|)  +  4 u |ref|
(u = 2^-24; second term: the fp32 accumulation of P.V and of the row sum; third: 1 / l, the product with it and the store). E_j is read
off the kernels (Model below carries the switches; `cite` names the lines):
    E_j  = expm1(ln 2 * ds_j) + (4 + 4 steps) u + [P_BF16 = 2^-8 if P is rounded to bf16: see the constant]
    ds_j = log2(e) u ((hd + 2) A_j + 8 (A_j + max_k A_k))                 score error in log2 units
           + [2^-8 log2(e) scale sum_i |q_i k_ji|    if the kernel rounds q * scale * log2(e) to bf16]
           + [log2(e) sum_i |q_i| (|dRh_i| + |dRw_i|) if the kernel rounds fp32 rel-pos tables to bf16; dR = R - bf16(R)]
    A_j  = scale sum_i |q_i k_ji| + sum_i |q_i Rh_i| + sum_i |q_i Rw_i|  (>= every partial sum of the score, >= |s_j|, >= |m|)
  (hd + 2) u A: an fp32 dot product of length hd (fma chain or MFMA) and the scale; 8 u (A + max A): the bias adds (2), the subtraction of
  the running reference m and the exponent's log2(e) product (2 + 1), the fp32 constants scale * log2(e) / q_prescale (2), one spare for
  the lazy reference, which sits within 8 of the maximum; 4 u: v_exp_f32 (1 ulp) twice (p and the rescale factor of its own tile);
  4 u per online-softmax step the weight is carried through (steps = number of key tiles: the factor alpha and the product with it).
  The row sum: win_attn / flash_global_pipe sum the bf16-rounded P (sum2_bf16, flash_attn.hip:69-71,1390), flash_fwd the fp32 P
  (flash_attn.hip:422-423): both are inside |e'_j| <= E_j.
A correct kernel outside its bound means a term is missing here: find it in the code and add it by name, never scale a bound.

EMULATIONS (emulate_*) are honest fp32 / bf16 restatements of the two arithmetic models (bf16 P in key tiles with fp32 accumulation; plain
fp32), PLANTED ERRORS (FAULTS_*) are wrong evaluations in fp64. Inputs (make_plain / make_sam) are seeded, give every key a distinct value
row and plant logit spikes of +30..60 (as test_attention_online_softmax_rescale does) on the first and last key of a tile, the last real
key, a key of a late tile and the memory row just past Tk, so that every planted error moves some output far outside its bound.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np
import torch

from tests.parity_util import U

LOG2E = 1.4426950408889634
LN2 = math.log(2.0)
F32, BF16 = torch.float32, torch.bfloat16
F64 = torch.float64
DT_F32, DT_BF16 = 0, 1                                   # cor_amd._native.F32 / BF16 (checked in the CPU test)
KERNEL_ROWLANE, KERNEL_FEWQ, KERNEL_FLASH_MFMA, KERNEL_FLASH_PIPELINED, KERNEL_WINDOW_BLOCK = 1, 2, 3, 4, 5
ENOSUPPORT = None                                        # expected_kernel_id: "the entry point refuses"
Q_PRESCALE_HD64 = float(np.float32(0.125) * np.float32(1.4426950408889634))
# P rounded to bf16 (8 significant bits, round to nearest even): half a spacing is 2^-9 of the TOP of a binade but 2^-8 of its bottom, so
# the unit round-off is 2^-8. With the exact running maximum the largest p is exactly 1 and the smaller figure looks sufficient; the
# kernels' lazy reference (flash_attn.hip:400-412, 1369-1381) leaves p = 2^x, 0 <= x <= 8, with any mantissa, and an emulation with that
# reference exceeds a 2^-9 model by up to 1.5 on the CPU (tests/test_cpu_attn_refs.py::test_p_rounding_term_is_the_unit_roundoff).
P_BF16 = 2.0 ** -8
TINY_W = 2.0 ** -100                                     # a weight below 2^-126 * 2^8 is flushed by v_exp_f32: absolute, per key


def expected_kernel_id(dtype, hd, Tq, Tk, sam_window, grid):
    """cor_attention_kernel_id's documented rules (attention.hip:340-354) restated: sam_window -1 = cor_attention, 0 = SAM global,
    > 0 = SAM windowed. None where the entry point answers COR_ENOSUPPORT."""
    bf = dtype in (BF16, DT_BF16)
    if sam_window < 0:
        if bf and hd in (64, 72, 80) and Tq >= 64 and Tk >= 64:
            return KERNEL_FLASH_MFMA
        if hd == 16 and Tq <= 8 and Tk >= 512:
            return KERNEL_FEWQ
        return KERNEL_ROWLANE if hd in (16, 32, 64, 72, 80) else ENOSUPPORT
    if bf and hd in (64, 80):
        if sam_window == 0 and grid == 64:
            return KERNEL_FLASH_PIPELINED if hd == 64 else KERNEL_FLASH_MFMA
        if sam_window == 14:
            return KERNEL_WINDOW_BLOCK if hd == 64 else KERNEL_FLASH_MFMA
    return KERNEL_ROWLANE if hd in (16, 32, 64, 80) else ENOSUPPORT


def sam_kernel_name(hd, grid, window, variant, prescaled):
    """Which bf16 matrix-core kernel cor_flash_sam_bf16 launches (flash_attn.hip:1552-1611); `prescaled` = the kernel sees scale_log2 == 1
    (q_prescale = Q_PRESCALE_HD64 at head_dim 64, flash_attn.hip:1549-1550). None where it declines (attn_rowlane takes over)."""
    if hd not in (64, 80) or variant not in (0, 1, 2, 4):
        return None
    if window == 0:
        if grid != 64:
            return None
        if hd == 80:
            return "flash_fwd<1,80>"
        if variant == 4 and prescaled:
            return "flash_global_w64"
        if variant == 0 and prescaled:
            return "flash_global_pipe<CB>"
        if variant in (0, 2, 4):
            return "flash_global_pipe"
        return "flash_fwd<1>"
    if window != 14:
        return None
    if hd == 80:
        return "flash_fwd<2,80>"
    return "flash_fwd<2>" if variant == 1 else "win_attn"


# ======================================================================================================
# error models
# ======================================================================================================
@dataclass(frozen=True)
class Model:
    name: str
    p_bf16: bool          # P rounded to bf16 before the P.V product (P_BF16 per weight)
    q_round: bool         # the kernel rounds q * scale * log2(e) to bf16 itself
    tbl_round: bool       # the kernel rounds the fp32 rel-pos tables to bf16
    tile: int             # keys per online-softmax step
    extra_steps: int      # merge steps after the key loop
    cite: str


MODELS = {
    # one query per lane, fp32 fma chains, chunks of 8 keys, __expf; fp32 tables used as they are
    "rowlane": Model("rowlane", False, False, False, 8, 0, "attention.hip:32-41 (dot_q), 88,97 (bias), 98-150 (softmax), 153-158 (store)"),
    # one key slot per lane (256 slots), per-key steps, 6 butterfly + 1 cross-wave merge
    "fewq": Model("fewq", False, False, False, 256, 8, "attention.hip:179,254 (q * scale), 199-208 / 267-276 (softmax), 211-234 / 278-301 (merges)"),
    # f32 MFMA, tiles of 64 keys, P kept in fp32
    "flash_f32": Model("flash_f32", False, False, False, 64, 0, "attention_f32.hip:72-83 (scores), 86-111 (softmax), 113-125 (P.V), 128-143 (store)"),
    # bf16 MFMA, tiles of 64 keys, P -> bf16; tables through table_frag_hd / table_frag
    "mfma": Model("mfma", True, False, True, 64, 0, "flash_attn.hip:137-142 (table_frag_hd), 264-270 / 301-304 (bias), 358,376,389 (scores), "
                  "403-426 (softmax, P -> bf16 pack8), 442 (P.V), 455-467 (store); flash_global_pipe :552,615,701; flash_global_w64 :932,943"),
    # win_attn: blocks of 32 keys, bias and -m as the score MFMA's C operand, P -> bf16, row sum over the rounded P
    "win_attn": Model("win_attn", True, False, True, 32, 0, "flash_attn.hip:75-79 (table_frag), 1302-1314 (bias), 1359-1365 (scores), 1370-1391 "
                      "(softmax, sum2_bf16), 1402 (P.V), 1411-1456 (store)"),
    # win_attn with a raw q: q * scale * log2(e) rounded to bf16 in the kernel
    "win_attn_raw": Model("win_attn_raw", True, True, True, 32, 0, "win_attn plus flash_attn.hip:1330-1337 (q re-scaled bf16 -> bf16)"),
}


def bf16_round(t):
    """fp64 / fp32 tensor -> its bf16 rounding, in the input's dtype."""
    return t.to(F32).to(BF16).to(t.dtype)


def _core(q, k, v, scale, model, bias=None, abias=None, ds_extra=None, skip=None, want_bound=True):
    """q [N, Tq, hd], k / v [N, Tk, hd] fp64, bias / abias / ds_extra [N, Tq, Tk] (natural units; ds_extra in log2 units).
    skip = (tile, t): planted error, the rescale of tile t skipped. -> (ref, bound or None) [N, Tq, hd]."""
    hd, Tk = q.shape[-1], k.shape[1]
    kt = k.transpose(1, 2)
    s = (q @ kt) * scale
    if bias is not None:
        s = s + bias
    w = torch.softmax(s, dim=-1)
    if skip is not None:
        tile, t = skip
        nt = -(-Tk // tile)
        pad = nt * tile - Tk
        sp = torch.nn.functional.pad(s, (0, pad), value=-math.inf).reshape(*s.shape[:2], nt, tile)
        cm = torch.cummax(sp.amax(-1), dim=-1).values                         # running reference after each tile
        f = torch.exp(cm[..., t] - cm[..., t - 1])[..., None]                # 1 / alpha: what the earlier tiles' sums stay too large by
        w = w.clone()
        w[..., :t * tile] *= f
        w = w / w.sum(-1, keepdim=True)
    ref = w @ v
    if not want_bound:
        return ref, None
    a = (q.abs() @ kt.abs()) * scale
    A = a if abias is None else a + abias
    ds = (LOG2E * U) * ((hd + 2) * A + 8.0 * (A + A.amax(-1, keepdim=True)))
    if model.q_round:
        ds = ds + (P_BF16 * LOG2E) * a                                          # q * scale * log2(e) -> bf16: the same unit round-off
    if ds_extra is not None:
        ds = ds + ds_extra
    steps = -(-Tk // model.tile) + model.extra_steps
    E = torch.expm1(LN2 * ds) + (4 + 4 * steps) * U + (P_BF16 if model.p_bf16 else 0.0)
    wE = w * E + TINY_W
    se = wE.sum(-1, keepdim=True)
    av = v.abs()
    bound = (wE @ av + ref.abs() * se) / (1.0 - se) + (Tk + hd) * U * (w @ av) + 4 * U * ref.abs()
    bound = torch.where(se < 1.0, bound, torch.full_like(bound, math.inf))
    return ref, bound


# ======================================================================================================
# plain multi-head attention
# ======================================================================================================
@dataclass
class Plain:
    """Operands of one cor_attention / cor_attention_f32 call, as values of `dtype` held in fp32. q [B*Tq, H*hd]; k, v
    [B*Tk + 1, H*hd]: the extra row is the memory row just past the last batch's keys (spiked: it must get no weight)."""
    B: int
    H: int
    Tq: int
    Tk: int
    hd: int
    dtype: torch.dtype
    q: torch.Tensor
    k: torch.Tensor
    v: torch.Tensor
    late_tile: int        # 64-key tile index of the planted late spike (0: none)

    @property
    def scale(self):
        return self.hd ** -0.5


def _spike_keys(Tk):
    """Keys that get a logit spike: first / last key of a 64-key tile, the last real key, a key in a late tile."""
    ks = {0, min(63, Tk - 1), Tk - 1}
    if Tk > 64:
        ks |= {64, min(127, Tk - 1)}
    late = 0
    if Tk > 64:
        late = (Tk - 1) // 64
        ks.add(min(late * 64 + 5, Tk - 1))
    return sorted(ks), late


def make_plain(B, H, Tq, Tk, hd, dtype, seed=0, amp=1.0):
    g = torch.Generator().manual_seed(1000 * seed + 7 * Tq + 13 * Tk + hd + 31 * H + B)
    D = H * hd
    q = torch.randn((B * Tq, D), generator=g) * amp
    k = torch.randn((B * Tk + 1, D), generator=g) * amp
    # distinct value rows: a per-key, per-head offset pattern beside the noise
    v = torch.randn((B * Tk + 1, D), generator=g) * amp
    v += (amp * 0.75) * torch.sin(torch.arange(B * Tk + 1, dtype=torch.float32)[:, None] * 0.37 + torch.arange(D, dtype=torch.float32)[None, :] * 1.3)
    keys, late = _spike_keys(Tk)
    scale = hd ** -0.5
    for b in range(B):
        for n, kj in enumerate(keys + [Tk]):                                 # Tk: the row past this batch's keys (the next batch's key 0)
            if kj == Tk and b < B - 1:
                continue                                                     # (that row is a real key of the next batch: keep it)
            qi = (5 * n + 3 * b) % Tq
            for h in range(H):
                qv = q[b * Tq + qi, h * hd:(h + 1) * hd]
                spike = 30.0 + 6.0 * ((n + h) % 6) + 6.0 * amp * amp               # other logits have a standard deviation of amp^2
                if kj == Tk:
                    spike += 40.0                                            # the row past Tk would dominate whatever else the query sees
                k[b * Tk + kj, h * hd:(h + 1) * hd] = qv * (spike / (scale * float(qv.square().sum())))
    q, k, v = (t.to(dtype).to(F32) for t in (q, k, v))
    return Plain(B, H, Tq, Tk, hd, dtype, q, k, v, late)


def _plain_split(P, fault):
    B, H, Tq, Tk, hd = P.B, P.H, P.Tq, P.Tk, P.hd
    q = P.q.to(F64).reshape(B, Tq, H, hd)
    if fault == "past_tk":                                                   # the row past Tk included
        idx = (torch.arange(B)[:, None] * Tk + torch.arange(Tk + 1)[None, :]).reshape(-1)
        k = P.k.to(F64)[idx].reshape(B, Tk + 1, H, hd)
        v = P.v.to(F64)[idx].reshape(B, Tk + 1, H, hd)
    else:
        k = P.k.to(F64)[:B * Tk].reshape(B, Tk, H, hd)
        v = P.v.to(F64)[:B * Tk].reshape(B, Tk, H, hd)
    if fault == "drop_last_key":
        k, v = k[:, :Tk - 1], v[:, :Tk - 1]
    if fault == "head_plus1":
        v = v.roll(-1, dims=2)
    if fault == "batch_plus1":
        k = k.roll(-1, dims=0)
    f = lambda t: t.permute(0, 2, 1, 3).reshape(B * H, t.shape[1], hd)
    return f(q), f(k), f(v)


FAULTS_PLAIN = ("drop_last_key", "past_tk", "skip_rescale", "head_plus1", "batch_plus1", "row_plus1")


def plain_fault_applies(P, fault):
    if fault == "drop_last_key":
        return P.Tk > 1
    if fault == "skip_rescale":
        return P.late_tile > 0
    if fault == "head_plus1":
        return P.H > 1
    if fault == "batch_plus1":
        return P.B > 1 and P.Tk > 1                                          # (one key has weight 1 whatever it holds)
    if fault == "row_plus1":
        return P.B * P.Tq > 1
    return True


def plain_eval(P, model, fault=None, want_bound=True):
    """-> (ref, bound) fp64 [B*Tq, H*hd]."""
    q, k, v = _plain_split(P, fault)
    skip = (64, P.late_tile) if fault == "skip_rescale" else None
    ref, bound = _core(q, k, v, P.scale, model, skip=skip, want_bound=want_bound)
    un = lambda t: None if t is None else t.reshape(P.B, P.H, P.Tq, P.hd).permute(0, 2, 1, 3).reshape(P.B * P.Tq, P.H * P.hd)
    ref, bound = un(ref), un(bound)
    if fault == "row_plus1":
        ref = ref.roll(1, dims=0)
    return ref, bound


def _online(s2, v, tile, p_bf16, sum_rounded, lazy=False):
    """Online softmax in the log2 domain over key tiles, fp32: s2 [N, Tq, Tk] fp32 log2-scores, v [N, Tk, hd] fp32. lazy: the reference m
    moves only when a tile maximum exceeds it by more than 8, as in the matrix-core kernels (flash_attn.hip:400-412): p reaches 2^8 and
    its mantissa is arbitrary, where the exact running maximum makes the largest p exactly 1."""
    N, Tq, Tk = s2.shape
    m = torch.full((N, Tq, 1), -math.inf, dtype=F32)
    l = torch.zeros((N, Tq, 1), dtype=F32)
    o = torch.zeros((N, Tq, v.shape[-1]), dtype=F32)
    for k0 in range(0, Tk, tile):
        st = s2[:, :, k0:k0 + tile]
        mx = st.amax(-1, keepdim=True)
        mn = torch.where(mx > m + 8.0, torch.maximum(m, mx), m) if lazy else torch.maximum(m, mx)
        alpha = torch.exp2(m - mn)
        p = torch.exp2(st - mn)
        pr = p.to(BF16).to(F32) if p_bf16 else p
        l = l * alpha + (pr if (sum_rounded or not p_bf16) else p).sum(-1, keepdim=True)
        o = o * alpha + pr @ v[:, k0:k0 + tile]
        m = mn
    return o * (1.0 / l)


def emulate_plain(P, model, lazy=False):
    """The arithmetic of the kernel family on P in fp32 (bf16 P where the model says so). -> fp32 [B*Tq, H*hd]."""
    q, k, v = (t.to(F32) for t in _plain_split(P, None))
    sl2 = torch.tensor(P.scale, dtype=F32) * torch.tensor(LOG2E, dtype=F32)
    if model.q_round:
        s2 = (q * sl2).to(BF16).to(F32) @ k.transpose(1, 2)
    else:
        s2 = (q @ k.transpose(1, 2)) * sl2
    o = _online(s2, v, min(model.tile, 64), model.p_bf16, model.name.startswith("win_attn"), lazy)
    return o.reshape(P.B, P.H, P.Tq, P.hd).permute(0, 2, 1, 3).reshape(P.B * P.Tq, P.H * P.hd)


# ======================================================================================================
# SAM attention
# ======================================================================================================
@dataclass
class Sam:
    """Operands of one cor_sam_attention call as values of `dtype` held in fp32: qkv [B*grid*grid, 3*H*hd] (q third pre-scaled by c and
    rounded when c != 1), pad_row [3*H*hd] likewise, rel_h / rel_w fp32 [2S-1, hd]."""
    B: int
    H: int
    hd: int
    grid: int
    window: int
    dtype: torch.dtype
    c: float
    qkv: torch.Tensor
    pad: torch.Tensor
    rel_h: torch.Tensor
    rel_w: torch.Tensor
    late_tile: int

    @property
    def S(self):
        return self.window if self.window > 0 else self.grid

    @property
    def nW(self):
        return -(-self.grid // self.window) if self.window > 0 else 1

    @property
    def scale(self):
        return self.hd ** -0.5


def make_sam(B, H, hd, grid, window, dtype, amp=1.0, prescale=False, exact_tables=True, seed=0):
    """prescale: the q third (and pad_row's) multiplied by c = scale * log2(e) as a float32 and rounded to `dtype`, as the engine's packer
    does; exact_tables: rel-pos tables made of bf16-representable fp32 values (the table-rounding term of the bound is then zero)."""
    g = torch.Generator().manual_seed(7000 * seed + 100 * B + 10 * H + hd + 3 * grid + window + int(amp * 100))
    S = window if window > 0 else grid
    T = S * S
    d = H * hd
    n = B * grid * grid
    qkv = torch.randn((n, 3 * d), generator=g) * amp
    pad = torch.randn((3 * d,), generator=g) * amp                            # a pad_row of the data's amplitude
    tamp = 0.3 * max(1.0, 1.0 / amp)                                          # keeps the bias O(1) at small amplitudes too
    rh = torch.randn((2 * S - 1, hd), generator=g) * tamp
    rw = torch.randn((2 * S - 1, hd), generator=g) * tamp
    if exact_tables:
        rh, rw = rh.to(BF16).to(F32), rw.to(BF16).to(F32)
    # distinct value rows
    qkv[:, 2 * d:] += (amp * 0.75) * torch.sin(torch.arange(n, dtype=torch.float32)[:, None] * 0.37 + torch.arange(d, dtype=torch.float32)[None, :] * 1.3)
    # logit spikes inside the first window / the image: key token kj of the key sequence is made to dominate query qi
    scale = hd ** -0.5
    keys, late = _spike_keys(T)
    nW = -(-grid // window) if window > 0 else 1

    def tok(b, t):                                                            # row of qkv holding token t of window 0 of image b, or -1 (padding)
        y, x = divmod(t, S)
        return b * grid * grid + y * grid + x if (y < grid and x < grid) else -1
    for b in range(B):
        for i, kj in enumerate(keys):
            rk, rq = tok(b, kj), tok(b, (5 * i + 3 * b) % T)
            if rk < 0 or rq < 0 or rk == rq:
                continue
            for h in range(H):
                qv = qkv[rq, h * hd:(h + 1) * hd]
                spike = 30.0 + 6.0 * ((i + h) % 6) + 6.0 * amp * amp               # other logits have a standard deviation of amp^2
                qkv[rk, d + h * hd:d + (h + 1) * hd] = qv * (spike / (scale * float(qv.square().sum())))
    c = 1.0
    if prescale:
        c = float(np.float32(scale) * np.float32(LOG2E))
        qkv[:, :d] *= c
        pad[:d] *= c
    qkv, pad = qkv.to(dtype).to(F32), pad.to(dtype).to(F32)
    return Sam(B, H, hd, grid, window, dtype, c, qkv, pad, rh, rw, late)


def _sam_windows(P, fault=None):
    """-> q, k, v fp64 [B, nW, nW, H, T, hd] (q unscaled: the pre-scale constant undone in fp64)."""
    B, H, hd, g, S, nW = P.B, P.H, P.hd, P.grid, P.S, P.nW
    Pd = nW * S
    pad = P.pad.to(F64).reshape(3, H * hd).clone()
    if fault == "pad_zero_kv":
        pad[1:] = 0
    if fault == "pad_zero_all":
        pad[:] = 0
    x = pad.reshape(1, 1, 1, 3, H * hd).repeat(B, Pd, Pd, 1, 1)
    x[:, :g, :g] = P.qkv.to(F64).reshape(B, g, g, 3, H * hd)
    x = x.reshape(B, nW, S, nW, S, 3, H, hd).permute(5, 0, 1, 3, 6, 2, 4, 7).reshape(3, B, nW, nW, H, S * S, hd)
    q, k, v = x[0] / P.c, x[1], x[2]
    if fault == "head_plus1":
        v = v.roll(-1, dims=3)
    if fault == "batch_plus1":
        k = k.roll(-1, dims=0)
    return q, k, v


def _sam_unpartition(P, o, transposed=False):
    """o [B, nW, nW, H, T, hd] -> [B*grid*grid, H*hd]."""
    B, H, hd, g, S, nW = P.B, P.H, P.hd, P.grid, P.S, P.nW
    o = o.reshape(B, nW, nW, H, S, S, hd)
    if transposed:
        o = o.transpose(4, 5)
    o = o.permute(0, 1, 4, 2, 5, 3, 6).reshape(B, nW * S, nW * S, H * hd)
    return o[:, :g, :g].reshape(B * g * g, H * hd)


def _rel_parts(q, R, idx):
    """q [N, Tq, hd], R [2S-1, hd], idx [Tq, S] (table row per (query, key row / column)) -> [N, Tq, S]."""
    Tt = q @ R.T                                                              # [N, Tq, 2S-1]
    return torch.gather(Tt, 2, idx[None].expand(q.shape[0], -1, -1))


FAULTS_SAM = ("drop_last_key", "skip_rescale", "rel_h_off1", "rel_w_off1", "rel_swapped", "bias_scaled_q", "pad_zero_kv", "pad_zero_all",
              "unpartition_T", "head_plus1", "batch_plus1", "row_plus1")


def sam_fault_applies(P, fault):
    if fault in ("pad_zero_kv", "pad_zero_all"):
        return P.window > 0 and P.grid % P.window != 0
    if fault == "skip_rescale":
        return P.late_tile > 0
    if fault == "head_plus1":
        return P.H > 1
    if fault == "batch_plus1":
        return P.B > 1
    return True


def sam_eval(P, model, fault=None, want_bound=True, rows=None):
    """-> (ref, bound) fp64 [B*grid*grid, H*hd]. rows (global attention only): evaluate these query tokens only -> [B, len(rows), H*hd]
    (the bound is per query, so a subset of rows is held to exactly the bound the whole output is)."""
    S, T, hd = P.S, P.S * P.S, P.hd
    q, k, v = _sam_windows(P, fault)
    lead = q.shape[:4]
    q, k, v = (t.reshape(-1, T, hd) for t in (q, k, v))
    N = q.shape[0]
    qsel = torch.arange(T) if rows is None else torch.as_tensor(rows, dtype=torch.long)
    assert rows is None or P.window == 0
    if rows is not None and fault == "unpartition_T":                         # row (qh, qw) holds what belongs to (qw, qh)
        qsel = (qsel % S) * S + qsel // S
    if rows is not None and fault == "row_plus1":                             # row t holds what belongs to row t - 1
        qsel = (qsel - 1) % T
    rh, rw = P.rel_h.to(F64), P.rel_w.to(F64)
    if fault == "rel_swapped":
        rh, rw = rw, rh
    drh = drw = None
    if model.tbl_round:                                                       # the kernel's tables are bf16(R): the reference keeps R, the bound
        drh, drw = (rh - bf16_round(rh)).abs(), (rw - bf16_round(rw)).abs()   # carries |q| . |R - bf16(R)|
        if not (drh.any() or drw.any()):
            drh = drw = None
    ar = torch.arange(S)
    nk = T - 1 if fault == "drop_last_key" else T
    skip = (model.tile if model.tile <= 64 else 64, P.late_tile * (64 // min(model.tile, 64))) if fault == "skip_rescale" else None
    refs, bounds = [], []
    qc = max(1, min(len(qsel), (1 << 22) // T))                               # at most 2^22 scores per piece: query chunks of one head,
    nc = max(1, (1 << 22) // (qc * T))                                        # or several small windows at once
    for n0 in range(0, N, nc):
        kn, vn = k[n0:n0 + nc, :nk], v[n0:n0 + nc, :nk]
        r_n, b_n = [], []
        for q0 in range(0, len(qsel), qc):
            sel = qsel[q0:q0 + qc]
            qq = q[n0:n0 + nc, sel]
            qh, qw = sel // S, sel % S
            ih = (qh[:, None] - ar[None, :] + S - 1)
            iw = (qw[:, None] - ar[None, :] + S - 1)
            if fault == "rel_h_off1":
                ih = (ih + 1).clamp(max=2 * S - 2)
            if fault == "rel_w_off1":
                iw = (iw + 1).clamp(max=2 * S - 2)
            qb = qq * P.scale if fault == "bias_scaled_q" else qq
            two = lambda a, b: (a[..., :, None] + b[..., None, :]).reshape(a.shape[0], len(sel), T)[..., :nk]
            bias = two(_rel_parts(qb, rh, ih), _rel_parts(qb, rw, iw))
            abias = dse = None
            if want_bound:
                abias = two(_rel_parts(qq.abs(), rh.abs(), ih), _rel_parts(qq.abs(), rw.abs(), iw))
                if drh is not None:
                    dse = LOG2E * two(_rel_parts(qq.abs(), drh, ih), _rel_parts(qq.abs(), drw, iw))
            r, bd = _core(qq, kn, vn, P.scale, model, bias, abias, dse, skip, want_bound)
            r_n.append(r)
            b_n.append(bd)
        refs.append(torch.cat(r_n, 1))
        bounds.append(torch.cat(b_n, 1) if want_bound else None)
    ref = torch.cat(refs, 0)
    bound = torch.cat(bounds, 0) if want_bound else None
    if rows is not None:
        un = lambda t: None if t is None else t.reshape(P.B, P.H, len(qsel), hd).permute(0, 2, 1, 3).reshape(P.B, len(qsel), P.H * hd)
        return un(ref), un(bound)
    un = lambda t, tr=False: None if t is None else _sam_unpartition(P, t.reshape(*lead, T, hd), tr)
    ref, bound = un(ref, fault == "unpartition_T"), un(bound)
    if fault == "row_plus1":
        ref = ref.roll(1, dims=0)
    return ref, bound


def emulate_sam(P, model, rows=None, lazy=False):
    """The kernel family's arithmetic in fp32: tables as the kernel feeds them (bf16 for the matrix-core kernels), bias = (R . q_given) *
    (log2(e) / c) from the q the caller passed, scores q_given . k * (scale * log2(e) / c) (+ the in-kernel bf16 rounding of q where the
    model has it), online softmax per key tile. -> fp32, shaped as sam_eval's result."""
    S, T, hd = P.S, P.S * P.S, P.hd
    q, k, v = _sam_windows(P)
    lead = q.shape[:4]
    q, k, v = ((t * (P.c if i == 0 else 1.0)).to(F32).reshape(-1, T, hd) for i, t in enumerate((q, k, v)))        # q_given again
    qsel = torch.arange(T) if rows is None else torch.as_tensor(rows, dtype=torch.long)
    q = q[:, qsel]
    rh, rw = (t.to(BF16).to(F32) if model.tbl_round else t for t in (P.rel_h, P.rel_w))
    f = lambda x: torch.tensor(x, dtype=F32)
    sl2, tsc = f(LOG2E) / f(math.sqrt(hd)) / f(P.c), f(LOG2E) / f(P.c)
    if hd == 64 and abs(float(sl2) - 1.0) < 1e-6:
        sl2, tsc = f(1.0), f(8.0)
    ar = torch.arange(S)
    qh, qw = qsel // S, qsel % S
    bh = _rel_parts(q, rh, qh[:, None] - ar[None, :] + S - 1) * tsc
    bw = _rel_parts(q, rw, qw[:, None] - ar[None, :] + S - 1) * tsc
    outs = []
    nc = max(1, (1 << 22) // (len(qsel) * T))                                 # one head of 4096 keys, or several small windows at once
    for n0 in range(0, q.shape[0], nc):
        qq, kn = q[n0:n0 + nc], k[n0:n0 + nc]
        if model.q_round and float(sl2) != 1.0:
            s2 = (qq * sl2).to(BF16).to(F32) @ kn.transpose(1, 2)
        else:
            s2 = (qq @ kn.transpose(1, 2)) * sl2
        s2 = s2 + (bh[n0:n0 + nc, :, :, None] + bw[n0:n0 + nc, :, None, :]).reshape(qq.shape[0], len(qsel), T)
        outs.append(_online(s2, v[n0:n0 + nc], min(model.tile, 64), model.p_bf16, model.name.startswith("win_attn"), lazy))
    o = torch.cat(outs, 0)
    if rows is not None:
        return o.reshape(P.B, P.H, len(qsel), hd).permute(0, 2, 1, 3).reshape(P.B, len(qsel), P.H * hd)
    return _sam_unpartition(P, o.reshape(*lead, T, hd))


# ======================================================================================================
# case tables (the CPU and the GPU file iterate the same lists)
# ======================================================================================================
OUT_PAIRS = ((F32, F32), (BF16, BF16), (BF16, F32), (F32, BF16))              # (operand dtype, output dtype)
B0, H0 = 2, 3                                                                 # small, not powers of two: the bh -> (b, h) split

# flash_fwd<0>: 1, 2, 3 and 5 key tiles with and without a tail, both sides of the 128-query block
FLASH_HD = (64, 72, 80)
FLASH_SHAPES = ((64, 64), (65, 127), (127, 65), (128, 128), (129, 130), (200, 257))
# attn_rowlane mode 0: around the 128-query block and the 8-key chunk; bf16 at hd 64 / 72 / 80 with Tq or Tk below 64 (the route boundary)
ROWLANE_HD = (16, 32, 64, 72, 80)
ROWLANE_SHAPES = ((1, 1), (7, 7), (128, 8), (129, 9), (7, 63), (129, 63))
ROWLANE_BOUNDARY = ((63, 200), (200, 63))
# attn_fewq (H * B >= 128) / attn_fewq_wide (< 128): hd 16
FEWQ_SHAPES = ((1, 512), (6, 513), (8, 1000), (6, 4096), (8, 512))
FEWQ_BH = ((2, 4), (1, 127), (2, 64))                                         # H * B = 8, 127, 128
FEWQ_NEIGHBOURS = ((9, 512), (8, 511))                                        # route to attn_rowlane
# flash_fwd_f32
F32_SHAPES = ((64, 64), (65, 63), (77, 130), (1, 200), (130, 1))

# SAM global on the matrix cores: (kernel name, variant, prescaled, hd, amplitudes)
GLOBAL_BH = ((1, 1), (2, 3))
GLOBAL_KERNELS = (
    ("flash_global_pipe<CB>", 0, True, 64, (0.05, 1.0, 6.0)),
    ("flash_global_pipe", 2, True, 64, (0.05, 1.0, 6.0)),
    ("flash_global_pipe", 0, False, 64, (1.0,)),
    ("flash_global_pipe", 4, False, 64, (1.0,)),                             # variant 4 without a pre-scaled q runs flash_global_pipe
    ("flash_fwd<1>", 1, False, 64, (1.0,)),
    ("flash_fwd<1>", 1, True, 64, (0.05, 1.0, 6.0)),
    ("flash_global_w64", 4, True, 64, (0.05, 1.0, 6.0)),
    ("flash_fwd<1,80>", 0, False, 80, (1.0,)),
)
# CPU file: the query rows the 4096-key cases are proved on (every spiked query, (5 i + 3 b) % T, is among the first 40)
GLOBAL_ROWS = tuple(sorted(set(range(0, 40)) | set(range(0, 4096, 41)) | {63, 64, 4032, 4095}))

# SAM windowed on the matrix cores: (kernel name, variant, prescaled, hd)
WINDOW_GRIDS = (14, 15, 28, 30)
WINDOW_KERNELS = (
    ("win_attn", 0, False, 64), ("win_attn", 0, True, 64),
    ("flash_fwd<2>", 1, False, 64), ("flash_fwd<2>", 1, True, 64),
    ("flash_fwd<2,80>", 0, False, 80), ("flash_fwd<2,80>", 1, True, 80),
)
WINDOW_AMPS_RAW_WIN_ATTN = (1.0,)                                            # win_attn rounds a raw q itself: amplitudes the CPU file proves

# SAM on attn_rowlane: (grid, window)
ROWLANE_SAM_HD = (16, 32, 64, 80)
ROWLANE_SAM_SHAPES = ((5, 0), (16, 0), (20, 0), (14, 14), (15, 14), (20, 14), (14, 7), (15, 7), (20, 7))


def sam_model_for(name, prescaled):
    if name == "win_attn":
        return MODELS["win_attn" if prescaled else "win_attn_raw"]
    return MODELS["mfma"]


def rowlane_sam_cases():
    """(hd, operand dtype, grid, window) that cor_sam_attention runs on attn_rowlane (modes 1 and 2)."""
    out = []
    for hd in ROWLANE_SAM_HD:
        for T in (F32, BF16):
            for grid, window in ROWLANE_SAM_SHAPES:
                if expected_kernel_id(T, hd, 0, 0, window, grid) == KERNEL_ROWLANE:
                    out.append((hd, T, grid, window))
    return out

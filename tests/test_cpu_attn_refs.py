"""CPU proof of the attention parity suite's references and bounds (tests/attn_refs.py), at every shape the GPU file
(tests/test_gpu_attn_kernels.py) runs: the references equal torch fp64 and the oracle; honest emulations of each arithmetic model lie inside
the a-priori bound; every planted error is rejected wherever it applies; the route table restates cor_attention_kernel_id's rules.
No library load, no GPU."""
import math
import os
import re

import pytest
import torch

from oracle import sam as osam
from tests import attn_refs as R
from tests.parity_util import compare

torch.set_grad_enabled(False)
F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ratio(got, ref, bound):
    rec, fails = compare(got, ref, bound)
    return rec["max_ratio"], fails


def _prove_plain(P, model, lazy=False, out_dtypes=(F32,)):
    """Emulation inside the bound (fp32 and, where asked, bf16 outputs); every applicable planted error outside it."""
    ref, bound = R.plain_eval(P, model)
    em = R.emulate_plain(P, model, lazy)
    for TO in out_dtypes:
        r, fails = _ratio(em.to(TO), ref, bound)
        assert not fails, (model.name, P.B, P.H, P.Tq, P.Tk, P.hd, TO, fails)
    for fault in R.FAULTS_PLAIN:
        if not R.plain_fault_applies(P, fault):
            continue
        bad, _ = R.plain_eval(P, model, fault, want_bound=False)
        for TO in out_dtypes:
            r, fails = _ratio(bad.to(TO), ref, bound)
            assert fails and r > 4.0, (model.name, fault, P.B, P.H, P.Tq, P.Tk, P.hd, TO, r)


def _prove_sam(P, model, rows=None, lazy=False, out_dtypes=(F32, BF16)):
    ref, bound = R.sam_eval(P, model, rows=rows)
    em = R.emulate_sam(P, model, rows, lazy)
    for TO in out_dtypes:
        r, fails = _ratio(em.to(TO), ref, bound)
        assert not fails, (model.name, P.B, P.H, P.hd, P.grid, P.window, P.c, TO, fails)
    for fault in R.FAULTS_SAM:
        if not R.sam_fault_applies(P, fault):
            continue
        bad, _ = R.sam_eval(P, model, fault, want_bound=False, rows=rows)
        for TO in out_dtypes:
            r, fails = _ratio(bad.to(TO), ref, bound)
            assert fails and r > 4.0, (model.name, fault, P.B, P.H, P.hd, P.grid, P.window, P.c, TO, r)


# ======================================================================================================
# the references are the operation
# ======================================================================================================
@pytest.mark.parametrize("B,H,Tq,Tk,hd", [(2, 3, 5, 9, 16), (1, 2, 70, 33, 72), (3, 1, 1, 200, 64)])
def test_plain_reference_equals_torch_fp64(B, H, Tq, Tk, hd):
    P = R.make_plain(B, H, Tq, Tk, hd, F32, seed=3)
    ref, _ = R.plain_eval(P, R.MODELS["rowlane"])
    sp = lambda t, T: t[:B * T].double().reshape(B, T, H, hd).transpose(1, 2)
    want = (torch.softmax(sp(P.q, Tq) @ sp(P.k, Tk).transpose(2, 3) * hd ** -0.5, -1) @ sp(P.v, Tk)).transpose(1, 2).reshape(B * Tq, H * hd)
    assert float((ref - want).abs().max()) <= 1e-13 * float(want.abs().max())


@pytest.mark.parametrize("grid,window,prescale", [(6, 0, False), (7, 0, True), (14, 14, False), (15, 14, True), (9, 7, False), (20, 7, False)])
def test_sam_reference_equals_oracle(grid, window, prescale):
    """sam_eval against oracle.sam: vit_attention over to_windows / from_windows (zero padding AFTER the norm: a padded token's qkv is the
    qkv bias = pad_row) and rel_pos_bias. The operands are an fp64 qkv = x W^T + b; with prescale the q third is multiplied by c first."""
    B, H, hd = 2, 3, 16
    d = H * hd
    g = torch.Generator().manual_seed(grid * 10 + window)
    S = window or grid
    x = torch.randn((B, grid, grid, d), generator=g, dtype=F64)
    sd = {"a.qkv.weight": torch.randn((3 * d, d), generator=g, dtype=F64) / math.sqrt(d), "a.qkv.bias": torch.randn((3 * d,), generator=g, dtype=F64),
          "a.rel_pos_h": torch.randn((2 * S - 1, hd), generator=g, dtype=F64) * 0.3, "a.rel_pos_w": torch.randn((2 * S - 1, hd), generator=g, dtype=F64) * 0.3,
          "a.proj.weight": torch.eye(d, dtype=F64), "a.proj.bias": torch.zeros(d, dtype=F64)}
    if window:
        xw, pad_hw = osam.to_windows(x, window)
        want = osam.from_windows(osam.vit_attention(sd, "a.", xw, H), window, pad_hw, (grid, grid))
    else:
        want = osam.vit_attention(sd, "a.", x, H)
    qkv = x.reshape(-1, d) @ sd["a.qkv.weight"].T + sd["a.qkv.bias"]
    pad = sd["a.qkv.bias"].clone()
    c = 1.0
    if prescale:
        c = 0.3606737554073334
        qkv[:, :d] *= c
        pad[:d] *= c
    P = R.Sam(B, H, hd, grid, window, F32, c, qkv, pad, sd["a.rel_pos_h"], sd["a.rel_pos_w"], 0)
    ref, bound = R.sam_eval(P, R.MODELS["rowlane"])
    assert ref.shape == (B * grid * grid, d) and bound.shape == ref.shape and bool((bound > 0).all())
    assert float((ref - want.reshape(-1, d)).abs().max()) <= 1e-12 * float(want.abs().max())
    # the pieces by themselves: the bias the reference adds is the oracle's
    q, _, _ = R._sam_windows(P)
    q = q.reshape(-1, S * S, hd)
    ar = torch.arange(S)
    tok = torch.arange(S * S)
    ih, iw = (tok // S)[:, None] - ar[None, :] + S - 1, (tok % S)[:, None] - ar[None, :] + S - 1
    bias = (R._rel_parts(q, sd["a.rel_pos_h"], ih)[..., :, None] + R._rel_parts(q, sd["a.rel_pos_w"], iw)[..., None, :]).reshape(q.shape[0], S * S, S * S)
    assert float((bias - osam.rel_pos_bias(q, sd["a.rel_pos_h"], sd["a.rel_pos_w"], S)).abs().max()) <= 1e-12
    if not window:                                                            # a subset of rows is the same rows
        rows = (0, 3, grid * grid - 1)
        r2, b2 = R.sam_eval(P, R.MODELS["rowlane"], rows=rows)
        for sub, full in ((r2, ref), (b2, bound)):                             # (the BLAS blocking differs with the row count: not bitwise)
            assert float((sub - full.reshape(B, grid * grid, d)[:, list(rows)]).abs().max()) <= 1e-12 * float(full.abs().max())


# ======================================================================================================
# emulations inside, planted errors outside: every GPU shape
# ======================================================================================================
@pytest.mark.parametrize("hd", R.FLASH_HD)
def test_flash_fwd0_shapes(hd):
    for Tq, Tk in R.FLASH_SHAPES:
        assert R.expected_kernel_id(BF16, hd, Tq, Tk, -1, 0) == R.KERNEL_FLASH_MFMA
        P = R.make_plain(R.B0, R.H0, Tq, Tk, hd, BF16)
        for lazy in (False, True):
            _prove_plain(P, R.MODELS["mfma"], lazy, (F32, BF16))


@pytest.mark.parametrize("hd", R.ROWLANE_HD)
def test_rowlane_plain_shapes(hd):
    for T in (F32, BF16):
        shapes = R.ROWLANE_SHAPES + (R.ROWLANE_BOUNDARY if hd in (64, 72, 80) else ())
        for Tq, Tk in shapes:
            assert R.expected_kernel_id(T, hd, Tq, Tk, -1, 0) == R.KERNEL_ROWLANE
            _prove_plain(R.make_plain(R.B0, R.H0, Tq, Tk, hd, T), R.MODELS["rowlane"], False, (F32, BF16))


@pytest.mark.parametrize("B,H", R.FEWQ_BH)
def test_fewq_shapes(B, H):
    for T in (F32, BF16):
        for Tq, Tk in R.FEWQ_SHAPES:
            assert R.expected_kernel_id(T, 16, Tq, Tk, -1, 0) == R.KERNEL_FEWQ
            _prove_plain(R.make_plain(B, H, Tq, Tk, 16, T), R.MODELS["fewq"], False, (F32, BF16))
    for Tq, Tk in R.FEWQ_NEIGHBOURS:
        assert R.expected_kernel_id(F32, 16, Tq, Tk, -1, 0) == R.KERNEL_ROWLANE


@pytest.mark.parametrize("hd", R.FLASH_HD)
def test_flash_f32_shapes(hd):
    for Tq, Tk in R.F32_SHAPES:
        _prove_plain(R.make_plain(R.B0, R.H0, Tq, Tk, hd, F32), R.MODELS["flash_f32"])


def _global_sets():
    seen = []
    for name, variant, pre, hd, amps in R.GLOBAL_KERNELS:
        for amp in amps:
            if (pre, hd, amp) not in seen:
                seen.append((pre, hd, amp))
    return seen


@pytest.mark.parametrize("pre,hd,amp", _global_sets())
@pytest.mark.parametrize("B,H", R.GLOBAL_BH)
def test_global_matrix_core_shapes(B, H, pre, hd, amp):
    """The 4096-key cases, on GLOBAL_ROWS (the bound is per query row). Both references of the running maximum."""
    P = R.make_sam(B, H, hd, 64, 0, BF16, amp, pre)
    for name, variant, p2, h2, amps in R.GLOBAL_KERNELS:
        if (p2, h2) == (pre, hd) and amp in amps:
            assert R.sam_kernel_name(hd, 64, 0, variant, pre and hd == 64) == name
    _prove_sam(P, R.MODELS["mfma"], R.GLOBAL_ROWS, lazy=True)


@pytest.mark.parametrize("B,H", [(1, 1), (2, 3)])
def test_global_unrepresentable_tables_carry_their_term(B, H):
    P = R.make_sam(B, H, 64, 64, 0, BF16, 1.0, True, exact_tables=False)
    _prove_sam(P, R.MODELS["mfma"], R.GLOBAL_ROWS, lazy=True)
    Pe = R.make_sam(B, H, 64, 64, 0, BF16, 1.0, True)
    rows = R.GLOBAL_ROWS[:8]
    assert float(R.sam_eval(P, R.MODELS["mfma"], rows=rows)[1].mean()) > float(R.sam_eval(Pe, R.MODELS["mfma"], rows=rows)[1].mean())


@pytest.mark.parametrize("grid", R.WINDOW_GRIDS + (64,))
def test_window_matrix_core_shapes(grid):
    for name, variant, pre, hd in R.WINDOW_KERNELS:
        assert R.sam_kernel_name(hd, grid, 14, variant, pre and hd == 64) == name
        model = R.sam_model_for(name, pre)
        amps = R.WINDOW_AMPS_RAW_WIN_ATTN if model.q_round else (1.0,)
        for amp in amps:
            _prove_sam(R.make_sam(R.B0, R.H0, hd, grid, 14, BF16, amp, pre), model, lazy=True)
    _prove_sam(R.make_sam(R.B0, R.H0, 64, grid, 14, BF16, 1.0, True, exact_tables=False), R.MODELS["win_attn"], lazy=True)


def test_win_attn_raw_q_amplitudes():
    """win_attn rounds a raw q * scale * log2(e) to bf16 itself: the bound grows with the logits. The amplitudes the GPU file may use are
    those at which every planted error is still rejected (this test); at amplitude 6 the term swallows whole keys and the case is void."""
    for amp in R.WINDOW_AMPS_RAW_WIN_ATTN:
        _prove_sam(R.make_sam(R.B0, R.H0, 64, 28, 14, BF16, amp, False), R.MODELS["win_attn_raw"])
    P = R.make_sam(R.B0, R.H0, 64, 28, 14, BF16, 6.0, False)
    ref, bound = R.sam_eval(P, R.MODELS["win_attn_raw"])
    assert float((bound / (ref.abs().max())).max()) > 0.5                     # void: the bound is of the order of the output


@pytest.mark.parametrize("hd", R.ROWLANE_SAM_HD)
def test_rowlane_sam_shapes(hd):
    n = 0
    for hd2, T, grid, window in R.rowlane_sam_cases():
        if hd2 == hd:
            _prove_sam(R.make_sam(R.B0, R.H0, hd, grid, window, T), R.MODELS["rowlane"])
            n += 1
    assert n >= 9                                                             # fp32 everywhere; bf16 wherever the matrix-core kernels decline


@pytest.mark.parametrize("p_bf16", [False, True])
def test_q_rounding_term_in_both_arithmetic_models(p_bf16):
    """Each arithmetic model with the in-kernel rounding of q * scale * log2(e) (only win_attn has it today): the emulation that rounds q
    is inside the bound that carries the term and outside the one that does not (at amplitude 3 the term is what decides)."""
    base = R.MODELS["mfma" if p_bf16 else "flash_f32"]
    rounded = R.Model(base.name + "+q_round", base.p_bf16, True, base.tbl_round, base.tile, base.extra_steps, base.cite)
    P = R.make_plain(R.B0, R.H0, 129, 130, 64, BF16, amp=3.0)
    em = R.emulate_plain(P, rounded)
    ref, with_term = R.plain_eval(P, rounded)
    _, without = R.plain_eval(P, base)
    assert _ratio(em, ref, with_term)[0] <= 1.0
    assert _ratio(em, ref, without)[0] > 1.0
    for fault in ("drop_last_key", "past_tk", "head_plus1", "row_plus1"):
        assert _ratio(R.plain_eval(P, rounded, fault, want_bound=False)[0], ref, with_term)[0] > 4.0, fault


def test_p_rounding_term_is_the_unit_roundoff():
    """A 2^-9 term for P -> bf16 holds only while the largest p is exactly 1 (exact running maximum). With the kernels' lazy reference an
    honest emulation exceeds such a bound; with the unit round-off 2^-8 it does not."""
    P = R.make_plain(R.B0, R.H0, 200, 257, 64, BF16, amp=3.0)
    m = R.MODELS["mfma"]
    em = R.emulate_plain(P, m, lazy=True)
    ref, bound = R.plain_eval(P, m)
    assert _ratio(em, ref, bound)[0] <= 1.0
    old = R.P_BF16
    try:
        R.P_BF16 = 2.0 ** -9
        _, b9 = R.plain_eval(P, m)
    finally:
        R.P_BF16 = old
    assert _ratio(em, ref, b9)[0] > 1.0


# ======================================================================================================
# route table
# ======================================================================================================
def test_route_table_restates_the_documented_rules():
    """The constants and expected_kernel_id against the source of cor_attention_kernel_id and include/cor_amd.h (text only)."""
    from cor_amd import _native as nat
    assert (nat.KERNEL_ROWLANE, nat.KERNEL_FEWQ, nat.KERNEL_FLASH_MFMA, nat.KERNEL_FLASH_PIPELINED, nat.KERNEL_WINDOW_BLOCK) == \
        (R.KERNEL_ROWLANE, R.KERNEL_FEWQ, R.KERNEL_FLASH_MFMA, R.KERNEL_FLASH_PIPELINED, R.KERNEL_WINDOW_BLOCK)
    assert (nat.F32, nat.BF16) == (R.DT_F32, R.DT_BF16)
    assert nat.Q_PRESCALE_HD64 == R.Q_PRESCALE_HD64
    src = open(os.path.join(ROOT, "cor_amd", "csrc", "attention.hip")).read()
    body = src[src.index('extern "C" int cor_attention_kernel_id'):src.index('extern "C" int cor_attention(')]
    for frag in ("(hd == 64 || hd == 72 || hd == 80) && Tq >= 64 && Tk >= 64) return COR_KERNEL_FLASH_MFMA",
                 "hd == 16 && Tq <= 8 && Tk >= 512) return COR_KERNEL_FEWQ",
                 "sam_window == 0 && grid == 64) return hd == 64 ? COR_KERNEL_FLASH_PIPELINED : COR_KERNEL_FLASH_MFMA",
                 "sam_window == 14) return hd == 64 ? COR_KERNEL_WINDOW_BLOCK : COR_KERNEL_FLASH_MFMA"):
        assert frag in body, frag
    hdr = open(os.path.join(ROOT, "include", "cor_amd.h")).read()
    for name, val in (("ROWLANE", 1), ("FEWQ", 2), ("FLASH_MFMA", 3), ("FLASH_PIPELINED", 4), ("WINDOW_BLOCK", 5)):
        assert re.search(r"COR_KERNEL_%s\s*=?\s*%d\b" % (name, val), hdr), name
    e = R.expected_kernel_id
    assert e(BF16, 64, 64, 64, -1, 0) == 3 and e(BF16, 64, 63, 64, -1, 0) == 1 and e(BF16, 64, 64, 63, -1, 0) == 1 and e(F32, 64, 64, 64, -1, 0) == 1
    assert e(F32, 16, 8, 512, -1, 0) == 2 and e(F32, 16, 9, 512, -1, 0) == 1 and e(BF16, 16, 8, 511, -1, 0) == 1 and e(F32, 32, 8, 512, -1, 0) == 1
    assert e(F32, 48, 8, 8, -1, 0) is None and e(F32, 72, 0, 0, 0, 8) is None
    assert e(BF16, 64, 0, 0, 0, 64) == 4 and e(BF16, 80, 0, 0, 0, 64) == 3 and e(BF16, 64, 0, 0, 0, 20) == 1 and e(F32, 64, 0, 0, 0, 64) == 1
    assert e(BF16, 64, 0, 0, 14, 30) == 5 and e(BF16, 80, 0, 0, 14, 30) == 3 and e(BF16, 64, 0, 0, 7, 14) == 1 and e(BF16, 32, 0, 0, 14, 14) == 1

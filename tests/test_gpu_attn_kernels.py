"""Attention kernel-by-kernel parity on the MI355X: every kernel of attention.hip, flash_attn.hip and attention_f32.hip against the fp64
reference and the a-priori per-element bound of tests/attn_refs.py (proved on the CPU by tests/test_cpu_attn_refs.py, which iterates the
same case tables). Every case
  * asserts its route first (cor_attention_kernel_id; where that id cannot tell two kernels apart, the case name carries the kernel that
    cor_flash_sam_bf16's dispatch runs, restated in attn_refs.sam_kernel_name),
  * compares the WHOLE output through parity_util.check (a bf16 output against the interval of admissible bf16 values),
  * writes into a sentinel-filled buffer with guard rows above and below (guard columns too where the entry point takes an output stride)
    and finds the guards untouched, bit for bit.
References are computed once per module (_cached)."""
import pytest
import torch

from tests import attn_refs as R
from tests.parity_util import check, check_bitwise

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

DEV = "cuda:0"
F32, BF16 = torch.float32, torch.bfloat16
GR, GC = 2, 8                       # guard rows above and below, guard columns left and right (8 elements keep every row 16-byte aligned)
SENTINEL = -12345.0
_CACHE = {}


def _ops():
    from cor_amd import ops
    from cor_amd import _native as nat
    return ops, nat


def _cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def _tn(T):
    return "bf16" if T == BF16 else "f32"


class Guarded:
    """A [rows, cols] output view inside a sentinel-filled buffer: GR guard rows above and below, gc guard columns on both sides."""

    def __init__(self, rows, cols, dtype, gc):
        self.buf = torch.full((rows + 2 * GR, cols + 2 * gc), SENTINEL, dtype=dtype, device=DEV)
        self.out = self.buf[GR:GR + rows, gc:gc + cols] if gc else self.buf[GR:GR + rows]
        assert self.out.data_ptr() % 16 == 0

    def assert_guards(self, name):
        b = self.buf.clone()
        b[GR:GR + self.out.shape[0], (b.shape[1] - self.out.shape[1]) // 2:(b.shape[1] + self.out.shape[1]) // 2] = SENTINEL
        want = torch.full_like(b, SENTINEL)
        same = b.view(torch.int16 if b.dtype == BF16 else torch.int32) == want.view(torch.int16 if b.dtype == BF16 else torch.int32)
        assert bool(same.all()), f"{name}: {int((~same).sum())} guard elements were written"


def _route(dtype, hd, Tq, Tk, window, grid):
    _, nat = _ops()
    kid = nat.load().cor_attention_kernel_id(nat.BF16 if dtype == BF16 else nat.F32, hd, Tq, Tk, window, grid)
    assert kid == R.expected_kernel_id(dtype, hd, Tq, Tk, window, grid), (kid, dtype, hd, Tq, Tk, window, grid)
    return kid


# ======================================================================================================
# plain multi-head attention
# ======================================================================================================
def _plain_ref(B, H, Tq, Tk, hd, T, model):
    def make():
        P = R.make_plain(B, H, Tq, Tk, hd, T)
        return (P,) + R.plain_eval(P, R.MODELS[model])
    return _cached(("plain", B, H, Tq, Tk, hd, T, model), make)


def _plain_operands(P, fused):
    """q, k, v on the device: three separate tensors, or column slices of one fused activation (row stride 3 D). The row past the last
    key (spiked) travels with k and v in both layouts."""
    D = P.H * P.hd
    T = P.dtype
    if fused:
        rows = max(P.B * P.Tq, P.B * P.Tk + 1)
        buf = torch.zeros((rows, 3 * D), dtype=T, device=DEV)
        buf[:P.B * P.Tq, :D] = P.q.to(T)
        buf[:P.B * P.Tk + 1, D:2 * D] = P.k.to(T)
        buf[:P.B * P.Tk + 1, 2 * D:] = P.v.to(T)
        return buf[:P.B * P.Tq, :D], buf[:P.B * P.Tk, D:2 * D], buf[:P.B * P.Tk, 2 * D:]
    q, k, v = P.q.to(T).to(DEV), P.k.to(T).to(DEV), P.v.to(T).to(DEV)
    return q, k[:P.B * P.Tk], v[:P.B * P.Tk]


def _run_plain(name, P, ref, bound, TO, fused=False, f32_entry=False):
    ops, _ = _ops()
    q, k, v = _plain_operands(P, fused)
    g = Guarded(P.B * P.Tq, P.H * P.hd, TO, GC)
    fn = ops.attention_f32 if f32_entry else ops.attention
    got = fn(q, k, v, P.B, P.H, P.Tq, P.Tk, P.hd, P.scale, out_dtype=TO, out=g.out)
    assert got.data_ptr() == g.out.data_ptr()
    torch.cuda.synchronize()
    g.assert_guards(name)
    check(name, got, ref, bound)
    return got


@pytest.mark.parametrize("TO", [F32, BF16], ids=_tn)
@pytest.mark.parametrize("fused", [False, True], ids=["separate", "fused"])
@pytest.mark.parametrize("hd", R.FLASH_HD)
def test_flash_fwd0(hd, fused, TO):
    for Tq, Tk in R.FLASH_SHAPES:
        assert _route(BF16, hd, Tq, Tk, -1, 0) == R.KERNEL_FLASH_MFMA
        P, ref, bound = _plain_ref(R.B0, R.H0, Tq, Tk, hd, BF16, "mfma")
        _run_plain(f"attn/flash_fwd<0,{hd}>_{Tq}x{Tk}_{'fused' if fused else 'separate'}_{_tn(TO)}", P, ref, bound, TO, fused)


@pytest.mark.parametrize("T,TO", R.OUT_PAIRS, ids=lambda t: _tn(t))
@pytest.mark.parametrize("hd", R.ROWLANE_HD)
def test_attn_rowlane_mode0(hd, T, TO):
    shapes = R.ROWLANE_SHAPES + (R.ROWLANE_BOUNDARY if hd in (64, 72, 80) else ())
    for Tq, Tk in shapes:
        assert _route(T, hd, Tq, Tk, -1, 0) == R.KERNEL_ROWLANE
        P, ref, bound = _plain_ref(R.B0, R.H0, Tq, Tk, hd, T, "rowlane")
        _run_plain(f"attn/attn_rowlane<0,{hd}>_{Tq}x{Tk}_{_tn(T)}_{_tn(TO)}", P, ref, bound, TO, fused=(Tq + Tk) % 2 == 0)


@pytest.mark.parametrize("T,TO", R.OUT_PAIRS, ids=lambda t: _tn(t))
@pytest.mark.parametrize("B,H", R.FEWQ_BH)
def test_attn_fewq(B, H, T, TO):
    """H * B < 128 runs attn_fewq_wide, from 128 on attn_fewq (attention.hip:305-311): the id is KERNEL_FEWQ for both."""
    kernel = "attn_fewq_wide" if H * B < 128 else "attn_fewq"
    for Tq, Tk in R.FEWQ_SHAPES:
        assert _route(T, 16, Tq, Tk, -1, 0) == R.KERNEL_FEWQ
        P, ref, bound = _plain_ref(B, H, Tq, Tk, 16, T, "fewq")
        _run_plain(f"attn/{kernel}_BH{B * H}_{Tq}x{Tk}_{_tn(T)}_{_tn(TO)}", P, ref, bound, TO)
    if (B, H) == R.FEWQ_BH[0]:
        for Tq, Tk in R.FEWQ_NEIGHBOURS:                                      # one query more / one key fewer: attn_rowlane
            assert _route(T, 16, Tq, Tk, -1, 0) == R.KERNEL_ROWLANE
            P, ref, bound = _plain_ref(B, H, Tq, Tk, 16, T, "rowlane")
            _run_plain(f"attn/attn_rowlane<0,16>_fewq_neighbour_{Tq}x{Tk}_{_tn(T)}_{_tn(TO)}", P, ref, bound, TO)


@pytest.mark.parametrize("T", [F32, BF16], ids=_tn)
def test_attn_fewq_sample_alone_equals_sample_in_the_128_block_launch(T):
    """attn_fewq_wide (one sample: 64 blocks) and attn_fewq (two samples: 128 blocks) merge the same slots in the same order: bitwise."""
    ops, _ = _ops()
    B, H = R.FEWQ_BH[2]
    assert B * H == 128 and H < 128
    for Tq, Tk in ((6, 513), (8, 1000)):
        P, ref, bound = _plain_ref(B, H, Tq, Tk, 16, T, "fewq")
        q, k, v = _plain_operands(P, False)
        big = ops.attention(q, k, v, B, H, Tq, Tk, 16, P.scale, out_dtype=F32)
        for b in range(B):
            one = ops.attention(q[b * Tq:(b + 1) * Tq], k[b * Tk:(b + 1) * Tk], v[b * Tk:(b + 1) * Tk], 1, H, Tq, Tk, 16, P.scale, out_dtype=F32)
            check_bitwise(f"attn/fewq_wide_vs_fewq_{Tq}x{Tk}_{_tn(T)}_b{b}", one, big[b * Tq:(b + 1) * Tq])


@pytest.mark.parametrize("hd", R.FLASH_HD)
def test_flash_fwd_f32(hd):
    """Against the fp32 bound, absolutely; the x3 output is the split [lo | hi | hi] of the fp32 output, bit for bit. cor_attention_f32
    admits every (Tq, Tk) >= 1 (attention_f32.hip:161-169)."""
    ops, _ = _ops()
    for Tq, Tk in R.F32_SHAPES:
        P, ref, bound = _plain_ref(R.B0, R.H0, Tq, Tk, hd, F32, "flash_f32")
        got = _run_plain(f"attn/flash_fwd_f32<{hd}>_{Tq}x{Tk}", P, ref, bound, F32, fused=Tq % 2 == 1, f32_entry=True)
        q, k, v = _plain_operands(P, False)
        g = Guarded(P.B * Tq, 3 * P.H * hd, BF16, GC)
        x3 = ops.attention_f32(q, k, v, P.B, P.H, Tq, Tk, hd, P.scale, out_dtype=ops.X3, out=g.out)
        torch.cuda.synchronize()
        g.assert_guards(f"flash_fwd_f32<{hd},x3>_{Tq}x{Tk}")
        hi = got.to(BF16)
        lo = (got - hi.to(F32)).to(BF16)
        check_bitwise(f"attn/flash_fwd_f32<{hd},x3>_{Tq}x{Tk}", x3, torch.cat([lo, hi, hi], dim=1))


def test_flash_fwd_f32_refusals():
    """Return codes only: head dims the kernel does not have, more than 65535 (sample, head) pairs, an output type it does not write."""
    ops, nat = _ops()
    for hd in (16, 32):
        q = torch.zeros((4, hd), device=DEV)
        with pytest.raises(nat.NativeError):
            ops.attention_f32(q, q, q, 1, 1, 4, 4, hd, 1.0)
    q = torch.zeros((1, 65536 * 64), device=DEV)
    with pytest.raises(nat.NativeError):
        ops.attention_f32(q, q, q, 1, 65536, 1, 1, 64, 1.0)
    lib = nat.load()
    q = torch.zeros((4, 64), device=DEV)
    o = torch.zeros((4, 64), device=DEV, dtype=BF16)
    rc = lib.cor_attention_f32(q.data_ptr(), 256, 64, q.data_ptr(), 256, 64, q.data_ptr(), 256, 64, o.data_ptr(), 256, 64, nat.BF16,
                               1, 1, 4, 4, 64, 1.0, torch.cuda.current_stream().cuda_stream)
    assert rc != 0


# ======================================================================================================
# SAM attention
# ======================================================================================================
def _sam_ref(B, H, hd, grid, window, T, amp, pre, exact, model):
    def make():
        P = R.make_sam(B, H, hd, grid, window, T, amp, pre, exact)
        return (P,) + R.sam_eval(P, R.MODELS[model])
    return _cached(("sam", B, H, hd, grid, window, T, amp, pre, exact, model), make)


def _sam_dev(P):
    def make():
        return tuple(t.to(DEV) for t in (P.qkv.to(P.dtype), P.pad.to(P.dtype), P.rel_h, P.rel_w))
    return _cached(("samdev", id(P)), make)


def _run_sam(name, P, ref, bound, TO, variant=0, reverse_too=True):
    ops, _ = _ops()
    qkv, pad, rh, rw = _sam_dev(P)
    g = Guarded(P.B * P.grid * P.grid, P.H * P.hd, TO, 0)
    got = ops.sam_attention(qkv, pad, rh, rw, P.B, P.H, P.grid, P.window, out_dtype=TO, variant=variant, q_prescale=P.c, out=g.out)
    assert got.data_ptr() == g.out.data_ptr()
    torch.cuda.synchronize()
    g.assert_guards(name)
    check(name, got, ref, bound)
    if reverse_too:                                                           # the work items from the last to the first: the same bits
        rev = ops.sam_attention(qkv, pad, rh, rw, P.B, P.H, P.grid, P.window, out_dtype=TO, variant=variant, q_prescale=P.c, reverse=True)
        check_bitwise(name + "_reverse", rev, got)
    return got


_GLOBAL_IDS = [f"{n}_v{v}_{'prescaled' if p else 'raw'}" for n, v, p, hd, amps in R.GLOBAL_KERNELS]
_GLOBAL_CASES = [(e, amp) for e, k in enumerate(R.GLOBAL_KERNELS) for amp in k[4]]


@pytest.mark.parametrize("B,H", R.GLOBAL_BH)
@pytest.mark.parametrize("entry,amp", _GLOBAL_CASES, ids=[f"{_GLOBAL_IDS[e]}_amp{a}" for e, a in _GLOBAL_CASES])
def test_sam_global_matrix_cores(entry, amp, B, H):
    """Grid 64 (the only size), every (image, head), fp32 and bf16 outputs. The id says FLASH_PIPELINED for every head-dim-64 variant:
    the kernel in the case name is the one flash_attn.hip:1552-1611 launches for (variant, pre-scaled or raw q). Amplitude 6 drives the
    log2-scores to +-100 and beyond (the lazy rescale fires often), 0.05 is nearly uniform attention."""
    name, variant, pre, hd, amps = R.GLOBAL_KERNELS[entry]
    assert _route(BF16, hd, 0, 0, 0, 64) == (R.KERNEL_FLASH_PIPELINED if hd == 64 else R.KERNEL_FLASH_MFMA)
    assert R.sam_kernel_name(hd, 64, 0, variant, pre and hd == 64) == name
    P, ref, bound = _sam_ref(B, H, hd, 64, 0, BF16, amp, pre, True, "mfma")
    assert not pre or hd != 64 or P.c == R.Q_PRESCALE_HD64
    for TO in (F32, BF16):
        _run_sam(f"attn/{name}_v{variant}_{'pre' if pre else 'raw'}_B{B}H{H}_amp{amp}_{_tn(TO)}", P, ref, bound, TO, variant)


@pytest.mark.parametrize("entry", [0, 1, 5, 6, 7], ids=lambda e: _GLOBAL_IDS[e])
def test_sam_global_unrepresentable_tables(entry):
    """fp32 rel-pos tables that are not bf16 values: the kernels round them (table_frag_hd), the reference does not, the bound carries
    |q| . |R - bf16(R)|."""
    name, variant, pre, hd, amps = R.GLOBAL_KERNELS[entry]
    P, ref, bound = _sam_ref(1, 1, hd, 64, 0, BF16, 1.0, pre, False, "mfma")
    for TO in (F32, BF16):
        _run_sam(f"attn/{name}_v{variant}_{'pre' if pre else 'raw'}_fp32tables_{_tn(TO)}", P, ref, bound, TO, variant, reverse_too=False)


_WINDOW_IDS = [f"{n}_v{v}_{'prescaled' if p else 'raw'}" for n, v, p, hd in R.WINDOW_KERNELS]


@pytest.mark.parametrize("grid", R.WINDOW_GRIDS)
@pytest.mark.parametrize("entry", range(len(R.WINDOW_KERNELS)), ids=_WINDOW_IDS)
def test_sam_window_matrix_cores(entry, grid):
    """14: one exact window; 15: 2 x 2 windows, one of them holding a single real token; 28: 2 x 2 exact; 30: 3 x 3 with 12-token padding."""
    name, variant, pre, hd = R.WINDOW_KERNELS[entry]
    assert _route(BF16, hd, 0, 0, 14, grid) == (R.KERNEL_WINDOW_BLOCK if hd == 64 else R.KERNEL_FLASH_MFMA)
    assert R.sam_kernel_name(hd, grid, 14, variant, pre and hd == 64) == name
    model = R.sam_model_for(name, pre)
    for amp in (R.WINDOW_AMPS_RAW_WIN_ATTN if model.q_round else (1.0,)):
        P, ref, bound = _sam_ref(R.B0, R.H0, hd, grid, 14, BF16, amp, pre, True, model.name)
        for TO in (F32, BF16):
            _run_sam(f"attn/{name}_v{variant}_{'pre' if pre else 'raw'}_g{grid}_amp{amp}_{_tn(TO)}", P, ref, bound, TO, variant)


@pytest.mark.parametrize("entry", range(len(R.WINDOW_KERNELS)), ids=_WINDOW_IDS)
def test_sam_window_grid64_once(entry):
    name, variant, pre, hd = R.WINDOW_KERNELS[entry]
    model = R.sam_model_for(name, pre)
    P, ref, bound = _sam_ref(R.B0, R.H0, hd, 64, 14, BF16, 1.0, pre, True, model.name)
    _run_sam(f"attn/{name}_v{variant}_{'pre' if pre else 'raw'}_g64_bf16", P, ref, bound, BF16, variant)


def test_sam_window_unrepresentable_tables():
    for name, variant, pre, hd in R.WINDOW_KERNELS:
        if not pre:
            continue
        model = R.sam_model_for(name, pre)
        P, ref, bound = _sam_ref(R.B0, R.H0, hd, 15, 14, BF16, 1.0, pre, False, model.name)
        for TO in (F32, BF16):
            _run_sam(f"attn/{name}_v{variant}_pre_g15_fp32tables_{_tn(TO)}", P, ref, bound, TO, variant, reverse_too=False)


@pytest.mark.parametrize("T", [F32, BF16], ids=_tn)
@pytest.mark.parametrize("hd", R.ROWLANE_SAM_HD)
def test_sam_on_attn_rowlane(hd, T):
    """Modes 1 (global) and 2 (windowed) of attn_rowlane: fp32 operands everywhere, bf16 operands where the matrix-core kernels decline
    (global at grid != 64, window != 14, head dim 16 / 32). The row-per-lane kernels take the raw q: q_prescale != 1 is refused."""
    ops, nat = _ops()
    n = 0
    for hd2, T2, grid, window in R.rowlane_sam_cases():
        if (hd2, T2) != (hd, T):
            continue
        n += 1
        assert _route(T, hd, 0, 0, window, grid) == R.KERNEL_ROWLANE
        assert T == F32 or R.sam_kernel_name(hd, grid, window, 0, False) is None
        P, ref, bound = _sam_ref(R.B0, R.H0, hd, grid, window, T, 1.0, False, True, "rowlane")
        for TO in (F32, BF16):
            _run_sam(f"attn/attn_rowlane<{2 if window else 1},{hd}>_g{grid}_w{window}_{_tn(T)}_{_tn(TO)}", P, ref, bound, TO)
        qkv, pad, rh, rw = _sam_dev(P)
        with pytest.raises(nat.NativeError):
            ops.sam_attention(qkv, pad, rh, rw, P.B, P.H, grid, window, q_prescale=0.5)
    assert n >= (9 if T == F32 else 6), n


# ======================================================================================================
# batch invariance: one image alone equals the same image inside a batch, bit for bit
# ======================================================================================================
def test_batch_invariance_plain():
    ops, _ = _ops()
    for f32_entry, T, model in ((False, BF16, "mfma"), (True, F32, "flash_f32")):
        fn = ops.attention_f32 if f32_entry else ops.attention
        Tq, Tk, hd = (129, 130, 72) if not f32_entry else (77, 130, 72)
        P, _, _ = _plain_ref(R.B0, R.H0, Tq, Tk, hd, T, model)
        q, k, v = _plain_operands(P, False)
        both = fn(q, k, v, P.B, P.H, Tq, Tk, hd, P.scale, out_dtype=F32)
        for b in range(P.B):
            one = fn(q[b * Tq:(b + 1) * Tq], k[b * Tk:(b + 1) * Tk], v[b * Tk:(b + 1) * Tk], 1, P.H, Tq, Tk, hd, P.scale, out_dtype=F32)
            check_bitwise(f"attn/batch_invariance_{'flash_fwd_f32' if f32_entry else 'flash_fwd<0>'}_b{b}", one, both[b * Tq:(b + 1) * Tq])


@pytest.mark.parametrize("kernel,grid,window", [("win_attn", 30, 14), ("flash_global_pipe<CB>", 64, 0)])
def test_batch_invariance_sam(kernel, grid, window):
    ops, _ = _ops()
    model = "win_attn" if window else "mfma"
    P, _, _ = _sam_ref(R.B0, R.H0, 64, grid, window, BF16, 1.0, True, True, model)
    assert R.sam_kernel_name(64, grid, window, 0, True) == kernel
    qkv, pad, rh, rw = _sam_dev(P)
    both = ops.sam_attention(qkv, pad, rh, rw, P.B, P.H, grid, window, q_prescale=P.c)
    n = grid * grid
    for b in range(P.B):
        one = ops.sam_attention(qkv[b * n:(b + 1) * n], pad, rh, rw, 1, P.H, grid, window, q_prescale=P.c)
        check_bitwise(f"attn/batch_invariance_{kernel}_b{b}", one, both[b * n:(b + 1) * n])

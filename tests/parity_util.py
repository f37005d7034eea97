"""Comparator of the small-kernel parity tests: a result against an fp64 reference under a PER-ELEMENT fp64 bound that is
derived beside the reference (tests/small_kernel_refs.py), never fitted to what a kernel returns.

  check(name, got, ref, bound)        |got - ref| <= bound element by element; a bf16 `got` must lie in
                                      [bf16_rne(ref - bound), bf16_rne(ref + bound)] (no blanket bf16 ulp)
  check_bitwise(name, got, want)      pure moves and single correctly rounded operations: equal bits, NaN compared as NaN-ness
  check_decision(name, got, v, ...)   thresholded / quantised outputs: equal to the fp64 decision except where the fp64 value lies
                                      within delta of the decision boundary

Non-finite policy of check(): nonfinite="finite" (default) demands a finite output and a finite reference; nonfinite="agree" demands NaN
where the reference has NaN, the same infinity where it has one, and holds every other element to its bound.

Every check appends {name, max_abs, max_ratio, finite, n} to the parity report of tests/test_gpu_parity.py (its REPORT file; max_ratio = max error / bound <= 1 for a
pass: the slack of each bound stays on record). compare() computes the same record without writing or asserting.
"""
from __future__ import annotations

import json
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24            # unit round-off of fp32
TINY = 2.0 ** -126        # smallest normal fp32: the absolute floor of a result that may underflow or be flushed


def to64(t):
    """A tensor / array of any float or integer dtype as a float64 numpy array (bf16 widens exactly)."""
    if isinstance(t, torch.Tensor):
        return t.detach().to("cpu").to(torch.float64).numpy()
    return np.asarray(t, dtype=np.float64)


def bf16_rne(x):
    """fp64 -> the nearest bfloat16 (ties to even, overflow to inf), returned as fp64. Direct: no double rounding through fp32."""
    x = np.asarray(x, dtype=np.float64)
    out = np.array(x, copy=True)
    fin = np.isfinite(x) & (x != 0)
    _, e = np.frexp(x[fin])                                     # |x| = m * 2^e, 0.5 <= m < 1
    q = np.ldexp(1.0, np.maximum(e, -125) - 8)                  # spacing of bf16 (8 significant bits) at x; subnormals share 2^-133
    r = np.rint(x[fin] / q) * q                                 # rint: ties to even
    r = np.where(np.abs(r) > 3.3895313892515355e38, np.sign(r) * np.inf, r)
    out[fin] = r
    return out


def _record(name, rec, report):
    if not report:
        return
    from tests.test_gpu_parity import REPORT                   # one report file for every GPU parity test
    try:
        os.makedirs(os.path.dirname(REPORT), exist_ok=True)
        with open(REPORT, "a") as f:
            f.write(json.dumps(dict(name=name, **rec)) + "\n")
    except OSError:
        pass


def compare(got, ref, bound, nonfinite="finite"):
    """-> (record, list of failure strings); record = {max_abs, max_ratio, finite, n}."""
    is_bf16 = isinstance(got, torch.Tensor) and got.dtype == torch.bfloat16
    g, r, b = to64(got), to64(ref), np.broadcast_to(to64(bound), np.shape(to64(ref)))
    fails = []
    if g.shape != r.shape:
        return dict(max_abs=float("inf"), max_ratio=float("inf"), finite=False, n=int(g.size)), [f"shape {g.shape} != {r.shape}"]
    assert nonfinite in ("finite", "agree")
    finite = bool(np.isfinite(g).all())
    if not np.all(b >= 0) or np.isnan(b).any():
        fails.append("the bound itself is negative or NaN")
    if nonfinite == "finite":
        if not finite:
            fails.append(f"{int((~np.isfinite(g)).sum())} non-finite outputs")
        if not np.isfinite(r).all():
            fails.append("non-finite reference under the 'finite' policy")
        live = np.isfinite(g) & np.isfinite(r)
    else:
        rn, ri = np.isnan(r), np.isinf(r)
        if not np.array_equal(np.isnan(g), rn):
            fails.append(f"NaN positions differ at {int((np.isnan(g) != rn).sum())} elements")
        if not (np.array_equal(np.isinf(g), ri) and np.array_equal(g[ri], r[ri])):
            fails.append("infinities differ from the reference")
        live = np.isfinite(g) & np.isfinite(r)
    with np.errstate(invalid="ignore"):
        err = np.abs(g - r)
    if is_bf16:                                                 # the interval of bf16 values a result within `b` of ref may round to
        lo, hi = bf16_rne(r - b), bf16_rne(r + b)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = err / np.maximum(np.abs(hi - r), np.abs(r - lo))       # against the half-width of the interval (for the record)
        ratio = np.where(g == r, 0.0, ratio)
        bad = live & ((g < lo) | (g > hi))
        ratio = np.where(bad, np.maximum(ratio, 1.0 + 2.0 ** -20), np.where(live, np.minimum(ratio, 1.0), ratio))
    else:
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = err / b
        ratio = np.where(err == 0, 0.0, ratio)
        bad = live & (err > b)
    ratio = np.where(live, np.nan_to_num(ratio, nan=np.inf), 0.0)
    if bad.any():
        i = int(np.argmax(np.where(live, ratio, -1.0)))
        fails.append(f"{int(bad.sum())}/{bad.size} elements outside their bound; worst at flat index {i}: got {g.flat[i]!r} ref {r.flat[i]!r} "
                     f"bound {b.flat[i]!r}")
    rec = dict(max_abs=float(err[live].max()) if live.any() else 0.0, max_ratio=float(ratio.max()) if ratio.size else 0.0, finite=finite,
               n=int(g.size))
    return rec, fails


def check(name, got, ref, bound, nonfinite="finite", report=True):
    rec, fails = compare(got, ref, bound, nonfinite)
    _record(name, rec, report)
    assert not fails, f"{name}: " + "; ".join(fails) + f"; {rec}"
    return rec


def _bits(t):
    if isinstance(t, torch.Tensor):
        t = t.detach().to("cpu").contiguous()
        if t.dtype == torch.bfloat16:
            return t.view(torch.int16).numpy().view(np.uint16), np.isnan(t.float().numpy())
        t = t.numpy()
    t = np.ascontiguousarray(t)
    if t.dtype.kind == "f":
        return t.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[t.dtype.itemsize]), np.isnan(t)
    return t, np.zeros(t.shape, dtype=bool)


def compare_bitwise(got, want):
    gb, gn = _bits(got)
    wb, wn = _bits(want)
    if gb.shape != wb.shape or gb.dtype != wb.dtype:
        return dict(max_abs=float("inf"), max_ratio=float("inf"), finite=False, n=int(gb.size)), [f"{gb.dtype}{gb.shape} != {wb.dtype}{wb.shape}"]
    diff = (gn != wn) | (~wn & (gb != wb))                      # NaN: NaN-ness only (the payload is not part of any contract here)
    g64 = to64(got)
    with np.errstate(invalid="ignore"):
        err = np.abs(g64 - to64(want))
    err = np.where(diff, np.nan_to_num(err, nan=np.inf, posinf=np.inf), 0.0)
    rec = dict(max_abs=float(err.max()) if err.size else 0.0, max_ratio=float("inf") if diff.any() else 0.0,
               finite=bool(np.isfinite(g64).all()), n=int(gb.size))
    fails = []
    if diff.any():
        i = int(np.argmax(diff))
        fails.append(f"{int(diff.sum())}/{diff.size} elements differ in bits; first at flat index {i}: got {g64.flat[i]!r} want {to64(want).flat[i]!r}")
    return rec, fails


def check_bitwise(name, got, want, report=True):
    rec, fails = compare_bitwise(got, want)
    _record(name, rec, report)
    assert not fails, f"{name}: " + "; ".join(fails)
    return rec


def compare_decision(got, value, decide, margin, slack=0):
    """got: integer outputs; value: the fp64 quantity decided on; decide(value) -> the fp64-exact output; margin(value) -> fp64 distance
    of value to the nearest decision boundary RELATIVE to delta (>= 1: well clear). A mismatch is allowed only where margin < 1, and
    then by at most `slack` output steps (0: any of the two sides, for a two-valued output)."""
    g = to64(got)
    v = to64(value)
    want = decide(v)
    mis = g != want
    near = margin(v) < 1.0
    bad = mis & ~near
    if slack:
        bad |= mis & (np.abs(g - want) > slack)
    rec = dict(max_abs=float(np.abs(g - want).max()) if g.size else 0.0, max_ratio=float("inf") if bad.any() else 0.0, finite=True,
               n=int(g.size), mismatches=int(mis.sum()), near_boundary=int(near.sum()))
    fails = []
    if bad.any():
        i = int(np.argmax(bad))
        fails.append(f"{int(bad.sum())}/{bad.size} outputs differ from the fp64 decision away from a boundary; first at flat index {i}: "
                     f"got {g.flat[i]!r} want {want.flat[i]!r} value {v.flat[i]!r}")
    return rec, fails


def check_decision(name, got, value, decide, margin, slack=0, report=True):
    rec, fails = compare_decision(got, value, decide, margin, slack)
    _record(name, rec, report)
    assert not fails, f"{name}: " + "; ".join(fails)
    return rec

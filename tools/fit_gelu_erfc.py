"""Coefficients of csrc/omni_internal.h::omni_gelu2 (the one-branch packed GELU of the GEMM epilogues).

    gelu(v) = v * (c0 - c1 * E),   E = exp2(p(t)) ~ erfc(t / sqrt 2),   t = min(|v|, 6 sqrt 2),   c1 = copysign(0.5, v),  c0 = 0.5 + c1

p is ONE polynomial in |v| for log2(erfc(|v| / sqrt 2)) on the whole clamped range (log2(e) and the 1 / sqrt 2 are inside the
coefficients).  What matters is the ABSOLUTE error of E (for v > 0 it is the relative error of the result; for v < 0 nothing
cancels), so the fit is a weighted minimax (Lawson's iteration on a dense Chebyshev grid, float64) of  E(t) ln 2 (p(t) - log2 erfc)
with the weight floored at 1e-3 to keep the far negative tail relatively accurate too.  The script prints the float32 coefficients and
the error of the float32 Horner evaluation against a float64 GELU, next to the same figures of the two-polynomial `omni_gelu`.
    python tools/fit_gelu_erfc.py [degree=10]"""
import sys

import numpy as np
from scipy.special import erf, erfc

TMAX = 6.0 * np.sqrt(2.0)


def fit(deg, iters=400):
    n = 6000
    t = 0.5 * TMAX * (1 - np.cos(np.pi * (np.arange(n) + 0.5) / n))
    f = np.log2(erfc(t / np.sqrt(2.0)))
    wt = np.maximum(erfc(t / np.sqrt(2.0)), 1e-3) * np.log(2.0)
    V = np.vander(t / TMAX, deg + 1, increasing=True)
    lw = np.ones(n)
    best = None
    for _ in range(iters):
        sw = np.sqrt(lw) * wt
        c, *_ = np.linalg.lstsq(V * sw[:, None], f * sw, rcond=None)
        e = np.abs(V @ c - f) * wt
        if best is None or e.max() < best[0]:
            best = (e.max(), c)
        lw = lw * (e + 1e-300)
        lw /= lw.sum()
    return best[1] / TMAX ** np.arange(deg + 1), best[0]


def fma32(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def gelu_onebranch(v, coef):
    v = v.astype(np.float32)
    t = np.minimum(np.abs(v), np.float32(TMAX))
    p = np.full_like(v, np.float32(coef[-1]))
    for c in coef[-2::-1]:
        p = fma32(p, t, np.float32(c))
    E = np.exp2(p.astype(np.float64)).astype(np.float32)
    c1 = np.copysign(np.float32(0.5), v)
    c0 = (np.float32(0.5) + c1).astype(np.float32)
    return (v * fma32(-c1, E, c0)).astype(np.float32)


def gelu_two_poly(v):
    v = v.astype(np.float32)
    a = (v * np.float32(0.70710678118654752440)).astype(np.float32)
    t = np.minimum(np.abs(a), np.float32(6.0)); s = (t * t).astype(np.float32)
    r = fma32(np.float32(-1.72853470e-5), t, np.float32(3.83197126e-4))
    u = fma32(np.float32(-3.88396438e-3), t, np.float32(2.42546219e-2))
    r = fma32(r, s, u)
    for c in (-1.06777847e-1, -6.34846687e-1, -1.28717512e-1):
        r = fma32(r, t, np.float32(c))
    r = fma32(r, t, -t)
    big = np.copysign((np.float32(1.0) - np.exp(r.astype(np.float64)).astype(np.float32)).astype(np.float32), a)
    q = np.full_like(a, -5.96761703e-4)
    for c in (4.99119423e-3, -2.67681349e-2, 1.12819925e-1, -3.76125336e-1, 1.28379166e-1):
        q = fma32(q, s, np.float32(c))
    e = np.where(t > np.float32(0.927734375), big, fma32(q, a, a))
    return ((np.float32(0.5) * v).astype(np.float32) * (np.float32(1.0) + e).astype(np.float32)).astype(np.float32)


def errors(got, x):
    x64 = x.astype(np.float64)
    ref = x64 * 0.5 * (1.0 + erf(x64 / np.sqrt(2.0)))
    neg = x64 * 0.5 * erfc(-x64 / np.sqrt(2.0))               # the same value without cancellation where x < 0
    ref = np.where(x64 < 0, neg, ref)
    err = np.abs(got.astype(np.float64) - ref)
    nz = ref != 0
    return err.max(), (err[nz] / np.abs(ref[nz])).max()


if __name__ == "__main__":
    deg = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    coef, e = fit(deg)
    c32 = coef.astype(np.float32)
    print(f"degree {deg}: weighted minimax error of E (float64 coefficients) {e:.3e}")
    print("coefficients (constant first):", ", ".join(f"{c:.9e}f" for c in c32))
    x = np.concatenate([np.linspace(-8, 8, 400001), np.random.default_rng(0).normal(0, 1.5, 400000)]).astype(np.float32)
    print("one-branch  max abs %.4e  max rel %.4e" % errors(gelu_onebranch(x, c32), x))
    print("two-poly    max abs %.4e  max rel %.4e" % errors(gelu_two_poly(x), x))

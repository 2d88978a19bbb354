"""csrc/omni_internal.h::omni_gelu2 (the one-branch packed GELU of the GEMM epilogues) restated in numpy with every operation
rounded to float32, against float64 x * 0.5 * (1 + erf(x / sqrt 2)).

The bound is the accuracy of the formula it replaces in those epilogues: maximum absolute and maximum relative error must each be
no larger than those of `omni_gelu` (two erf polynomials + select, restated below as in tests/test_host_cpu.py::test_erf_polynomial)
on the same samples.  Measured on these samples (max abs / max rel):
    one-branch (omni_gelu2)   3.84e-07 / 1.00e+00, on the inputs whose reference is a normal number 5.52e-04
    two-polynomial omni_gelu  4.47e-07 / 1.00e+00, on the inputs whose reference is a normal number 1.00e+00
The maximum absolute error of both is the final rounding at |x| ~ 8; the relative one is taken where the reference is not zero, and
the subnormals next to 0 (where x / 2 is not representable) put it at 1.0 for both; the two-polynomial form also reaches 1.0 on normal
numbers because it returns 0 below x = -5.6 (1 + erf cancels for x < 0).

Also checked bitwise on the same samples, the two exact rewrites that went into every epilogue with it: fma(acc, 2^-k, bias) against
acc * 2^-k + bias, and v * fma(0.5, e, 0.5) against 0.5 * v * (1 + e)."""
import numpy as np
import pytest

SQRT2 = np.sqrt(2.0)
TMAX = np.float32(8.48528137423857)           # 6 sqrt 2: the clamp of |x|
# p(t) ~ log2 erfc(t / sqrt 2), highest degree first (tools/fit_gelu_erfc.py 11)
COEF = (1.137868688e-09, -5.171069262e-08, 1.014483701e-06, -1.117507963e-05, 7.388171798e-05, -2.645340865e-04, -3.723767077e-05,
        6.994847674e-03, -5.247364566e-02, -4.592104554e-01, -1.151105404e+00, 1.941864447e-08)


def f32(x):
    return np.asarray(x, np.float64).astype(np.float32)


def fma(a, b, c):
    return f32(np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64))


def around(x, n=64):
    """all float32 values within n ulp of x, both sides"""
    out = [np.float32(x)]
    for d in (np.float32(np.inf), np.float32(-np.inf)):
        v = np.float32(x)
        for _ in range(n):
            v = np.nextafter(v, d)
            out.append(v)
    return np.array(out, np.float32)


@pytest.fixture(scope="module")
def samples():
    x = np.concatenate([np.linspace(-8, 8, 400001), np.random.default_rng(0).normal(0, 1.5, 400000)]).astype(np.float32)
    return np.concatenate([x, around(0.0), around(TMAX), around(-TMAX)])


@pytest.fixture(scope="module")
def ref64(samples):
    from scipy.special import erf, erfc
    x = samples.astype(np.float64)
    # for x < 0 the same value through erfc: the float64 1 + erf would itself cancel
    return np.where(x < 0, x * 0.5 * erfc(-x / SQRT2), x * 0.5 * (1.0 + erf(x / SQRT2)))


def gelu_onebranch(v):
    t = np.minimum(np.abs(v), TMAX)
    p = fma(np.float32(COEF[0]), t, np.float32(COEF[1]))
    for c in COEF[2:]:
        p = fma(p, t, np.float32(c))
    E = f32(np.exp2(p.astype(np.float64)))
    c1 = np.copysign(np.float32(0.5), v)
    c0 = f32(np.float32(0.5) + c1)
    return f32(v * fma(-c1, E, c0))


def erf_two_poly(a):
    t = np.minimum(np.abs(a), np.float32(6.0)); s = f32(t * t)
    r = fma(np.float32(-1.72853470e-5), t, np.float32(3.83197126e-4))
    u = fma(np.float32(-3.88396438e-3), t, np.float32(2.42546219e-2))
    r = fma(r, s, u)
    for c in (-1.06777847e-1, -6.34846687e-1, -1.28717512e-1):
        r = fma(r, t, np.float32(c))
    r = fma(r, t, -t)
    big = np.copysign(f32(np.float32(1.0) - f32(np.exp(r.astype(np.float64)))), a)
    q = np.full_like(a, -5.96761703e-4)
    for c in (4.99119423e-3, -2.67681349e-2, 1.12819925e-1, -3.76125336e-1, 1.28379166e-1):
        q = fma(q, s, np.float32(c))
    return np.where(t > np.float32(0.927734375), big, fma(q, a, a))


def gelu_two_poly(v):
    """omni_gelu: 0.5f * v * (1.0f + omni_erff(v * 0.70710678f)), left to right"""
    e = erf_two_poly(f32(v * np.float32(0.70710678118654752440)))
    return f32(f32(np.float32(0.5) * v) * f32(np.float32(1.0) + e))


def errors(got, ref):
    err = np.abs(got.astype(np.float64) - ref)
    nz = ref != 0
    return float(err.max()), float((err[nz] / np.abs(ref[nz])).max())


def test_onebranch_gelu_is_no_worse_than_the_two_polynomial_form(samples, ref64):
    new_abs, new_rel = errors(gelu_onebranch(samples), ref64)
    old_abs, old_rel = errors(gelu_two_poly(samples), ref64)
    print(f"one-branch max abs {new_abs:.4e} max rel {new_rel:.4e} | two-polynomial max abs {old_abs:.4e} max rel {old_rel:.4e}")
    assert new_abs <= old_abs, (new_abs, old_abs)
    assert new_rel <= old_rel, (new_rel, old_rel)
    # the few-ulp neighbourhood of 0 holds subnormals, where x / 2 is not representable and both forms reach 1.0: the same comparison
    # on the inputs whose reference is a normal number
    normal = np.abs(ref64) >= 2.0 ** -126
    _, new_rel_n = errors(gelu_onebranch(samples[normal]), ref64[normal])
    _, old_rel_n = errors(gelu_two_poly(samples[normal]), ref64[normal])
    print(f"normal references only: one-branch max rel {new_rel_n:.4e} | two-polynomial max rel {old_rel_n:.4e}")
    assert new_rel_n <= old_rel_n, (new_rel_n, old_rel_n)
    assert np.isfinite(gelu_onebranch(samples)).all()


def test_fma_with_power_of_two_scale_is_mul_add_bitwise(samples):
    """acc * 2^-k is exact, so fma(acc, 2^-k, bias) rounds the same sum once: same bits as the product followed by the sum"""
    acc = samples
    bias = np.roll(samples, 12345)
    for k in (0, 1, 5, 9, 14):
        osc = np.float32(2.0 ** -k)
        assert np.array_equal(fma(acc, osc, bias).view(np.uint32), f32(f32(acc * osc) + bias).view(np.uint32)), k


def test_half_fold_is_bitwise(samples):
    """v * fma(0.5, e, 0.5) against (0.5 * v) * (1 + e) with e = erf of the two-polynomial form: fma(0.5, e, 0.5) is the correctly
    rounded (1 + e) / 2, and halving commutes with rounding outside the subnormal range"""
    v = samples
    e = erf_two_poly(f32(v * np.float32(0.70710678118654752440)))
    a = f32(f32(np.float32(0.5) * v) * f32(np.float32(1.0) + e))
    b = f32(v * fma(np.float32(0.5), e, np.float32(0.5)))
    normal = (np.abs(v) >= np.float32(2.0 ** -100)) | (v == 0)       # the samples around 0 reach into the subnormals
    assert np.array_equal(a[normal].view(np.uint32), b[normal].view(np.uint32))
    assert np.allclose(a[~normal], b[~normal], rtol=0, atol=2.0 ** -148)

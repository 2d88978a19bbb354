"""The per-pixel bounds of tests/conv_f64.py are loose enough to hold and tight enough to matter (pure torch, no kernels).

Accepted: a float32 F.conv2d against both f32 bounds (exact f32 and split-f16 plans promise f32-class results), and f16-rounded operands
with f32 accumulation and an f16 output against the f16 bound — over shapes of the kernel cases, Cout = 1 included (single-value rows,
where cancellation makes the relative error largest).  Rejected: five ways for a rewritten kernel to be wrong, each fed to the same
comparison the kernel checks use (`seg_err` per output pixel against the float64 convolution); each test prints whether the old
whole-tensor check (gpu_checks.check_conv: max|err| / max|ref| < 2e-5) would have accepted the defect."""
import math

import pytest
import torch
import torch.nn.functional as F

import conv_f64 as C
import plan_interp as PI

F64 = torch.float64
B, H, W, K3, S2, CIN, COUT = 2, 19, 17, 3, 2, 24, 40       # conv_f64.S_3x3_S2 with the generic loader's Cin = 6 V (f32): M = 180, K = 216


def _old_accepts(y, ref, tol=2e-5):
    return float((y.to(F64) - ref.to(F64)).abs().max() / ref.to(F64).abs().max()) < tol


def _operands(seed, cin=CIN, cout=COUT, k=K3):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, cin, H, W, generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) / math.sqrt(cin * k * k)
    return x, w, torch.randn(cout, generator=g)


def _rows(y):
    return y.permute(0, 2, 3, 1).reshape(-1, y.shape[1])


def _ref(x, w, b, s=S2):
    return _rows(F.conv2d(x.to(F64), w.to(F64), b.to(F64), stride=s, padding=w.shape[-1] // 2))


def _judge(name, defect, ref, fams=("f32", "split")):
    e, i = C.seg_err(defect, ref, ref.shape[1])
    old = _old_accepts(defect, ref)
    cout = ref.shape[1]
    print(f"{name}: defect {e:.2e} at row {i}; bounds {[C.bound(f, cout) for f in fams]}; old whole-tensor check accepts the defect: {old}")
    for f in fams:
        assert e > C.bound(f, cout), (name, f, e)
    return old


@pytest.mark.parametrize("cin,cout,k,s", [(24, 40, 3, 2), (24, 1, 3, 2), (48, 1, 1, 2), (160, 1, 1, 1), (96, 72, 1, 1), (64, 1, 3, 1)])
def test_float32_convolution_is_accepted_by_both_f32_bounds(cin, cout, k, s):
    worst = 0.0
    for seed in range(4):
        x, w, b = _operands(seed, cin, cout, k)
        y = _rows(F.conv2d(x, w, b, stride=s, padding=k // 2))
        worst = max(worst, C.seg_err(y, _ref(x, w, b, s), cout)[0])
    print(f"float32 conv2d Cin {cin} Cout {cout} k{k}s{s}: {worst:.2e}")
    assert worst <= C.bound("f32", cout) and worst <= C.bound("split", cout)


@pytest.mark.parametrize("cin,cout,k,s", [(48, 40, 3, 2), (48, 1, 3, 2), (96, 72, 1, 1), (160, 1, 1, 1)])
def test_f16_operands_with_f32_accumulation_are_accepted_by_the_f16_bound(cin, cout, k, s):
    worst = 0.0
    for seed in range(4):
        x, w, b = _operands(seed, cin, cout, k)
        xq, wq = x.half().float(), w.half().float()
        y = _rows(F.conv2d(xq, wq, b, stride=s, padding=k // 2)).half()
        worst = max(worst, C.seg_err(y, _ref(xq, wq, b, s), cout)[0])
    print(f"f16 operands, f32 accumulation, f16 output Cin {cin} Cout {cout} k{k}s{s}: {worst:.2e}")
    assert worst <= C.bound("f16", cout)


def test_padding_tap_multiplied_by_a_neighbour_is_rejected():
    """output pixel (0, 0, 3) lies on the top border: its tap (r = 0, s = 1) is padding.  The defect multiplies that ONE tap by the
    pixel below it instead of zero — one of 1620 rows is wrong."""
    x, w, b = _operands(0)
    ref = _ref(x, w, b)
    y = ref.clone()
    wo = 3
    y[wo] += w[:, :, 0, 1].to(F64) @ x[0, :, 0, wo * S2].to(F64)
    _judge("padding tap not zeroed", y, ref)


def test_dropped_last_ragged_k_vector_is_rejected():
    """generic loader, K = 216 = 13 slices of 16 + 8: the last 4-wide vector (tap (2, 2), channels 20 .. 23) never loaded"""
    x, w, b = _operands(1)
    ref = _ref(x, w, b)
    wd = w.clone()
    wd[:, 20:24, 2, 2] = 0.0
    _judge("last ragged K vector dropped", _ref(x, wd, b), ref)


def test_missing_split_k_partial_of_one_tile_is_rejected():
    """3 splits over 14 K slices (5 + 5 + 4 slices of 16): the last split's partial is missing from the sum of rows 64 .. 127"""
    x, w, b = _operands(2)
    ref = _ref(x, w, b)
    w2 = w.permute(0, 2, 3, 1).reshape(COUT, -1).clone()
    w2[:, 160:] = 0.0
    part = _ref(x, w2.view(COUT, K3, K3, CIN).permute(0, 3, 1, 2), b)
    y = ref.clone()
    y[64:128] = part[64:128]
    _judge("one split's partial missing for one tile", y, ref)


def test_dropped_cross_term_of_the_split_product_is_rejected():
    """a . w from split operands (a = ah + al, w = wh + wl; f16 halves rounded toward zero) without the al . wh term: about 2^-12"""
    x, w, b = _operands(3)
    ref = _ref(x, w, b)
    ah = PI._rtz_f16(x).to(F64)
    wh = PI._rtz_f16(w).to(F64)
    wl = PI._rtz_f16((w.to(F64) - wh).float()).to(F64)
    y = _rows(F.conv2d(ah, wh, b.to(F64), stride=S2, padding=1) + F.conv2d(ah, wl, None, stride=S2, padding=1))
    _judge("al.wh cross term dropped", y, ref)


def test_tail_row_holding_the_previous_tiles_row_is_rejected():
    """M = 180 on 64-row tiles: one row of the ragged last tile (m = 150 >= 128) holds row m - 64"""
    x, w, b = _operands(4)
    ref = _ref(x, w, b)
    y = ref.clone()
    y[150] = ref[150 - 64]
    _judge("tail row from the previous tile", y, ref)


def test_pixel_metric_sees_what_the_whole_tensor_check_divides_away():
    """a low-magnitude row (1 % of the tensor's scale) that is 0.1 % off: 1e-5 of the tensor's largest value"""
    x, w, b = _operands(5)
    ref = _ref(x, w, b)
    ref[77] *= 0.01
    y = ref.clone()
    y[77] *= 1 + 1e-3
    assert _old_accepts(y, ref)
    assert _judge("low-magnitude row 0.1 % off", y, ref)

"""Which kernel `omni_launch_conv` picks, asked of the launcher itself (`omni_debug_conv_cfg`: the function the launch calls), without
a GPU: the set of instantiations the heuristic can ever reach, what the tile override i22 changes, and that the launcher names no
instantiation outside that set."""
import ctypes

import pytest

import conv_f64 as C
import gpu_checks as G
from omniparser_amd import _lib as L

TYPED_TILES = ((64, 64, 64, "generic"), (64, 64, 64, "aligned"), (64, 64, 64, "pointwise"), (64, 64, 128, "aligned"), (64, 64, 128, "pointwise"),
               (128, 64, 64, "generic"), (128, 64, 64, "aligned"), (128, 64, 64, "pointwise"),
               (128, 128, 64, "generic"), (128, 128, 64, "aligned"), (128, 128, 64, "pointwise"))
REACHABLE = {"f32": {("f32",) + t for t in TYPED_TILES}, "f16": {("f16",) + t for t in TYPED_TILES},
             "split": {("split", bm, bn, 128, ld) for bm, bn in ((64, 64), (128, 64), (128, 128)) for ld in ("aligned", "pointwise")}}


@pytest.mark.parametrize("fam", ["f32", "f16", "split"])
def test_heuristic_reaches_exactly_these_instantiations(fam):
    """M over 1 .. 2^20 x Cout x Cin x k x s x workspace: the unforced heuristic's reach.  128-row tiles never walk 128-byte K slices
    and a 128-byte slice never meets the generic loader — the instantiations that were compiled for them are gone (next test)."""
    seen = C.sweep(fam)
    print(fam, "reachable:", sorted(seen))
    assert seen == REACHABLE[fam], (sorted(seen - REACHABLE[fam]), sorted(REACHABLE[fam] - seen))
    assert not any(bm == 128 and rb == 128 for f, bm, bn, rb, ld in seen if f != "split")


def test_launcher_names_no_instantiation_outside_the_reachable_set():
    assert C.launcher_names() == {(bm, bn, rb) for bm, bn, rb, _ in TYPED_TILES} == {(64, 64, 128), (64, 64, 64), (128, 64, 64), (128, 128, 64)}


@pytest.mark.parametrize("fam", ["f32", "f16", "split"])
def test_tile_override_reaches_the_same_set_at_any_size(fam):
    """i22 = 1 / 2 / 3 gives exactly that tile for every shape of the sweep, the K-slice rule stays (128 rows -> 64 bytes), and
    the three codes together reach what the heuristic reaches — nothing more"""
    union = set()
    for tile, (bm, bn) in C.TILES.items():
        seen = C.sweep(fam, tile)
        assert {(i[1], i[2]) for i in seen} == {(bm, bn)}, (tile, sorted(seen))
        assert all(i[3] == 64 for i in seen if i[1] == 128 and fam != "split")
        union |= seen
    assert union == REACHABLE[fam]


def test_existing_conv_cases_land_where_they_always_did():
    """the (BM, BN, RB, loader) that gpu_checks.CONV_CASES reach on the register-staged kernel (i22 = 0): unchanged by the override"""
    f32 = {(64, 64, 64, "generic"), (64, 64, 128, "aligned"), (64, 64, 128, "pointwise"), (128, 64, 64, "pointwise"), (128, 128, 64, "aligned")}
    for fam, want in (("f32", f32), ("f16", f32 | {(64, 64, 64, "aligned")})):
        seen = set()
        for B, H, W, cin, cout, k, s, *_ in G.CONV_CASES:
            if cin % C.vec(fam):
                continue
            p = k // 2
            Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
            op = L.make_op(L.OP_CONV, L.F16 if fam == "f16" else L.F32, p=[256, 256, None, None, 256, 256],
                           i={0: B, 1: H, 2: W, 3: cin, 4: cin, 6: k, 7: k, 8: s, 9: p, 10: Ho, 11: Wo, 12: cout, 13: cout, 19: 32 * 1024})
            seen.add(C.inst(L.conv_cfg(op))[1:])
        assert seen == want, (fam, sorted(seen))


def test_detector_first_layer_takes_the_128x64_generic_kernel():
    """4 stored channels, 3x3 stride 2 at the benched 1088x1920 input (M = 522 240, Cout = 64), and the smallest square stride-1 image
    tests/test_gpu_s_conv_f64.py launches in its place"""
    op = L.make_op(L.OP_CONV, L.F32, p=[256, 256, None, None, 256, 256],
                   i={0: 1, 1: 1088, 2: 1920, 3: 4, 4: 4, 6: 3, 7: 3, 8: 2, 9: 1, 10: 544, 11: 960, 12: 64, 13: 64, 19: 32 * 1024})
    cfg = L.conv_cfg(op)
    assert C.inst(cfg) == ("f32", 128, 64, 64, "generic") and cfg["splits"] == 1 and cfg["waves"] == 4, cfg
    for side, want in ((361, (64, 64)), (362, (128, 64))):
        op = L.make_op(L.OP_CONV, L.F32, p=[256, 256, None, None, 256, 256],
                       i={0: 1, 1: side, 2: side, 3: 4, 4: 4, 6: 3, 7: 3, 8: 1, 9: 1, 10: side, 11: side, 12: 64, 13: 64, 19: 32 * 1024})
        assert C.inst(L.conv_cfg(op))[1:3] == want, side


def test_split_count_override_stays_split_only_and_modes_are_reported():
    op = C.cfg_op("f32", 180, 32, 40, 3, 2, ws=True, tile=1)
    base = L.conv_cfg(op)
    op.i[23] = 5
    assert L.conv_cfg(op) == base and base["reduce"] == "reduce_launch" and base["splits"] == 2, base       # i23 ignored when i20 = 0
    op = C.cfg_op("split", 180, 32, 40, 3, 2, ws=True, tile=3, splits=4)
    assert L.conv_cfg(op) == {"family": "split", "bm": 128, "bn": 128, "rb": 128, "loader": "aligned", "splits": 3, "reduce": "reduce_launch",
                              "waves": 8}
    op = C.cfg_op("split", 180, 32, 40, 3, 2, ws=True, tile=2, splits=4, cnt=64)
    cfg = L.conv_cfg(op)
    assert cfg["reduce"] == "in_launch_combine" and cfg["waves"] == 4, cfg
    op.i[24] = 1                                        # fewer counters than output tiles: the reduce launch
    assert L.conv_cfg(op)["reduce"] == "reduce_launch"
    op = C.cfg_op("split", 180, 32, 40, 3, 2, ws=False, tile=2, splits=4)
    assert L.conv_cfg(op)["splits"] == 1                # no workspace, no split


def test_bad_ops_are_errors_of_the_query_as_of_the_launch():
    for fam in ("f32", "split"):
        op = C.cfg_op(fam, 180, 32, 40, 3, 2, tile=4)
        out = (ctypes.c_int * 8)()
        assert L.lib().omni_debug_conv_cfg(ctypes.byref(op), out) == -1 and b"bad tile code 4" in L.lib().omni_last_error()
        assert L.lib().omni_op_launch(ctypes.byref(op), None) == -1 and b"bad tile code 4" in L.lib().omni_last_error()
    op = C.cfg_op("f32", 180, 32, 128, 1, 1)
    op.i[20] = 2
    with pytest.raises(L.OmniError):
        L.conv_cfg(op)
    op = C.cfg_op("f32", 180, 6, 40, 1, 1)
    with pytest.raises(L.OmniError, match="multiples of 4"):
        L.conv_cfg(op)

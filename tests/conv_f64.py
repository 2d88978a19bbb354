"""Convolution kernels (csrc/conv_igemm.hip) against a float64 convolution, inside guard bands, one launch per instantiation.

What `gpu_checks.check_conv` (ten shapes, one whole-tensor max|err| / max|ref|, operands in allocations of their own) does not see:
  * which kernel ran: every case names the instantiation it is meant for — (family, BM, BN, RB, loader) — and asserts through
    `omni_debug_conv_cfg` (the launcher's own choice) that it lands there; the tile is forced with OMNI_OP_CONV i22, so a few hundred
    rows reach the 128-row tiles the heuristic only takes at >= 1024 workgroups;
  * reads beyond an operand: input, weights, bias, residual, split-K workspace, arrival counters and output of a launch live in ONE
    allocation (`caption_f64.Arena`) whose guard bands and padding columns hold 0xFF bytes (NaN in f32 and f16); the input is a
    [B*H*W, ldi] matrix with ldi > Cin and in_coff > 0, residual and output have pitches and offsets of their own.  A padding tap, a
    ragged K vector or a tail row read from outside its extent reaches an accumulator as NaN.  (A read whose value is discarded
    cannot be seen this way.)
  * writes beyond an operand, missing writes: the output and the workspace are prefilled with 0xFF; afterwards every in-extent
    output element must have been written, every byte outside the extents (rows behind M, unused columns, guards) must still be
    0xFF and every input operand must hold what was uploaded;
  * local errors: the error is measured per output pixel (one row of Cout values, `seg_err`), so a defect confined to a border
    pixel, a tile's tail rows or a low-magnitude row is not divided by the tensor's largest value.
The reference is F.conv2d in float64 on the operands as the kernel sees them (rounded to f16 for f16 plans, split weights decoded from
the packed tensor), then activation and residual.  The whole-tensor tolerances of check_conv (2e-5 / 4e-3) are asserted on the same
outputs as well.

BOUNDS: worst `seg_err` per family over the forced-tile cases and the unforced large cases, measured on the MI355X -> bound, with a
margin of at most 8x for summation-order differences between tiles and splits.  Rows of ONE value (Cout = 1: the class head) have a
bound of their own: where the dot product cancels, the row's denominator is the floor (1e-2 of the tensor's largest value) and the
rounding of K products shows 10 - 30x larger than in a row of 40+ channels, whose largest value sets the scale; one bound for both
would hold the wide rows to the single-value rows' error.  [host emulation, forced-tile cases only, in brackets]
  family                                               rows of Cout >= 40             rows of Cout = 1
  f32    exact f32 MFMA (OMNI_CONV_SPLIT=0 plans)      1.44e-6 [5.9e-7] -> 8e-6       1.77e-5 [9.6e-6] -> 1e-4
  split  f32 activations x split-f16 weights (i20 = 1) 5.73e-7 [4.1e-7] -> 3e-6       1.22e-5 [9.1e-6] -> 7e-5
  f16    f16 plans                                     4.86e-4 [4.86e-4] -> 3 x 2^-10 4.76e-4 -> 3 x 2^-10   (the f16 rounding of the output
                                                                                      is half an f16 epsilon = 4.88e-4)
tests/test_conv_bounds_cpu.py shows that each bound accepts a float32 convolution / f16 operands with f32 accumulation and rejects five
plausible kernel defects."""
import math
import re
from pathlib import Path

import torch
import torch.nn.functional as F

from caption_f64 import FLOOR, Arena, seg_err, where  # noqa: F401  (shared, not copied)
from omniparser_amd import _lib as L
from omniparser_amd.planner import PlanBuilder

F64 = torch.float64
BOUNDS = {"f32": (8e-6, 1e-4), "split": (3e-6, 7e-5), "f16": (3 * 2.0 ** -10, 3 * 2.0 ** -10)}      # (Cout > 1, Cout = 1)
WHOLE_TOL = {"f32": 2e-5, "split": 2e-5, "f16": 4e-3}           # gpu_checks.check_conv's whole-tensor max|err| / max|ref|
N_CNT = 64                                                     # arrival counters handed to a combine launch
EMU_LIMIT = 2e8                                                # multiply-adds one case may cost the host emulation


def bound(fam, cout):
    return BOUNDS[fam][1 if cout == 1 else 0]


def vec(fam):
    return 8 if fam == "f16" else 4


def tdt(fam):
    return torch.float16 if fam == "f16" else torch.float32


def inst(cfg):
    """the kernel instantiation of a debug-query answer"""
    return (cfg["family"], cfg["bm"], cfg["bn"], cfg["rb"], cfg["loader"])


# ------------------------------------------------------------------------------------------------ cases
TILES = {1: (64, 64), 2: (128, 64), 3: (128, 128)}
# (B, H, W, k, s): M = B * Ho * Wo with pad = k // 2
S_3x3_S2 = (2, 19, 17, 3, 2)      # M = 180: full tile(s) + ragged tail, a tile straddles the image boundary (m = 90), odd H / W, stride 2
S_3x3_S1 = (1, 13, 11, 3, 1)      # M = 143: stride 1, all four borders
S_1x1_S2 = (2, 19, 17, 1, 2)      # M = 180: k = 1 but strided -> the conv loader with as few K slices as Cin gives
S_PW_A = (2, 9, 11, 1, 1)         # M = 198
S_PW_B = (1, 7, 19, 1, 1)         # M = 133


def _case(fam, tile, loader, rb, shape, cin, n, ws=False, splits=0, combine=False):
    """n: running number inside the instantiation — cycles Cout (40, BN + 8, 1), the activation and the residual"""
    bm, bn = TILES[tile]
    B, H, W, k, s = shape
    return dict(fam=fam, tile=tile, expect=(fam, bm, bn, rb, loader), B=B, H=H, W=W, k=k, s=s, Cin=cin, Cout=(40, bn + 8, 1)[n % 3],
                act=(L.ACT_SILU, L.ACT_GELU, L.ACT_NONE)[(n + n // 3) % 3], res=n % 2 == 1, ws=ws, splits=splits, combine=combine)


def typed_cases(fam):
    """register-staged kernel, f32 (V = 4) or f16 (V = 8): every reachable (BM, BN, RB, loader) with the tile forced by i22.
    A K slice holds RB / 16 vectors.  Per instantiation: 1, 2, 3 and >= 5 K slices where Cin allows them (a 64x64 tile takes 64-byte
    slices only when Cin is an ODD multiple of 4 V, so 2 slices of a pointwise layer do not exist there), Cout = 40 / BN + 8 / 1, three
    activations, residual on and off, and split-K launches with the reduce kernel where the heuristic produces them (workspace given,
    >= 8 K slices): the 3x3 aligned cases (9 slices -> 2 splits of 5 + 4) and the generic Cin = 6 V 3x3 case (14 slices -> 3 splits)."""
    V = vec(fam)
    out = []
    for tile, (bm, bn) in TILES.items():
        for rb in ((64, 128) if bm == 64 else (64,)):
            unit = (rb // 16) * V                                   # channels per K slice
            mult = (1, 3, 5) if (bm == 64 and rb == 64) else (1, 2, 3, 5)
            cs = [_case(fam, tile, "pointwise", rb, (S_PW_A, S_PW_B)[j % 2], m * unit, j) for j, m in enumerate(mult)]
            out += cs
            al = [_case(fam, tile, "aligned", rb, S_1x1_S2, m * unit, j) for j, m in enumerate(mult[:3])]
            n = len(al)
            al += [_case(fam, tile, "aligned", rb, S_3x3_S2, unit, n, ws=True), _case(fam, tile, "aligned", rb, S_3x3_S1, unit, n + 1),
                   _case(fam, tile, "aligned", rb, S_3x3_S1, unit, n + 2, ws=True)]
            out += al
            if rb == 64:
                out += [_case(fam, tile, "generic", rb, S_1x1_S2, V, 0),            # 1 ragged slice
                        _case(fam, tile, "generic", rb, S_1x1_S2, 6 * V, 1),        # 2 slices, the second half empty
                        _case(fam, tile, "generic", rb, S_3x3_S1, V, 2),            # 3 slices (K = 9 V)
                        _case(fam, tile, "generic", rb, S_3x3_S2, 2 * V, 3),        # 5 slices, ragged last one (K = 18 V)
                        _case(fam, tile, "generic", rb, S_3x3_S1, 6 * V, 4, ws=True),   # 14 slices -> split-K, reduce kernel
                        _case(fam, tile, "generic", rb, S_3x3_S2, 6 * V, 5)]
    return out


def split_cases():
    """split-f16 kernel (i20 = 1), all three tiles x both loaders, i22 / i23 forced: no split, the reduce launch and the in-launch
    combine, with K slices that do not divide by the split count (5 + 4, 2 + 1, 2 + 2 + 1)."""
    out = []
    for tile in TILES:
        c = lambda *a, **k: _case("split", tile, *a, **k)
        out += [c("pointwise", 128, S_PW_A, 32, 0, splits=1), c("pointwise", 128, S_PW_B, 64, 1, ws=True, splits=2),
                c("pointwise", 128, S_PW_A, 96, 2, ws=True, splits=2, combine=True), c("pointwise", 128, S_PW_B, 160, 3, ws=True, splits=3),
                c("pointwise", 128, S_PW_A, 160, 4, ws=True, splits=3, combine=True), c("pointwise", 128, S_PW_B, 160, 5, splits=1),
                c("aligned", 128, S_3x3_S2, 32, 0, splits=1), c("aligned", 128, S_3x3_S1, 32, 1, ws=True, splits=2),
                c("aligned", 128, S_3x3_S2, 32, 2, ws=True, splits=4, combine=True), c("aligned", 128, S_1x1_S2, 32, 3, splits=1),
                c("aligned", 128, S_1x1_S2, 64, 4, ws=True, splits=2, combine=True), c("aligned", 128, S_3x3_S1, 64, 5, ws=True, splits=5)]
    return out


def large_cases(fam):
    """the heuristic's own path (i22 = 0), one large case per 128-row tile, and (exact f32 only) the detector's first layer — 3x3 over
    4 stored channels — at the smallest square image at which the heuristic takes the 128x64 tile with the generic loader."""
    rb = 128 if fam == "split" else 64
    al = "aligned"
    big = [dict(fam=fam, tile=0, expect=(fam, 128, 64 if fam != "split" else 128, rb, "pointwise"), B=2, H=50, W=93, k=1, s=1, Cin=1024, Cout=1024,
                act=L.ACT_GELU, res=True, ws=True, splits=0, combine=False),
           dict(fam=fam, tile=0, expect=(fam, 128, 128, rb, al), B=1, H=95, W=97, k=3, s=1, Cin=64, Cout=2048,
                act=L.ACT_SILU, res=False, ws=True, splits=0, combine=False)]
    if fam == "f32":
        big.append(dict(fam=fam, tile=0, expect=(fam, 128, 64, 64, "generic"), B=1, H=362, W=362, k=3, s=1, Cin=4, Cout=64,
                        act=L.ACT_SILU, res=False, ws=True, splits=0, combine=False))
    return big


def case_cost(c):
    p = c["k"] // 2
    Ho, Wo = (c["H"] + 2 * p - c["k"]) // c["s"] + 1, (c["W"] + 2 * p - c["k"]) // c["s"] + 1
    return c["B"] * Ho * Wo * c["Cout"] * c["k"] * c["k"] * c["Cin"]


# ------------------------------------------------------------------------------------------------ one launch
def decode_split(wp, cout, K):
    """[Cout][K/16][16 hi | 16 lo] f16 -> f64 [Cout, K]: w = hi + lo * 2^-11 (what conv_split_kernel multiplies by)"""
    t = wp.view(cout, K // 16, 2, 16).to(F64)
    return (t[:, :, 0] + t[:, :, 1] / 2048.0).reshape(cout, K)


def reference(c, x, w2d, b, res):
    """f64 convolution of NCHW x with [Cout, K] weights (k = (r * kw + s) * Cin + c), then activation and residual -> [M, Cout]"""
    k, cin, cout = c["k"], c["Cin"], c["Cout"]
    w4 = w2d.view(cout, k, k, cin).permute(0, 3, 1, 2)
    ref = F.conv2d(x.to(F64), w4.to(F64), b.to(F64), stride=c["s"], padding=k // 2)
    if c["act"] == L.ACT_SILU:
        ref = F.silu(ref)
    elif c["act"] == L.ACT_GELU:
        ref = F.gelu(ref)
    ref = ref.permute(0, 2, 3, 1).reshape(-1, cout)
    return ref + res.to(F64) if res is not None else ref


def build_case(c, seed=0, dev=None):
    """operands of one case in one arena + the op + the f64 reference"""
    g = torch.Generator().manual_seed(seed)
    fam, V, t = c["fam"], vec(c["fam"]), tdt(c["fam"])
    B, H, W, k, s, cin, cout = c["B"], c["H"], c["W"], c["k"], c["s"], c["Cin"], c["Cout"]
    p = k // 2
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    M, K = B * Ho * Wo, k * k * cin
    x = torch.randn(B, cin, H, W, generator=g).to(t)
    w2d = (torch.randn(cout, K, generator=g) / math.sqrt(K))
    b = torch.randn(cout, generator=g)
    res = torch.randn(M, cout, generator=g).to(t) if c["res"] else None
    if fam == "split":
        wp = PlanBuilder.split_f16(w2d).view(cout, 2 * K)
        wref = decode_split(wp, cout, K)
    else:
        wp = w2d.to(t)
        wref = wp
    ldi, icoff = cin + 3 * V, 2 * V                  # vector loads: pitch and offset are multiples of V (the op requires it)
    ldr, rcoff = cout + 5, 3                         # scalar loads / stores: any pitch, any offset
    ldo, ocoff = cout + 2 * V + 3, V + 1
    ws_kib = 0
    if c["ws"]:
        # unforced cases: the product's 32 MiB; forced ones: room for the splits asked for (the heuristic of the typed kernels takes <= 3 here)
        ws_kib = 32 * 1024 if c["tile"] == 0 else (max(c["splits"], 4) * M * cout * 4 + 1023) // 1024
    ar = Arena()
    ar.add("x", t, B * H * W, ldi, data=((icoff, x.permute(0, 2, 3, 1).reshape(-1, cin)),))
    ar.add("w", wp.dtype, cout, wp.shape[1], data=((0, wp),))
    ar.add("b", torch.float32, 1, cout, data=((0, b.view(1, cout)),))
    if res is not None:
        ar.add("r", t, M, ldr, data=((rcoff, res),))
    if ws_kib:
        ar.add("ws", torch.float32, 1, ws_kib * 256, scratch=True)
    if c["combine"]:
        ar.add("cnt", torch.int32, 1, N_CNT, data=((0, torch.zeros(1, N_CNT, dtype=torch.int32)),))
    ar.add("y", t, M, ldo, out=((ocoff, cout),))
    ar.build(dev)
    op = L.make_op(L.OP_CONV, L.F16 if fam == "f16" else L.F32,
                   p=[ar.ptr("x"), ar.ptr("w"), ar.ptr("b"), ar.ptr("r") if res is not None else None, ar.ptr("y"),
                      ar.ptr("ws") if ws_kib else None, ar.ptr("cnt") if c["combine"] else None],
                   i={0: B, 1: H, 2: W, 3: cin, 4: ldi, 5: icoff, 6: k, 7: k, 8: s, 9: p, 10: Ho, 11: Wo, 12: cout, 13: ldo, 14: ocoff, 15: c["act"],
                      16: ldr if res is not None else 0, 17: rcoff if res is not None else 0, 19: ws_kib, 20: 1 if fam == "split" else 0,
                      22: c["tile"], 23: c["splits"] if fam == "split" else 0, 24: N_CNT if c["combine"] else 0})
    ins = {"x": (icoff, cin), "w": (0, wp.shape[1]), "b": (0, cout)}
    if res is not None:
        ins["r"] = (rcoff, cout)
    return ar, op, reference(c, x, wref, b, res), (ocoff, cout, (B, Ho, Wo)), ins


def _part(ar, host, name, off, cc):
    start, dt, rows, ld = ar.parts[name][:4]
    esz = torch.empty((), dtype=dt).element_size()
    return host[start:start + rows * ld * esz].view(dt).view(rows, ld)[:, off:off + cc].view({2: torch.int16, 4: torch.int32}[esz]).clone()


def _launch(ar, op, what, ins):
    """launch; nothing outside the extents changed, every output element written (Arena.fetch), every input operand unchanged"""
    import gpu_checks as G
    host = ar.dev.cpu()
    before = {n: _part(ar, host, n, off, cc) for n, (off, cc) in ins.items()}
    L.launch(op); G._sync()
    ar.fetch(what)
    for n, (off, cc) in ins.items():
        assert torch.equal(_part(ar, ar.host, n, off, cc), before[n]), f"{what}: input operand {n} was modified"


def run_case(c, seed=0, dev=None, check_bound=True):
    """one case: debug query == the instantiation the case names, launch inside guard bands, f64 reference per output pixel.
    Returns (worst pixel error, (b, ho, wo), whole-tensor error, config)."""
    ar, op, ref, (ocoff, cout, lead), ins = build_case(c, seed, dev)
    what = "conv " + describe(c)
    cfg = L.conv_cfg(op)
    assert inst(cfg) == c["expect"], f"{what}: lands on {inst(cfg)}, not on the instantiation it names"
    if c["fam"] == "split" and c["tile"]:
        want = "none" if c["splits"] == 1 else ("in_launch_combine" if c["combine"] else "reduce_launch")
        assert cfg["reduce"] == want and (c["splits"] == 1) == (cfg["splits"] == 1), f"{what}: {cfg}"
    elif c["tile"]:
        assert (cfg["reduce"] == "reduce_launch") == c["ws"], f"{what}: {cfg}"
    _launch(ar, op, what, ins)
    got = ar.get("y", ocoff, cout)
    if c["combine"]:
        # the in-launch combine leaves every counter zero, a second launch (a graph replay) gives the same bits, and so does the
        # reduce launch: the same partials summed in the same order
        assert int(ar.get("cnt", 0, N_CNT).abs().sum()) == 0, f"{what}: arrival counters not reset"
        _launch(ar, op, what + " (second combine launch)", ins)
        assert torch.equal(ar.get("y", ocoff, cout, raw=True), got.view(torch.int32)) and int(ar.get("cnt", 0, N_CNT).abs().sum()) == 0, \
            f"{what}: second combine launch differs"
        op.i[24] = 0
        assert L.conv_cfg(op)["reduce"] == "reduce_launch"
        _launch(ar, op, what + " (reduce launch)", ins)
        op.i[24] = N_CNT
        y2 = ar.get("y", ocoff, cout)
        assert torch.equal(y2.view(torch.int32), got.view(torch.int32)), \
            f"{what}: in-launch combine differs from the reduce launch in {int((y2 != got).sum())} values"
    e, i = seg_err(got, ref, cout)
    whole = float((got.to(F64) - ref).abs().max() / ref.abs().max())
    loc = where(i, lead)
    print(f"{what}: {inst(cfg)} splits {cfg['splits']} {cfg['reduce']}: pixel error {e:.2e} at {loc}, whole-tensor {whole:.2e}")
    if check_bound:
        bnd = bound(c["fam"], cout)
        assert e <= bnd, f"{what}: pixel {loc} is off by {e:.3e} of its own magnitude (bound {bnd:.1e}); {cfg}"
        assert whole < WHOLE_TOL[c["fam"]], f"{what}: whole-tensor error {whole:.3e}"
    return e, loc, whole, cfg


def describe(c):
    return (f"{c['fam']} tile {c['tile']} {c['B']}x{c['H']}x{c['W']} Cin {c['Cin']} Cout {c['Cout']} k{c['k']}s{c['s']} act {c['act']}"
            f"{' +res' if c['res'] else ''}{' ws' if c['ws'] else ''}{' splits ' + str(c['splits']) if c['splits'] else ''}"
            f"{' combine' if c['combine'] else ''}")


def run_cases(cases, seed=0, check_bound=True):
    """every case (no case is skipped); returns {"launched", "worst" / "worst_one": (error, case, location) over the rows of Cout > 1 /
    Cout = 1, "instantiations", "reduce"}"""
    out = {"launched": 0, "worst": (0.0, None, None), "worst_one": (0.0, None, None), "instantiations": set(), "reduce": set()}
    for n, c in enumerate(cases):
        e, loc, _, cfg = run_case(c, seed + n, check_bound=check_bound)
        out["launched"] += 1
        out["instantiations"].add(inst(cfg))
        out["reduce"].add(cfg["reduce"])
        if c["combine"]:
            out["reduce"].add("reduce_launch")
        key = "worst_one" if c["Cout"] == 1 else "worst"
        if e >= out[key][0]:
            out[key] = (e, describe(c), loc)
    return out


# ------------------------------------------------------------------------------------------------ the launcher's choice
SWEEP_M = sorted({m + d for e in range(0, 21) for m in (1 << e,) for d in (-1, 0, 1) if 1 <= m + d <= 1 << 20}
                 | {64 * n for n in (511, 512, 513, 767, 768, 769, 1023, 1024, 1025)} | {128 * n for n in (511, 512, 1023, 1024, 1025)}
                 | {100, 400, 1600, 6400, 9300, 25600, 102400, 131769, 522240})
SWEEP_COUT = (1, 40, 64, 65, 320, 2048)
SWEEP_CIN = (4, 8, 16, 24, 32, 48, 64, 256)


def cfg_op(fam, M, cin, cout, k, s, ws=True, tile=0, splits=0, cnt=0):
    """an op of M output pixels for the debug query alone (dummy non-NULL pointers: nothing is dereferenced): one image row"""
    Wi = M if s == 1 else 2 * M - 1
    return L.make_op(L.OP_CONV, L.F16 if fam == "f16" else L.F32, p=[256, 256, None, None, 256, 256 if ws else None, 256 if cnt else None],
                     i={0: 1, 1: 1, 2: Wi, 3: cin, 4: cin, 5: 0, 6: k, 7: k, 8: s, 9: k // 2, 10: 1, 11: M, 12: cout, 13: cout, 14: 0,
                        19: 32 * 1024 if ws else 0, 20: 1 if fam == "split" else 0, 22: tile, 23: splits, 24: cnt})


def sweep(fam, tile=0, with_cfg=False):
    """the instantiations `omni_launch_conv` can pick over M in 1 .. 2^20, Cout, Cin, k in {1, 3}, s in {1, 2}, with and without a
    workspace (tile = 0: the unforced heuristic)"""
    V = 32 if fam == "split" else vec(fam)
    seen = set()
    for cin in SWEEP_CIN:
        if cin % V:
            continue
        for cout in SWEEP_COUT:
            for k in (1, 3):
                for s in (1, 2):
                    for ws in (True, False):
                        op = cfg_op(fam, 1, cin, cout, k, s, ws, tile)
                        for M in SWEEP_M:
                            op.i[2], op.i[11] = (M if s == 1 else 2 * M - 1), M
                            cfg = L.conv_cfg(op)
                            seen.add((inst(cfg), cfg["reduce"], cfg["waves"]) if with_cfg else inst(cfg))
    return seen


def launcher_names():
    """the (BM, BN, RB) the register-staged launcher can name: the `launch_cfg<T, ...>` instantiations in the source"""
    src = (Path(L.__file__).resolve().parent / "csrc" / "conv_igemm.hip").read_text()
    return {tuple(map(int, m)) for m in re.findall(r"launch_cfg<T,\s*(\d+),\s*(\d+),\s*(\d+)>", src)}

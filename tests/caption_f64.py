"""Captioner kernels (csrc/caption_ops.hip) against float64 references, inside guard bands.

The references are the functions of tests/plan_interp.py that the CPU interpreter itself runs (in float32); here they run in float64 on
the host.  Three things a whole-tensor max-error check does not see are covered:
  * local errors: the error is measured per output row segment (one token, or one token x head / group) relative to that segment's own
    magnitude (`seg_err`), so a defect confined to one head, window or border pixel is not averaged away;
  * reads beyond an operand: every operand lives inside ONE allocation (`Arena`) whose guard bands and unused padding columns hold NaN
    (bytes 0xFF), so an out-of-extent read poisons the output; strided operands get pitches wider than their data and nonzero offsets;
  * writes beyond an operand and missing writes: outputs are prefilled with the same 0xFF pattern; afterwards every in-extent output
    element must have been written and every byte outside the extents must still be 0xFF.
The bounds (`BOUNDS`) come from the worst segment error measured on the MI355X over each family's cases, with a margin of at most 8x; the
negative controls in tests/test_caption_bounds_cpu.py show that each bound rejects a plausible kernel defect and accepts the f32
interpreter."""
import math

import numpy as np
import torch

import plan_interp as PI
from omniparser_amd import _lib as L
from plan_interp import split_decode

F64 = torch.float64
GUARD = 1024                    # bytes of 0xFF before, between and after the operands
FLOOR = 1e-2                    # a segment's denominator is at least FLOOR x the tensor's largest |reference| value

# Bounds per (family, plan dtype): the worst segment error measured on the MI355X over the family's cases (both tiers; the host emulation
# measures the same numbers) times a margin of at most 8x.  f32 plans [measured worst -> bound]:
#   dwconv3 1.6e-7 -> 1e-6; dwconv3_ln 5.6e-7 -> 4e-6; layernorm 4.7e-7 -> 3e-6; proj_prep 7.7e-7 -> 4e-6; embed_step 7.2e-8 -> 5e-7;
#   window / MHA / rows / channel attention, O(1) scores 4.1e-6 -> 1e-5, sharp scores (spread >= 20) 1.3e-5 -> 5e-5;
#   decode attention O(1) 6.1e-7 -> 4e-6, sharp 1.9e-6 -> 1.5e-5;
#   layernorm rows at mean 1e3: 7.9e-5 -> 2e-4 — above the split arithmetic's 2e-6 because the f32 statistics cannot resolve the row
#   mean of a 1e3-offset row better than half an ulp of 1e3 (3e-5): the float32 interpreter shows 4e-5 on the same rows.
# f16 plans: every family measured <= 0.5 f16 epsilon (the rounding of the f16 output) -> 3 epsilons (2^-10 each).
F16_EPS = 2.0 ** -10
BOUNDS = {
    # family            f32 plans  f16 plans
    "dwconv3":          (1e-6, 3 * F16_EPS),
    "dwconv3_ln":       (4e-6, 3 * F16_EPS),
    "layernorm":        (3e-6, 3 * F16_EPS),
    "layernorm_1e3":    (2e-4, 3 * F16_EPS),
    "attention":        (1e-5, 3 * F16_EPS),
    "attention_sharp":  (5e-5, 3 * F16_EPS),
    "attn_decode":      (4e-6, 3 * F16_EPS),
    "attn_decode_sharp": (1.5e-5, 3 * F16_EPS),
    "proj_prep":        (4e-6, 3 * F16_EPS),
    "embed_step":       (5e-7, 3 * F16_EPS),
}


def bound(family, dtype):
    return BOUNDS[family][0 if dtype == L.F32 else 1]


def seg_err(y, ref, seg, floor=FLOOR):
    """worst per-segment error: y / ref flattened into rows of `seg` trailing elements; a row's error is max|y - ref| divided by
    max(max|ref| over the row, floor x max|ref| over the tensor).  Returns (error, flat segment index); NaN counts as infinite."""
    a = y.detach().to(F64).reshape(-1, seg)
    r = ref.detach().to(F64).reshape(-1, seg)
    den = r.abs().amax(1).clamp_min(floor * float(r.abs().max())).clamp_min(1e-300)
    e = (a - r).abs().amax(1) / den
    e = torch.where(torch.isnan(e) | torch.isnan(a).any(1), torch.full_like(e, math.inf), e)
    i = int(torch.argmax(e))
    return float(e[i]), i


def where(i, lead):
    """flat segment index -> its coordinates in the segment grid `lead` (e.g. (batch, token, head))."""
    return tuple(int(v) for v in np.unravel_index(i, lead))


# ------------------------------------------------------------------------------------------------ guard bands
class Arena:
    """All operands of one launch in ONE device allocation: guard | operand | guard | operand | ... | guard.  An operand is a
    [rows, ld] matrix of which only some column ranges are its extent; everything else (guards, padding columns) is 0xFF bytes — NaN
    in f32 and f16 — and must still be after the launch.  Output extents are prefilled with 0xFF too and must all be overwritten."""

    def __init__(self):
        self.parts = {}
        self.size = GUARD

    def add(self, name, dtype, rows, ld, data=(), out=(), scratch=False):
        """data: ((col_offset, tensor [rows, c]), ...) input columns; out: ((col_offset, c), ...) output columns;
        scratch: the whole [rows, ld] block may be written (workspaces)."""
        esz = torch.empty((), dtype=dtype).element_size()
        start = (self.size + 255) // 256 * 256
        self.parts[name] = (start, dtype, rows, ld, data, out, scratch)
        self.size = start + rows * ld * esz + GUARD
        return self

    def build(self, dev):
        import gpu_checks as G
        buf = torch.full((self.size,), 0xFF, dtype=torch.uint8)
        mask = torch.zeros(self.size, dtype=torch.bool)
        for start, dt, rows, ld, data, out, scratch in self.parts.values():
            esz = torch.empty((), dtype=dt).element_size()
            v = buf[start:start + rows * ld * esz].view(dt).view(rows, ld)
            mv = mask[start:start + rows * ld * esz].view(rows, ld, esz)
            for off, t in data:
                v[:, off:off + t.shape[1]] = t.reshape(rows, -1).to(dt)
                mv[:, off:off + t.shape[1]] = True
            for off, c in out:
                mv[:, off:off + c] = True
            if scratch:
                mv[:] = True
        self.mask = mask
        self.dev = buf.to(dev if dev is not None else G.DEV)
        return self

    def ptr(self, name, elem_off=0):
        start, dt = self.parts[name][:2]
        return self.dev.data_ptr() + start + elem_off * torch.empty((), dtype=dt).element_size()

    def fetch(self, what):
        """copy back; assert nothing outside the extents changed and every output element was written."""
        host = self.dev.cpu()
        bad = (host != 0xFF) & ~self.mask
        if bool(bad.any()):
            pos = int(torch.nonzero(bad)[0])
            owner = max(((s, n) for n, (s, *_) in self.parts.items() if s <= pos), default=(0, "leading guard"))
            raise AssertionError(f"{what}: byte {pos} outside every extent was written ({pos - owner[0]} bytes past the start of {owner[1]})")
        self.host = host
        for name, (start, dt, rows, ld, data, out, scratch) in self.parts.items():
            for off, c in out:
                raw = self.get(name, off, c, raw=True)
                unwritten = int((raw == -1).sum())
                assert unwritten == 0, f"{what}: {unwritten} elements of output {name} not written"
        return self

    def get(self, name, off, c, raw=False):
        start, dt, rows, ld = self.parts[name][:4]
        esz = torch.empty((), dtype=dt).element_size()
        v = self.host[start:start + rows * ld * esz].view(dt).view(rows, ld)[:, off:off + c]
        return v.view({2: torch.int16, 4: torch.int32}[esz]) if raw else v.clone()


# ------------------------------------------------------------------------------------------------ cases
# (family, params).  Scales: "unit" = randn inputs; "sharp" = attention scores spread over >= 20 (the softmax picks few keys);
# "offset" = LayerNorm rows with mean 1e3 and standard deviation 1.
# GPU tier: every caption-op signature of the captioner's plans at the benched 768x768 crops, 2 crops (florence.py::_CaptionPlans;
# tests/test_caption_bounds_cpu.py::test_gpu_tier_covers_every_benched_caption_op keeps this list in step with the plans).
B2 = 2
GPU_TIER = (
    [("dwconv3_ln", dict(B=B2, H=H, W=H, C=C, osplit=1, scale="unit")) for H, C in ((192, 128), (96, 256), (48, 512))]
    + [("dwconv3", dict(B=B2, H=24, W=24, C=1024, scale="unit"))]
    + [("layernorm", dict(rows=B2 * n, C=C, period=0, omode=om, scale=sc))
       for n, C, om in ((36864, 128, 0), (9216, 256, 0), (2304, 512, 0), (576, 1024, 1), (577, 768, 0), (585, 768, 2), (1, 768, 0))
       for sc in ("unit", "offset")]
    + [("layernorm", dict(rows=B2 * 585, C=768, period=585, omode=2, scale=sc)) for sc in ("unit", "offset")]
    + [("attn_window", dict(B=B2, H=H, heads=C // 32, D=32, osplit=os_, scale=sc))
       for H, C in ((192, 128), (96, 256), (48, 512), (24, 1024)) for os_ in (1, 0) for sc in ("unit", "sharp")]
    + [("chan_attn", dict(B=B2, N=N, G=G, chunk=1024, osplit=os_, scale=sc))
       for N, G in ((36864, 4), (9216, 8), (2304, 16), (576, 32)) for os_ in (1, 0) for sc in ("unit", "sharp")]
    + [("attn_mha", dict(B=B2, S=585, heads=12, D=64, osplit=os_, scale=sc)) for os_ in (1, 0) for sc in ("unit", "sharp")]
    + [("proj_prep", dict(B=B2, N=576, C=1024, scale="unit")), ("assemble", dict(B=B2, n_img=577, n_txt=8, C=768))]
    + [("attn_decode_self", dict(B=B2, heads=12, cap=21, step=st, scale=sc)) for st in (0, 1, 10, 19) for sc in ("unit", "sharp")]
    + [("attn_decode_cross", dict(B=B2, heads=12, S=585, scale=sc)) for sc in ("unit", "sharp")]
    + [("embed_step", dict(B=B2, C=768, V=51290, T=21, off=2, step=7, scale="unit"))]
    + [("greedy_step", dict(B=4, V=51290, T=21, step=st)) for st in (0, 5, 19)]
)

# Emulated tier: reduced shapes that reach every launcher branch of csrc/caption_ops.hip (run on the host emulation and, cheaply, on
# the GPU).  Branch -> case that reaches it (f32 / f16 = plan dtype):
#   dwconv3        strip kernel (power-of-two vectors per pixel)           dwconv3 C=128 (f32, f16)
#                  point kernel                                             dwconv3 C=96 (f32), C=24 (f16)
#   dwconv3_ln     dwln_strip_kernel<1,32> / <1,64> / <2,64>, osplit 0 / 1  dwconv3_ln f32 C=128 / 256 / 512, osplit 0 and 1
#                  one wave per pixel (dwconv3_ln_kernel)                   dwconv3_ln f32 C=1024, f16 C=128
#   layernorm      layernorm_f32v4_kernel<NIT,LPR,omode>: (1,32) (1,64)     layernorm f32 C=128 / 256 / 512 / 768 / 1024
#                  (2,64) (3,64) (4,64) x omode 0 / 1 / 2                   x omode 0 / 1 / 2
#                  layernorm_kernel<T,NIT> (generic typed)                  layernorm f32 C=102 (C % 4 != 0), f16 C=768
#   attn_rows      window_attn_mfma_f32_kernel / window_attn_mfma_kernel    attn_window f32 / f16 (heads 1, 4, 8, 16, 32)
#                  mha_mfma_f32_kernel / mha_mfma_kernel                    attn_mha f32 / f16
#                  attn_rows_kernel<T,32> / <T,64>                          attn_rows D=32 (mode 0), D=64 (mode 1)
#   chan_attn      chan_scores_mfma + chan_softmax + chan_apply_mfma_split  chan_attn f32 chunk=1024 (G 4, 8, 16, 32)
#                  chan_scores_kernel + chan_apply_kernel (scalar)          chan_attn f32 chunk=1001, f16
#   attn_decode    attn_decode_cross_kernel                                 attn_decode_cross f32
#                  attn_decode_kernel (generic)                             attn_decode_self f32 / f16, attn_decode_cross f16 and
#                                                                           f32 with a misaligned pitch (ldc % 4 != 0)
#   greedy_step / embed_step / proj_prep / assemble (one kernel each)        greedy_step, embed_step, proj_prep, assemble
EMU_TIER = (
    [("dwconv3", dict(B=2, H=9, W=11, C=C, scale="unit")) for C in (128, 96)]
    + [("dwconv3_ln", dict(B=2, H=H, W=W, C=C, osplit=os_, scale="unit"))
       for (H, W, C) in ((7, 13, 128), (13, 5, 256), (5, 9, 512), (6, 7, 1024)) for os_ in (0, 1)]
    + [("layernorm", dict(rows=rows, C=C, period=0, omode=om, scale=sc))
       for rows, C in ((37, 128), (21, 256), (19, 512), (13, 768), (11, 1024)) for om in (0, 1, 2) for sc in ("unit", "offset")]
    + [("layernorm", dict(rows=18, C=768, period=6, omode=2, scale="offset")), ("layernorm", dict(rows=9, C=102, period=3, omode=0, scale="unit"))]
    + [("attn_window", dict(B=2, H=H, heads=heads, D=32, osplit=os_, scale=sc))
       for H, heads in ((13, 1), (16, 4), (12, 8), (24, 16), (14, 32)) for os_ in (0, 1) for sc in ("unit", "sharp")]
    + [("attn_mha", dict(B=2, S=S, heads=2, D=64, osplit=os_, scale=sc)) for S in (77, 130) for os_ in (0, 1) for sc in ("unit", "sharp")]
    + [("attn_rows", dict(B=2, S=37, heads=2, D=32, mode=0, scale="sharp")), ("attn_rows", dict(B=1, H=13, heads=2, D=64, mode=1, scale="unit"))]
    + [("chan_attn", dict(B=2, N=N, G=G, chunk=1024, osplit=os_, scale=sc))
       for N, G in ((2500, 4), (300, 8), (150, 16), (40, 32)) for os_ in (0, 1) for sc in ("unit", "sharp")]
    + [("chan_attn", dict(B=2, N=2100, G=4, chunk=1001, osplit=0, scale="sharp"))]
    + [("proj_prep", dict(B=2, N=36, C=256, scale="unit")), ("assemble", dict(B=2, n_img=5, n_txt=8, C=256))]
    + [("attn_decode_self", dict(B=3, heads=2, cap=21, step=st, scale=sc)) for st in (0, 1, 10, 19) for sc in ("unit", "sharp")]
    + [("attn_decode_cross", dict(B=3, heads=2, S=S, scale=sc, ldpad=pad)) for S in (130, 3) for pad in (64, 2) for sc in ("unit", "sharp")]
    + [("embed_step", dict(B=3, C=256, V=1000, T=21, off=2, step=7, scale="unit"))]
    + [("greedy_step", dict(B=4, V=3000, T=21, step=st)) for st in (0, 5, 19)]
)
F16_ONLY_EMU = [("dwconv3", dict(B=2, H=9, W=11, C=24, scale="unit"))]


def family_bound(family, prm, dtype):
    """the bound of a case: attention families share one (O(1) / sharp scores), LayerNorm rows at mean 1e3 have their own."""
    fam = {"attn_decode_self": "attn_decode", "attn_decode_cross": "attn_decode", "attn_window": "attention", "attn_mha": "attention",
           "attn_rows": "attention", "chan_attn": "attention"}.get(family, family)
    if prm.get("scale") == "sharp":
        fam += "_sharp"
    if fam == "layernorm" and prm.get("scale") == "offset":
        fam = "layernorm_1e3"
    return bound(fam, dtype)


def _valid(family, prm, dtype):
    """cases that exist for the plan dtype (split outputs are f32-plan formats; misaligned pitches only matter to the f32 kernels)."""
    if dtype != L.F32 and (prm.get("osplit") or prm.get("omode", 0) != 0 or prm.get("ldpad", 64) % 4):
        return False
    if family == "chan_attn" and dtype != L.F32 and prm["chunk"] != 1024:
        return False
    return True


def tier_cases(tier, dtype):
    cases = {"gpu": GPU_TIER, "emu": EMU_TIER + (F16_ONLY_EMU if dtype != L.F32 else [])}[tier]
    return [(f, p) for f, p in cases if _valid(f, p, dtype)]


# ------------------------------------------------------------------------------------------------ one case
def _tdt(dtype):
    return torch.float32 if dtype == L.F32 else torch.float16


def _rows_out(ar, name, off, C, split):
    t = ar.get(name, off, C)
    return split_decode(t.contiguous()) if split else t


def run_case(family, prm, dtype, seed=0, dev=None, check_bound=True):
    """launch one case inside guard bands; returns {output: (worst segment error, where)}.  Raises AssertionError on a guard / write
    failure, and (check_bound) when an error exceeds the family's bound."""
    g = torch.Generator().manual_seed(seed)
    tdt = _tdt(dtype)
    R = lambda *s: torch.randn(*s, generator=g)
    sc = prm.get("scale", "unit")
    sharp = 8.0 if sc == "sharp" else 1.0
    ar = Arena()
    errs = {}
    fam = family

    if fam == "dwconv3":
        B, H, W, C = prm["B"], prm["H"], prm["W"], prm["C"]
        x, w, b = R(B, H, W, C).to(tdt), (R(3, 3, C) * 0.3).to(tdt), R(C)
        ar.add("x", tdt, B * H * W, C, data=((0, x.view(-1, C)),)).add("w", tdt, 9, C, data=((0, w.view(9, C)),)).add("b", torch.float32, 1, C, data=((0, b.view(1, C)),))
        ar.add("y", tdt, B * H * W, C, out=((0, C),))
        op = lambda: L.make_op(L.OP_DWCONV3, dtype, p=[ar.ptr("x"), ar.ptr("w"), ar.ptr("b"), None, ar.ptr("y")], i={0: B, 1: H, 2: W, 3: C})
        ar.build(dev); L.launch(op()); _sync(); ar.fetch(fam)
        ref = PI.dwconv3_ref(x, w, b, F64)
        errs["y"] = (seg_err(ar.get("y", 0, C), ref, C), (B, H, W))
    elif fam == "dwconv3_ln":
        B, H, W, C, os_ = prm["B"], prm["H"], prm["W"], prm["C"], prm["osplit"]
        x, w, b, gg, be = R(B, H, W, C).to(tdt), (R(3, 3, C) * 0.3).to(tdt), R(C), R(C), R(C)
        for n, t in (("x", x.view(-1, C)), ("w", w.view(9, C))):
            ar.add(n, tdt, t.shape[0], C, data=((0, t),))
        for n, t in (("b", b), ("g", gg), ("be", be)):
            ar.add(n, torch.float32, 1, C, data=((0, t.view(1, C)),))
        ar.add("y1", tdt, B * H * W, C, out=((0, C),)).add("h", tdt, B * H * W, C, out=((0, C),))
        ar.build(dev)
        L.launch(L.make_op(L.OP_DWCONV3_LN, dtype, p=[ar.ptr("x"), ar.ptr("w"), ar.ptr("b"), ar.ptr("h"), ar.ptr("y1"), ar.ptr("g"), ar.ptr("be")],
                           i={0: B, 1: H, 2: W, 3: C, 6: os_}, f={0: 1e-5}))
        _sync(); ar.fetch(fam)
        y1r, hr = PI.dwconv3_ln_ref(x, w, b, gg, be, 1e-5, F64)
        errs["y1"] = (seg_err(ar.get("y1", 0, C), PI.dwconv3_ref(x, w, b, F64), C), (B, H, W))
        errs["h"] = (seg_err(_rows_out(ar, "h", 0, C, os_), hr, C), (B, H, W))
    elif fam == "layernorm":
        rows, C, period, om = prm["rows"], prm["C"], prm["period"], prm["omode"]
        x = R(rows, C) + (1e3 if sc == "offset" else 0.0)
        x = x.to(tdt)
        add = R(period, C).to(tdt) if period else None
        gg, b = R(C), R(C)
        ar.add("x", tdt, rows, C, data=((0, x),))
        if add is not None:
            ar.add("add", tdt, period, C, data=((0, add),))
        ar.add("g", torch.float32, 1, C, data=((0, gg.view(1, C)),)).add("b", torch.float32, 1, C, data=((0, b.view(1, C)),))
        ar.add("y", tdt, rows, C, out=((0, C),))
        if om == 2:
            ar.add("y2", tdt, rows, C, out=((0, C),))
        ar.build(dev)
        L.launch(L.make_op(L.OP_LAYERNORM, dtype, p=[ar.ptr("x"), ar.ptr("add") if add is not None else None, ar.ptr("g"), ar.ptr("b"), ar.ptr("y"),
                                                    ar.ptr("y2") if om == 2 else None],
                           i={0: rows, 1: 1, 3: C, 5: period, 6: om}, f={0: 1e-5}))
        _sync(); ar.fetch(fam)
        ref = PI.layernorm_ref(x, add, gg, b, 1e-5, F64)
        errs["y"] = (seg_err(_rows_out(ar, "y", 0, C, om == 1), ref, C), (rows,))
        if om == 2:
            errs["y2"] = (seg_err(_rows_out(ar, "y2", 0, C, True), ref, C), (rows,))
    elif fam in ("attn_window", "attn_mha", "attn_rows"):
        heads, D = prm["heads"], prm["D"]
        C = heads * D
        mode = 1 if fam == "attn_window" else (0 if fam == "attn_mha" else prm["mode"])
        os_ = prm.get("osplit", 0)
        if mode == 1:
            B, H = prm["B"], prm["H"]
            W = H
            nw = ((H + 11) // 12) * ((W + 11) // 12)
            groups, nq, rows, lead = B * nw, 144, B * H * W, (B, H * W, heads)
        else:
            B, S = prm["B"], prm.get("S", 0)
            groups, nq, rows, lead = B, S, B * S, (B, S, heads)
        # pitches wider than the data, operands at nonzero offsets, NaN between them
        qoff, koff, voff, ld = 16, C + 32, 2 * C + 48, 3 * C + 64
        ooff, ldo = 16, C + 32
        q, k, v = R(rows, C) * sharp, R(rows, C), R(rows, C)
        q, k, v = q.to(tdt), k.to(tdt), v.to(tdt)
        kb, vb = R(C), R(C)
        ar.add("qkv", tdt, rows, ld, data=((qoff, q), (koff, k), (voff, v)))
        if mode == 1:
            ar.add("kb", torch.float32, 1, C, data=((0, kb.view(1, C)),)).add("vb", torch.float32, 1, C, data=((0, vb.view(1, C)),))
        ar.add("o", tdt, rows, ldo, out=((ooff, C),))
        ar.build(dev)
        L.launch(L.make_op(L.OP_ATTN_ROWS, dtype, p=[ar.ptr("qkv"), ar.ptr("qkv"), ar.ptr("qkv"), None, ar.ptr("o"),
                                                    ar.ptr("kb") if mode == 1 else None, ar.ptr("vb") if mode == 1 else None],
                           i={0: ld, 1: ld, 2: ld, 3: ldo, 4: qoff, 5: koff, 6: voff, 7: ooff, 8: heads, 9: nq, 10: nq, 11: groups, 12: mode,
                              13: H if mode == 1 else 0, 14: W if mode == 1 else 0, 15: D, 16: os_}, f={0: D ** -0.5}))
        _sync(); ar.fetch(fam)
        if mode == 1:
            ref = PI.attn_window_ref(*(t.view(B, H, W, C) for t in (q, k, v)), kb, vb, heads, D ** -0.5, F64)
        else:
            ref = PI.attn_plain_ref(*(t.view(B, S, C) for t in (q, k, v)), heads, D ** -0.5, F64)
        errs["o"] = (seg_err(_rows_out(ar, "o", ooff, C, os_), ref, D), lead)
    elif fam == "chan_attn":
        B, N, G, chunk, os_ = prm["B"], prm["N"], prm["G"], prm["chunk"], prm["osplit"]
        C = 32 * G
        qkv = R(B, N, 3, C)
        qkv[:, :, 0] *= sharp
        qkv = qkv.reshape(B * N, 3 * C).to(tdt)
        chunks = (N + chunk - 1) // chunk
        ar.add("qkv", tdt, B * N, 3 * C, data=((0, qkv),)).add("o", tdt, B * N, C, out=((0, C),))
        ar.add("ws", torch.float32, B * G * chunks, 1024, scratch=True)
        ar.build(dev)
        L.launch(L.make_op(L.OP_CHAN_ATTN, dtype, p=[ar.ptr("qkv"), None, None, None, ar.ptr("o"), ar.ptr("ws")],
                           i={0: B, 1: N, 3: C, 4: G, 5: chunk, 6: os_}))
        _sync(); ar.fetch(fam)
        ref = PI.chan_attn_ref(qkv.view(B, N, 3 * C), G, 0.0, F64)
        errs["o"] = (seg_err(_rows_out(ar, "o", 0, C, os_), ref, 32), (B, N, G))
    elif fam == "proj_prep":
        B, N, C = prm["B"], prm["N"], prm["C"]
        x, pos, tmp = R(B * N, C).to(tdt), R(N, C), R(C)
        ar.add("x", tdt, B * N, C, data=((0, x),)).add("pos", torch.float32, N, C, data=((0, pos),)).add("tmp", torch.float32, 1, C, data=((0, tmp.view(1, C)),))
        ar.add("y", tdt, B * (N + 1), C, out=((0, C),))
        ar.build(dev)
        L.launch(L.make_op(L.OP_PROJ_PREP, dtype, p=[ar.ptr("x"), ar.ptr("pos"), ar.ptr("tmp"), None, ar.ptr("y")], i={0: B, 1: N, 3: C}))
        _sync(); ar.fetch(fam)
        ref = PI.proj_prep_ref(x.view(B, N, C), pos, tmp, F64)
        errs["y"] = (seg_err(ar.get("y", 0, C), ref, C), (B, N + 1))
    elif fam == "assemble":
        B, ni, nt, C = prm["B"], prm["n_img"], prm["n_txt"], prm["C"]
        img, txt = R(B * ni, C).to(tdt), R(nt, C).to(tdt)
        ar.add("img", tdt, B * ni, C, data=((0, img),)).add("txt", tdt, nt, C, data=((0, txt),)).add("y", tdt, B * (ni + nt), C, out=((0, C),))
        ar.build(dev)
        L.launch(L.make_op(L.OP_ASSEMBLE, dtype, p=[ar.ptr("img"), ar.ptr("txt"), None, None, ar.ptr("y")], i={0: B, 1: ni, 2: nt, 3: C}))
        _sync(); ar.fetch(fam)
        want = torch.cat([img.view(B, ni, C), txt.unsqueeze(0).expand(B, nt, C)], 1).reshape(-1, C)
        assert torch.equal(ar.get("y", 0, C), want), "assemble"
        errs["y"] = ((0.0, 0), (B, ni + nt))
    elif fam in ("attn_decode_self", "attn_decode_cross"):
        B, heads = prm["B"], prm["heads"]
        C = heads * 64
        ldo = C + 32
        ar.add("o", tdt, B, ldo, out=((0, C),))
        if fam == "attn_decode_self":
            cap, st = prm["cap"], prm["step"]
            qoff, koff, voff, ldq = 16, C + 32, 2 * C + 48, 3 * C + 64
            ldc = C + 64
            q, kn, vn = (R(B, C) * sharp).to(tdt), R(B, C).to(tdt), R(B, C).to(tdt)
            kc, vc = R(B, cap, C), R(B, cap, C)
            kc[:, st:] = float("nan"); vc[:, st:] = float("nan")          # rows not yet appended: a read of them poisons the output
            kc, vc = kc.to(tdt), vc.to(tdt)
            ar.add("qkv", tdt, B, ldq, data=((qoff, q), (koff, kn), (voff, vn)))
            ar.add("kc", tdt, B * cap, ldc, data=((0, kc.view(-1, C)),)).add("vc", tdt, B * cap, ldc, data=((0, vc.view(-1, C)),))
            ar.add("step", torch.int32, 1, 1, data=((0, torch.tensor([[st]], dtype=torch.int32)),))
            ar.build(dev)
            L.launch(L.make_op(L.OP_ATTN_DECODE, dtype, p=[ar.ptr("qkv"), ar.ptr("qkv"), ar.ptr("qkv"), ar.ptr("kc"), ar.ptr("o"), ar.ptr("vc"), ar.ptr("step")],
                               i={0: ldq, 1: qoff, 2: ldq, 3: koff, 4: voff, 5: ldo, 6: heads, 7: 0, 8: cap, 9: C, 10: B, 11: ldc}, f={0: 0.125}))
            _sync(); ar.fetch(fam)
            ref = PI.attn_decode_self_ref(q, kc[:, :st], vc[:, :st], kn, vn, heads, 0.125, F64)
            kc2, vc2 = (ar.get(n, 0, C).view(B, cap, C) for n in ("kc", "vc"))
            assert torch.equal(kc2[:, st], kn) and torch.equal(vc2[:, st], vn), "attn_decode self: cache append"
            assert torch.equal(kc2[:, :st], kc[:, :st]) and torch.equal(vc2[:, :st], vc[:, :st]), "attn_decode self: cache rows changed"
        else:
            S, pad = prm["S"], prm.get("ldpad", 64)
            ldq, qoff = C + 32, 8
            ldc = 2 * C + pad
            q = (R(B, C) * sharp).to(tdt)
            kv = R(B * S, 2 * C).to(tdt)
            ar.add("q", tdt, B, ldq, data=((qoff, q),)).add("kv", tdt, B * S, ldc, data=((0, kv),))
            ar.build(dev)
            L.launch(L.make_op(L.OP_ATTN_DECODE, dtype, p=[ar.ptr("q"), None, None, ar.ptr("kv"), ar.ptr("o"), ar.ptr("kv", C), None],
                               i={0: ldq, 1: qoff, 5: ldo, 6: heads, 7: S, 8: S, 9: C, 10: B, 11: ldc}, f={0: 0.125}))
            _sync(); ar.fetch(fam)
            kv3 = kv.view(B, S, 2 * C)
            ref = PI.attn_decode_ref(q, kv3[..., :C], kv3[..., C:], heads, 0.125, F64)
        errs["o"] = (seg_err(ar.get("o", 0, C), ref, 64), (B, heads))
    elif fam == "embed_step":
        B, C, V, T, off, st = prm["B"], prm["C"], prm["V"], prm["T"], prm["off"], prm["step"]
        table, pos = R(V, C).to(tdt), R(T + off, C).to(tdt)
        ids = torch.randint(0, V, (B, T), generator=g, dtype=torch.int32)
        ids[0, st] = V - 1                                                  # the last row of the table
        ar.add("table", tdt, V, C, data=((0, table),)).add("pos", tdt, T + off, C, data=((0, pos),))
        ar.add("ids", torch.int32, B, T, data=((0, ids),)).add("step", torch.int32, 1, 1, data=((0, torch.tensor([[st]], dtype=torch.int32)),))
        ar.add("y", tdt, B, C, out=((0, C),))
        ar.build(dev)
        L.launch(L.make_op(L.OP_EMBED_STEP, dtype, p=[ar.ptr("table"), ar.ptr("pos"), ar.ptr("ids"), None, ar.ptr("y"), None, ar.ptr("step")],
                           i={0: B, 3: C, 4: T, 5: off}, f={0: 27.7128}))
        _sync(); ar.fetch(fam)
        ref = PI.embed_step_ref(table.reshape(-1), pos[st + off], ids[:, st].long(), C, 27.7128, F64)
        errs["y"] = (seg_err(ar.get("y", 0, C), ref, C), (B,))
    elif fam == "greedy_step":
        return _greedy_case(prm, dtype, g, dev)
    else:
        raise ValueError(fam)
    out = {}
    bnd = family_bound(fam, prm, dtype) if fam != "assemble" else 0.0
    for name, ((e, i), lead) in errs.items():
        out[name] = (e, where(i, lead))
        assert e <= bnd or not check_bound, f"{fam} {prm} {name}: worst segment error {e:.3e} at {where(i, lead)} > {bnd:.1e}"
    return out


def _sync():
    import gpu_checks as G
    G._sync()


def _greedy_case(prm, dtype, g, dev):
    """V-wide arg-max with the bias, the 3-gram ban, forced BOS / EOS, finished rows, exact ties in different threads' strides, a
    logits pitch wider than V (NaN beyond V)."""
    tdt = _tdt(dtype)
    B, V, T, st = prm["B"], prm["V"], prm["T"], prm["step"]
    ldl = V + 40
    logits = torch.randn(B, V, generator=g)
    bias = torch.randn(V, generator=g) * 0.01
    ids = torch.randint(3, V, (B, T), generator=g, dtype=torch.int32)
    ids[:, 0] = 2
    top = float((logits + bias).max()) + 1.0
    # row 0: the best token is banned by a repeated 3-gram (... a b X ... a b) -> the runner-up wins
    if st >= 4:
        a_, b_, x_ = 11, 12, 13
        ids[0, 1:4] = torch.tensor([a_, b_, x_], dtype=torch.int32); ids[0, st - 1:st + 1] = torch.tensor([a_, b_], dtype=torch.int32)
        logits[0, x_] = top + 5.0 - bias[x_]
    # row 1: an exact tie between index 7 and index 7 + 256 * 3 + 129 (different lanes and strides): the lower index wins
    for j in (7, 7 + 256 * 3 + 129):
        logits[1, j] = top + 1.0 - bias[7]; bias[j] = bias[7]
    # row 2: a tie between the first and the last index of the vocabulary (equal logits, equal biases: a tie in every precision)
    logits[2, 0] = logits[2, V - 1] = top + 2.0
    bias[V - 1] = bias[0]
    fin = torch.zeros(B, dtype=torch.int32)
    fin[B - 1] = 1
    lg = logits.to(tdt)
    ar = Arena()
    ar.add("logits", tdt, B, ldl, data=((0, lg),)).add("bias", torch.float32, 1, V, data=((0, bias.view(1, V)),))
    ar.add("ids", torch.int32, B, T, data=((0, ids),)).add("fin", torch.int32, 1, B, data=((0, fin.view(1, B)),))
    ar.add("step", torch.int32, 1, 1, data=((0, torch.tensor([[st]], dtype=torch.int32)),))
    ar.build(dev)
    L.launch(L.make_op(L.OP_GREEDY_STEP, dtype, p=[ar.ptr("logits"), ar.ptr("bias"), ar.ptr("ids"), ar.ptr("fin"), None, None, ar.ptr("step")],
                       i={0: B, 1: V, 2: ldl, 3: T, 4: 20, 5: 3, 6: 0, 7: 2, 8: 1, 9: 0, 10: 2, 11: 1}))
    _sync(); ar.fetch("greedy_step")
    ids_r, fin_r = ids.clone(), fin.clone()
    toks = PI.greedy_step_ref(lg, bias, ids_r, fin_r, st, 20, 3, 2, 1, 0, 2, F64)
    got = ar.get("ids", 0, T)
    assert torch.equal(got, ids_r), f"greedy_step step {st}: {got[:, st + 1].tolist()} vs {toks}"
    assert torch.equal(ar.get("fin", 0, B).view(-1), fin_r) and int(ar.get("step", 0, 1)) == st + 1, "greedy_step bookkeeping"
    if st not in (0, 19):
        assert toks[1] == 7 and toks[2] == 0, toks
    return {"ids": (0.0, ())}


def check_caption_f64(dtype=L.F32, tier="emu", families=None, seed=0):
    """every case of a tier: guard bands + f64 reference + bound.  Returns {family: (worst error, case, output, location)}."""
    worst = {}
    for n, (fam, prm) in enumerate(tier_cases(tier, dtype)):
        if families and fam not in families:
            continue
        res = run_case(fam, prm, dtype, seed=seed + n)
        key = fam + ("_1e3" if prm.get("scale") == "offset" else "")
        for name, (e, loc) in res.items():
            if key not in worst or e > worst[key][0]:
                worst[key] = (e, prm, name, loc)
    return worst


# ------------------------------------------------------------------------------------------------ plan signatures
def op_signature(op, B):
    """the dispatch-relevant shape of a caption op of a B-crop plan (None for the other kinds)."""
    i, k, dt = op.i, op.kind, op.dtype
    if k == L.OP_DWCONV3:
        return ("dwconv3", dt, i[1], i[2], i[3])
    if k == L.OP_DWCONV3_LN:
        return ("dwconv3_ln", dt, i[1], i[2], i[3], i[6])
    if k == L.OP_LAYERNORM:
        return ("layernorm", dt, i[0] * max(i[1], 1) // B, i[3], i[5], i[6])
    if k == L.OP_ATTN_ROWS:
        return ("attn_window", dt, i[13], i[8], i[15], i[16]) if i[12] == 1 else ("attn_mha", dt, i[9], i[8], i[15], i[16])
    if k == L.OP_CHAN_ATTN:
        return ("chan_attn", dt, i[1], i[4], i[5], i[6])
    if k == L.OP_PROJ_PREP:
        return ("proj_prep", dt, i[1], i[3])
    if k == L.OP_ASSEMBLE:
        return ("assemble", dt, i[1], i[2], i[3])
    if k == L.OP_ATTN_DECODE:
        return ("attn_decode_cross", dt, i[6], i[7]) if i[7] > 0 else ("attn_decode_self", dt, i[6], i[8])
    if k == L.OP_EMBED_STEP:
        return ("embed_step", dt, i[3], i[4], i[5])
    if k == L.OP_GREEDY_STEP:
        return ("greedy_step", dt, i[1], i[3], i[5], i[9], i[10])
    return None


def case_signature(fam, p, dtype=L.F32):
    """the same signature for a case of the tables above."""
    return {"dwconv3": lambda: (fam, dtype, p.get("H"), p.get("W"), p.get("C")),
            "dwconv3_ln": lambda: (fam, dtype, p.get("H"), p.get("W"), p.get("C"), p.get("osplit")),
            "layernorm": lambda: (fam, dtype, p["rows"] // B2, p["C"], p["period"], p["omode"]),
            "attn_window": lambda: (fam, dtype, p.get("H"), p["heads"], p["D"], p["osplit"]),
            "attn_mha": lambda: (fam, dtype, p.get("S"), p["heads"], p["D"], p["osplit"]),
            "attn_rows": lambda: None,
            "chan_attn": lambda: (fam, dtype, p["N"], p["G"], p["chunk"], p["osplit"]),
            "proj_prep": lambda: (fam, dtype, p["N"], p["C"]),
            "assemble": lambda: (fam, dtype, p["n_img"], p["n_txt"], p["C"]),
            "attn_decode_cross": lambda: (fam, dtype, p["heads"], p["S"]),
            "attn_decode_self": lambda: (fam, dtype, p["heads"], p["cap"]),
            "embed_step": lambda: (fam, dtype, p["C"], p["T"], p["off"]),
            "greedy_step": lambda: (fam, dtype, p["V"], p["T"], 3, 0, 2)}[fam]()

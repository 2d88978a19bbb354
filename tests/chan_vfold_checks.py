"""Checks of the channel block with Wv folded into the per-image projection as well (Florence2Captioner.fold_chan_v):
the per-image bias of the LDS-DMA GEMM, the bias table / scale product of OMNI_OP_CHAN_ATTN i11 = 1, the fold GEMM W'' = W' . Wv with
the re-pack behind it (OMNI_OP_SPLIT_CONVERT i6 = 1), and a channel block's tail in its three forms.  Shared by the host-emulation test
(tests/test_chan_vfold_emu_cpu.py) and the GPU test (tests/test_gpu_v_chan_vfold.py); device and synchronisation are those of
gpu_checks (which the emulation fixture redirects)."""
import math

import torch

import gpu_checks as G
from chan_fold_checks import _launch, _pack_images, _split_view
from omniparser_amd import _lib as L
from omniparser_amd.planner import PlanBuilder, View
from plan_interp import split_decode

SHAPES = ((128, 3, 512), (256, 3, 512), (512, 3, 512))     # (C, B, N): an image below the 256-row tile, exactly one tile, two tiles
GUARD = 64                                                 # floats of 7.0 behind every scratch tensor


def _guarded(n):
    return torch.full((n + GUARD,), 7.0, device=G.DEV)


def _guards_ok(t, sizes):
    return {k: bool((t[k][n:] == 7.0).all()) for k, n in sizes.items()}


def _scratch(B, C, N, partial=256):
    Gr = C // 32
    sizes = {"wf": B * C * C + B * C, "wb": B * C * C, "sc": B, "mx": B * (C // 64) * Gr}
    t = {k: _guarded(n) for k, n in sizes.items()}
    t["ws"] = torch.zeros(B * Gr * ((N + partial - 1) // partial) * 1024, device=G.DEV)
    return t, sizes


def _chan_op(t, qkv_ptr, w_ptr, B, N, C, vfold, have_scores=False, oscmul=0.0):
    """OMNI_OP_CHAN_ATTN in fold mode as the captioner's folded stages issue it (i5 = 1024, i10 = 256), with i11 = vfold"""
    return L.make_op(L.OP_CHAN_ATTN, L.F32,
                     p=[qkv_ptr, w_ptr, t["wf"].data_ptr(), t["wb"].data_ptr(), None, t["ws"].data_ptr(), t["sc"].data_ptr(), t["mx"].data_ptr()],
                     i={0: B, 1: N, 3: C, 4: C // 32, 5: 1024, 6: 1, 8: 1, 9: 1 if have_scores else 0, 10: 256, 11: vfold}, f={1: oscmul})


def _tilings(C):
    """(OMNI_GEMM_TILE, OMNI_GEMM_SCHED) a launch with C output channels can run on: the launcher's choice, both 256x256 schedules where that
    tile exists, and the other tiles an image of C rows is a whole number of"""
    t = [(None, None)]
    if C % 256 == 0:
        t += [("256x256", None), ("256x256", "1"), ("256x128", None)]
    return t + [("128x128", None)]


def check_bias_table_and_scale(seed=0, shapes=SHAPES):
    """OMNI_OP_CHAN_ATTN i11 = 1 over a real q|k (standalone scores, i9 = 0): W', its packed bytes and everything else as in fold mode
    (bit for bit the i11 = 0 op on the same inputs); the scale table holds split_f16_b's 2^-k times f1 exactly; the bias table
    b''[b][o] = sum_c W'[b][o][c] bv[c] + bp[o] lies within the bound of a C-term f32 chain, C * 2^-24 * sum_c |W'| |bv| per element, of the
    f64 value computed from the f32 W' the kernel stored (the chain bound check_fold states for W', extended to C terms).  Guard bands
    behind W' + table, the packed matrices, the scales and the block maxima stay untouched."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for C, B, N in shapes:
        qkv = torch.randn(B * N, 3 * C, generator=g)
        qkv[:, :2 * C] *= 1.5 / N ** 0.25
        wp = torch.randn(C, C, generator=g) / math.sqrt(C)
        wp[5] = 0.0                                           # a zero row of W': b'' = bp there, exactly
        bv, bp = torch.randn(C, generator=g) * 0.1, torch.randn(C, generator=g)
        qd = qkv.to(G.DEV)
        wcat = torch.cat([wp.reshape(-1), bv, bp]).to(G.DEV)
        t0, _ = _scratch(B, C, N)
        t1, sizes = _scratch(B, C, N)
        kv = 2.0 ** -9
        _launch([_chan_op(t0, qd.data_ptr(), wcat.data_ptr(), B, N, C, 0), _chan_op(t1, qd.data_ptr(), wcat.data_ptr(), B, N, C, 1, oscmul=kv)])
        n = B * C * C
        assert torch.equal(t0["wf"][:n], t1["wf"][:n]) and torch.equal(t0["wb"][:n], t1["wb"][:n]), f"i11 = 1 changed W' (C={C})"
        assert (t0["wf"][n:] == 7.0).all(), "i11 = 0 wrote a bias table"
        assert torch.equal(t0["sc"][:B].cpu() * kv, t1["sc"][:B].cpu()), f"scale table != 2^-k * f1 (C={C})"
        wf = t1["wf"][:n].cpu().view(B, C, C).double()
        got = t1["wf"][n:n + B * C].cpu().view(B, C).double()
        ref = wf @ bv.double() + bp.double()
        bound = C * 2.0 ** -24 * (wf.abs() @ bv.double().abs())
        excess = ((got - ref).abs() - bound).max().item()
        assert excess <= 0.0, f"bias table C={C}: |b'' - f64| exceeds the C-term chain bound by {excess:.3e}"
        assert torch.equal(got[:, 5], bp.double()[5].expand(B)), "zero row of W': b'' must be bp"
        gd = _guards_ok(t1, sizes)
        assert all(gd.values()), f"guard bands (C={C}): {gd}"
        out[C] = {"worst_fraction_of_bound": ((got - ref).abs() / bound.clamp_min(1e-300)).max().item()}
    return out


def check_fold_gemm(seed=0, shapes=SHAPES):
    """The fold GEMM W''_b = W'_b . Wv on gemm_dma (packed per-image matrices as the token operand, Wv^T as the shared weight, i26 = C,
    i27 = 0, the product 2^-k 2^-kv in the scale table) and the re-pack (OMNI_OP_SPLIT_CONVERT i6 = 1) on both sides of it.  Image 1 is all
    zeros (k = 0), image 2 is 2^10 larger than image 0; every tiling of `_tilings`.

    Bound of W'' against the f64 product of the SAME f32 inputs, per element, with S = sum_c |W'[o][c]| |Wv[c][k]|:
      * operands: an element x of a matrix scaled so that its largest magnitude lies in [2^12, 2^13) is stored as hi + lo with
        hi = f16(x), lo = f16(x - hi), both round-to-nearest: |x - hi| <= 2^-11 |x|, and lo keeps that to 2^-11 of itself while it is a
        normal f16 number, to half a subnormal step 2^-25 otherwise: |x - (hi + lo)| <= 2^-22 |x| + 2^-25 (a "22-bit operand").  Two such
        operands: 2 * 2^-22 * S, plus the floors e' * sum_c |Wv| + ev * sum_c |W'| with e' = 2^-25 2^-k, ev = 2^-25 2^-kv (unscaled);
      * products: the kernel adds hi.hi + lo.hi + hi.lo and drops lo.lo, |lo.lo| <= 2^-11 |x| * 2^-11 |y|: 2^-22 * S;
      * accumulation in f32 over the C terms, as check_fold's chain bound counts it (one rounding of the running sum per term, each at
        most 2^-24 of a partial sum that S bounds): C * 2^-24 * S; the final 2^-k 2^-kv is a power of two and exact.
    Sum: (3 * 2^-22 + C * 2^-24) * S + floors (first order; the second-order terms are below 2^-44 S).
    The packed bytes and scales behind the GEMM must be PlanBuilder.split_f16_b of the f32 W'' it wrote, bit for bit."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for C, B, N in shapes:
        Gr = C // 32
        w1 = torch.randn(B, C, C, generator=g) / math.sqrt(C)
        w1[1] = 0.0
        w1[2] *= 1024.0
        wv = torch.randn(C, C, generator=g) / math.sqrt(C)
        pb0 = PlanBuilder(G.DEV, L.F32)
        wvt = pb0.pack_weight_dma(wv.t().contiguous())
        S = w1.double().abs() @ wv.double().abs()
        ref = w1.double() @ wv.double()
        n = B * C * C
        for tile, sched in _tilings(C):
            t, sizes = _scratch(B, C, N)
            t["wf"][:n] = w1.reshape(-1).to(G.DEV)
            pbp = PlanBuilder(G.DEV, L.F32)
            pbp.repack_per_image(t["wf"], t["wb"], t["sc"], t["mx"], B, C)
            pack = pbp.ops[0]
            _launch([pack])
            sc1 = t["sc"][:B].cpu()
            for b in range(B):
                pk, osc = PlanBuilder.split_f16_b(w1[b])
                assert float(sc1[b]) == osc and torch.equal(t["wb"][b * C * C:(b + 1) * C * C].cpu().view(torch.uint8), pk.reshape(-1).view(torch.uint8)), \
                    f"re-pack of W' (C={C}, image {b})"
            t["sc"][:B] *= wvt.omni_oscale                    # what i11 = 1 leaves there (check_bias_table_and_scale)
            pb = PlanBuilder(G.DEV, L.F32)
            pb.fold_gemm(t["wb"], t["sc"], wvt, t["wf"], B, C)
            _launch(pb.ops, {"OMNI_GEMM_TILE": tile, "OMNI_GEMM_SCHED": sched})
            w2 = t["wf"][:n].cpu().view(B, C, C)
            floors = 2.0 ** -25 * (sc1.double().view(B, 1, 1) * wv.double().abs().sum(0).view(1, 1, C)
                                   + wvt.omni_oscale * w1.double().abs().sum(2, keepdim=True))
            bound = (3 * 2.0 ** -22 + C * 2.0 ** -24) * S + floors
            excess = ((w2.double() - ref).abs() - bound).max().item()
            worst = ((w2.double() - ref).abs() / bound.clamp_min(1e-300)).max().item()
            assert excess <= 0.0, f"fold GEMM C={C} {tile} sched {sched}: |W'' - f64| exceeds the bound by {excess:.3e}"
            assert not w2[1].any(), "zero image"
            assert (t["wf"][n:] == 7.0).all(), "fold GEMM wrote behind its matrices"
            _launch([pack])
            for b in range(B):
                pk, osc = PlanBuilder.split_f16_b(w2[b])
                assert float(t["sc"][b]) == osc, f"re-pack C={C} image {b}: 2^-k {float(t['sc'][b])} != {osc}"
                assert torch.equal(t["wb"][b * C * C:(b + 1) * C * C].cpu().view(torch.uint8), pk.reshape(-1).view(torch.uint8)), \
                    f"re-pack C={C} image {b} ({tile}, sched {sched}): packed bytes"
            gd = _guards_ok(t, sizes)
            assert all(gd.values()), f"guard bands (C={C}, {tile}): {gd}"
            out[(C, tile, sched)] = worst
    return out


def check_per_image_bias(seed=0, shapes=SHAPES):
    """OMNI_OP_CONV i29 = 1: the same bias vector in every image = the shared-bias launch bit for bit on every tiling; different biases
    per image against the f64 product image by image (rel 2e-6, check_gemm_per_image's bound); a per-image bias without per-image mode
    and a misaligned table come back as OMNI_E_ARG without a launch."""
    g = torch.Generator().manual_seed(seed)
    worst = 0.0
    for C, B, _ in shapes:
        rows, M = 256, B * 256
        x = torch.randn(M, C, generator=g) * 1.5
        ws = torch.randn(B, C, C, generator=g) / math.sqrt(C)
        ws[1] = 0.0
        ws[2] *= 1024.0
        bias = torch.randn(B, C, generator=g)
        res = torch.randn(M, C, generator=g)
        wb, sc = _pack_images(ws)
        for tile, sched in _tilings(C):
            pb = PlanBuilder(G.DEV, L.F32)
            xv = _split_view(pb, x, C, 0)
            wbd, scd = wb.to(G.DEV), sc.to(G.DEV)
            same = bias[0].repeat(B, 1).contiguous().to(G.DEV)
            o1, o2, o3 = (View(res.clone().view(1, M, 1, C).to(G.DEV), 0, C) for _ in range(3))
            pb.conv_per_image(xv, wbd, scd, same[0], o1, o1, rows)
            assert pb.ops[-1].i[29] == 0
            pb.conv_per_image(xv, wbd, scd, same, o2, o2, rows, bias_per_image=True)
            pb.conv_per_image(xv, wbd, scd, bias.to(G.DEV), o3, o3, rows, bias_per_image=True)
            _launch(pb.ops, {"OMNI_GEMM_TILE": tile, "OMNI_GEMM_SCHED": sched})
            assert torch.equal(o1.t.cpu(), o2.t.cpu()), f"one bias in every image != the shared-bias launch (C={C}, {tile}, sched {sched})"
            xd = split_decode(xv.t.view(M, C).cpu()).double()
            got = o3.t.view(M, C).cpu().double()
            for b in range(B):
                wd = split_decode(wb[b].view(C, C)).double() * float(sc[b])
                r0 = slice(b * rows, (b + 1) * rows)
                e = G.rel_err(got[r0], xd[r0] @ wd.t() + bias[b].double() + res[r0].double())
                assert e < 2e-6, f"per-image bias C={C} {tile} image {b}: rel err {e:.3e}"
                worst = max(worst, e)
    # ---- argument errors
    C, B, rows = 128, 2, 256
    pb = PlanBuilder(G.DEV, L.F32)
    xv = _split_view(pb, torch.randn(B * rows, C, generator=g), C, 0)
    wb, sc = _pack_images(torch.randn(B, C, C, generator=g))
    table = torch.zeros(B * C + 4, device=G.DEV)
    ov = View(torch.full((1, B * rows, 1, C), 7.0, device=G.DEV), 0, C)
    pb.conv_per_image(xv, wb.to(G.DEV), sc.to(G.DEV), table[:B * C], ov, None, rows, bias_per_image=True)
    _launch(pb.ops[:1])
    bad = []
    shared = pb.ops[1].i[26], pb.ops[1].i[27]
    for what in ("no per-image mode", "misaligned"):
        op = pb.ops[1]
        if what == "no per-image mode":
            op.i[26], op.i[27] = 0, 0
        else:
            op.i[26], op.i[27] = shared
            op.p[2] = table.data_ptr() + 4
        try:
            _launch([op])
        except L.OmniError as e:
            if "-1" in str(e).split(":")[0]:                  # OMNI_E_ARG
                bad.append(what)
    assert bad == ["no per-image mode", "misaligned"] and (ov.t == 7.0).all(), f"OMNI_E_ARG without a launch expected, got {bad}"
    return {"worst_rel_err": worst}


def check_block_tail(seed=0, shapes=SHAPES):
    """A channel block's tail B_ + proj(chan_attn(qkv(h))) on the same h, weights and residual in its three forms — today's ops, folded
    (v launch + per-image projection on v), folded with Wv (scores epilogue, softmax + fold + bias table, fold GEMM, re-pack, per-image
    projection on h with the per-image bias) — each within rel 3e-6 (max norm) of an f64 evaluation of its operands, the bound
    chan_fold_checks.check_composition holds the first two to.  In the third form qkv is NaN-filled and must stay untouched.
    Measured on the MI355X (C = 128 / 256 / 512): unfolded 1.2e-7 / 1.1e-7 / 1.4e-7, folded 7.6e-8 / 8.5e-8 / 1.3e-7, with Wv 7.1e-8 / 8.6e-8 / 1.0e-7."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for C, B, N in shapes:
        Gr, M = C // 32, B * N
        h = torch.randn(M, C, generator=g)
        wqkv = torch.randn(3 * C, C, generator=g) / math.sqrt(C)
        wqkv[:2 * C] *= 1.5 / N ** 0.25
        bqkv = torch.randn(3 * C, generator=g) * 0.1
        bqkv[:2 * C] *= 1.0 / N ** 0.25
        wproj = torch.randn(C, C, generator=g) / math.sqrt(C)
        bproj = torch.randn(C, generator=g)
        res = torch.randn(M, C, generator=g)
        pb = PlanBuilder(G.DEV, L.F32)
        hv = _split_view(pb, h, C, 0)
        wp = pb.pack_weight_dma(wqkv)
        wqk = pb.weight_rows(wp, 0, 2 * C)
        # ---- today's ops
        qkv1, att = pb.alloc(1, M, 1, 3 * C), pb.alloc(1, M, 1, C)
        o1 = View(res.clone().view(1, M, 1, C).to(G.DEV), 0, C)
        pb.conv(hv, wp, pb.upload(bqkv), qkv1, 1)
        ws1 = torch.zeros(B * Gr * 1024, device=G.DEV)
        pb.add_op(L.make_op(L.OP_CHAN_ATTN, L.F32, p=[qkv1.ptr, None, None, None, att.ptr, ws1.data_ptr()],
                            i={0: B, 1: N, 3: C, 4: Gr, 5: 1024, 6: 1}))
        att.fmt = "split"
        wpp, bpd = pb.pack_weight_dma(wproj), pb.upload(bproj)
        pb.conv(att, wpp, bpd, o1, 1, res=o1)
        # ---- folded (v launch)
        qkv2 = pb.alloc(1, M, 1, 3 * C)
        o2 = View(res.clone().view(1, M, 1, C).to(G.DEV), 0, C)
        pb.conv(hv, wqk, pb.upload(bqkv[:2 * C]), qkv2.slice(0, 2 * C), 1)
        vs = qkv2.slice(2 * C, C)
        pb.conv(hv, pb.weight_rows(wp, 2 * C, C), pb.upload(bqkv[2 * C:]), vs, 1, out_split=True)
        t2, _ = _scratch(B, C, N)
        wplain = pb.upload(wproj)
        pb.add_op(_chan_op(t2, qkv2.ptr, wplain.data_ptr(), B, N, C, 0))
        pb.conv_per_image(vs, t2["wb"], t2["sc"], bpd, o2, o2, N)
        # ---- folded with Wv
        qkv3 = torch.full((M, 3 * C), float("nan"), device=G.DEV)
        o3 = View(res.clone().view(1, M, 1, C).to(G.DEV), 0, C)
        t3, sizes = _scratch(B, C, N)
        wqs, bqs = pb.pack_weight_qk_groups(wqk), pb.upload(bqkv[:2 * C][pb.qk_group_rows(C)])
        pb.conv_scores(hv, wqs, bqs, t3["ws"], N)
        wvt = pb.pack_weight_dma(wqkv[2 * C:].t().contiguous())
        wcat = pb.upload(torch.cat([wproj.reshape(-1), bqkv[2 * C:], bproj]))
        pb.add_op(_chan_op(t3, qkv3.data_ptr(), wcat.data_ptr(), B, N, C, 1, have_scores=True, oscmul=wvt.omni_oscale))
        pb.fold_gemm(t3["wb"], t3["sc"], wvt, t3["wf"], B, C)
        pb.repack_per_image(t3["wf"], t3["wb"], t3["sc"], t3["mx"], B, C)
        pb.conv_per_image(hv, t3["wb"], t3["sc"], t3["wf"][B * C * C:B * C * C + B * C], o3, o3, N, bias_per_image=True)
        _launch(pb.ops)
        assert torch.isnan(qkv3).all(), f"the v-folded block wrote into qkv (C={C})"
        gd = _guards_ok(t3, sizes)
        assert all(gd.values()), f"guard bands (C={C}): {gd}"
        # ---- f64 evaluation of the operands
        hd = split_decode(hv.t.view(M, C).cpu()).double()
        wqd = split_decode(wp.cpu().view(torch.float32).view(3 * C, C)).double() * wp.omni_oscale
        qk = hd @ wqd[:2 * C].t() + bqkv[:2 * C].double()
        q, k = (qk[:, j * C:(j + 1) * C].view(B, N, Gr, 32) for j in range(2))
        A = torch.softmax(torch.einsum("bngi,bngj->bgij", q, k) / math.sqrt(N), -1)
        wpd = split_decode(wpp.cpu().view(torch.float32).view(C, C)).double() * wpp.omni_oscale
        errs = {}
        for name, o, wvd, wprd in (("unfolded", o1, wqd[2 * C:], wpd), ("folded", o2, wqd[2 * C:], wproj.double()),
                                   ("folded_v", o3, wqkv[2 * C:].double(), wproj.double())):
            v = (hd @ wvd.t() + bqkv[2 * C:].double()).view(B, N, Gr, 32)
            a64 = torch.einsum("bgij,bngj->bngi", A, v).reshape(M, C)
            errs[name] = G.rel_err(o.t.view(M, C).cpu().double(), a64 @ wprd.t() + bproj.double() + res.double())
        errs["folded_v_vs_folded"] = G.rel_err(o3.t.view(M, C).cpu().double(), o2.t.view(M, C).cpu().double())
        print(f"chan v-fold block tail C={C} B={B} N={N}: {errs}")
        for name in ("unfolded", "folded", "folded_v"):
            assert errs[name] < 3e-6, f"{name} channel block tail (C={C}, N={N}): rel err {errs[name]:.3e} vs f64"
        out[(C, B, N)] = errs
    return out

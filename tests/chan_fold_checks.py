"""Checks of the folded channel attention (DESIGN 3 "channel attention folded into its projection"): the LDS-DMA GEMM with one weight
matrix per image, the softmax + fold + pack kernels, and a channel block's tail computed both ways.  Shared by the host-emulation
test (tests/test_chan_fold_emu_cpu.py) and the GPU test (tests/test_gpu_r_chan_fold.py); the device and the synchronisation are those
of gpu_checks (which the emulation fixture redirects)."""
import math
import os

import torch

import gpu_checks as G
from omniparser_amd import _lib as L
from omniparser_amd.planner import PlanBuilder, View
from plan_interp import split_decode


def _launch(ops, env=None):
    env = {k: v for k, v in (env or {}).items() if v is not None}
    os.environ.update(env)
    try:
        for op in ops:
            L.launch(op)
        G._sync()
    finally:
        for k in env:
            os.environ.pop(k, None)


def _pack_images(ws):
    """[images, N, K] f32 -> (format-B bytes as f32-sized elements [images, N * K], 2^-k per image) by PlanBuilder.split_f16_b"""
    packs = [PlanBuilder.split_f16_b(w) for w in ws]
    wb = torch.stack([p[0].reshape(-1).view(torch.float32) for p in packs])
    return wb, torch.tensor([p[1] for p in packs], dtype=torch.float32)


def _split_view(pb, x, ld, coff):
    """x [M, K] as a format-B channel slice [coff, coff + K) of an [M, ld] buffer (garbage elsewhere)"""
    M, K = x.shape
    buf = torch.randn(M, ld)
    buf[:, coff:coff + K] = x
    v = View(buf.view(1, M, 1, ld).to(G.DEV), coff, K)
    pb.split_convert(v)
    return v


# (images, rows per image, K, N, residual, activation operand as the slice ld = 3K / coff = 2K, OMNI_GEMM_TILE, OMNI_GEMM_SCHED, weights)
# weights: "rand" | "scales" = image 0 all zeros, image 1 = 2^10 x the size of the others
PER_IMAGE_CASES = [
    (3, 256, 128, 128, False, False, None, None, "rand"),           # launcher's choice (128x128 here)
    (3, 256, 128, 128, True, True, "256x128", None, "rand"),        # ONE 256-row tile per image: adjacent tiles, different weights
    (3, 256, 128, 128, True, False, "128x128", None, "scales"),
    (3, 128, 128, 128, True, True, "128x128", None, "rand"),        # 128 rows per image on the 128-row tile
    (3, 512, 256, 256, True, True, "256x256", None, "rand"),        # ping-pong schedule
    (3, 512, 256, 256, False, False, "256x256", "1", "scales"),     # lockstep schedule
    (3, 512, 256, 256, True, False, "256x128", None, "scales"),
    (3, 512, 256, 256, False, True, "128x128", None, "rand"),
    (64, 128, 128, 256, True, True, "128x128", None, "rand"),       # 64 row tiles x 2 N tiles: the XCD tile order
]


def check_gemm_per_image(seed=0, cases=None):
    """OMNI_OP_CONV i20 = 2 with i26 / i27 / p6 vs the f64 product of the decoded operands, image by image (rel err < 2e-6, the bound
    of gpu_checks.check_gemm_dma); a per-image launch whose images all hold the SAME matrix equals the shared-weight launch (new fields
    zero) bit for bit; rows per image that are no whole number of tiles come back as an error."""
    g = torch.Generator().manual_seed(seed)
    worst, details = 0.0, []
    for case in (cases or PER_IMAGE_CASES):
        nimg, rows, K, N, use_res, sliced, tile, sched, wkind = case
        M = nimg * rows
        x = torch.randn(M, K, generator=g) * 1.5
        ws = torch.randn(nimg, N, K, generator=g) / math.sqrt(K)
        if wkind == "scales":
            ws[0] = 0.0
            ws[1] *= 1024.0
        b = torch.randn(N, generator=g)
        res = torch.randn(M, N, generator=g) if use_res else None
        pb = PlanBuilder(G.DEV, L.F32)
        xv = _split_view(pb, x, 3 * K, 2 * K) if sliced else _split_view(pb, x, K, 0)
        wb, sc = _pack_images(ws)
        wbd, scd, bd = wb.to(G.DEV), sc.to(G.DEV), b.to(G.DEV)
        ov = View(torch.full((1, M, 1, N + 16), 7.0, device=G.DEV), 16, N)
        rv = View(res.clone().view(1, M, 1, N).to(G.DEV), 0, N) if use_res else None
        pb.conv_per_image(xv, wbd, scd, bd, ov, rv, rows)
        _launch(pb.ops, {"OMNI_GEMM_TILE": tile, "OMNI_GEMM_SCHED": sched})
        xd = split_decode(xv.t.view(M, xv.ld).cpu()[:, xv.coff:xv.coff + K].contiguous()).double()
        full = ov.t.view(M, N + 16).cpu()
        assert (full[:, :16] == 7.0).all(), f"per-image gemm wrote outside its channel slice: {case}"
        got = full[:, 16:].double()
        for i in range(nimg):
            wd = split_decode(wb[i].view(N, K)).double() * float(sc[i])
            assert (wd - ws[i].double()).abs().max() <= 2.0 ** -21 * ws[i].abs().max()
            r0 = slice(i * rows, (i + 1) * rows)
            ref = xd[r0] @ wd.t() + b.double()
            if use_res:
                ref = ref + res[r0].double()
            e = G.rel_err(got[r0], ref)
            details.append((case, i, e))
            assert e < 2e-6, f"per-image gemm {case} image {i}: rel err {e:.3e} >= 2e-6"
            worst = max(worst, e)
    # ---- the new fields zero = the shared-weight launch; the same matrix in every image must give its bits
    same = {}
    for tile, sched in (("256x256", None), ("256x256", "1"), ("256x128", None), ("128x128", None)):
        nimg, rows, K, N = 2, 256, 128, 256
        M = nimg * rows
        x = torch.randn(M, K, generator=g)
        w = torch.randn(N, K, generator=g) / math.sqrt(K)
        b = torch.randn(N, generator=g)
        res = torch.randn(M, N, generator=g)
        pb = PlanBuilder(G.DEV, L.F32)
        xv = _split_view(pb, x, K, 0)
        wp = pb.pack_weight_dma(w)
        bd = pb.upload(b)
        o1 = View(res.clone().view(1, M, 1, N).to(G.DEV), 0, N)
        o2 = View(res.clone().view(1, M, 1, N).to(G.DEV), 0, N)
        pb.conv(xv, wp, bd, o1, 1, res=o1)
        assert pb.ops[-1].i[26] == 0 and pb.ops[-1].i[27] == 0 and not pb.ops[-1].p[6]
        wb, sc = _pack_images(w[None].repeat(nimg, 1, 1))
        pb.conv_per_image(xv, wb.to(G.DEV), sc.to(G.DEV), bd, o2, o2, rows)
        _launch(pb.ops, {"OMNI_GEMM_TILE": tile, "OMNI_GEMM_SCHED": sched})
        same[(tile, sched)] = bool(torch.equal(o1.t.cpu(), o2.t.cpu()))
        assert same[(tile, sched)], f"shared-weight launch and per-image launch of one matrix differ ({tile}, sched {sched})"
    # ---- rows per image that are no whole number of tiles: an error, never a launch
    pb = PlanBuilder(G.DEV, L.F32)
    xv = _split_view(pb, torch.randn(3 * 128, 128, generator=g), 128, 0)
    wb, sc = _pack_images(torch.randn(3, 128, 128, generator=g))
    ov = View(torch.full((1, 3 * 128, 1, 128), 7.0, device=G.DEV), 0, 128)
    pb.conv_per_image(xv, wb.to(G.DEV), sc.to(G.DEV), None, ov, None, 128)
    _launch(pb.ops[:1])
    refused = False
    try:
        _launch(pb.ops[1:], {"OMNI_GEMM_TILE": "256x128"})
    except L.OmniError as e:
        refused = "-1" in str(e).split(":")[0]                # OMNI_E_ARG
    assert refused and (ov.t == 7.0).all(), "rows_per_img % BM != 0 must come back as OMNI_E_ARG without a launch"
    return {"worst_rel_err": worst, "cases": len(details), "bitwise_same_matrix": same, "details": [(str(c), i, e) for c, i, e in details]}


def _chan_fold_op(qkv, wplain, B, N, C, att=None, chunk_tokens=1024):
    """fold-mode OMNI_OP_CHAN_ATTN over qkv [B * N, 3C] (device tensor) and its scratch: (op, dict of the scratch tensors)"""
    Gr = C // 32
    chunks = (N + chunk_tokens - 1) // chunk_tokens
    t = {"ws": torch.zeros(B * Gr * chunks * 1024, device=G.DEV), "wf": torch.zeros(B * C * C, device=G.DEV),
         "wb": torch.zeros(B * C * C, device=G.DEV), "sc": torch.zeros(B, device=G.DEV), "mx": torch.zeros(B * (C // 64) * Gr, device=G.DEV)}
    op = L.make_op(L.OP_CHAN_ATTN, L.F32,
                   p=[qkv.data_ptr(), wplain.data_ptr(), t["wf"].data_ptr(), t["wb"].data_ptr(), None, t["ws"].data_ptr(),
                      t["sc"].data_ptr(), t["mx"].data_ptr()],
                   i={0: B, 1: N, 3: C, 4: Gr, 5: chunk_tokens, 6: 1, 8: 1})
    t["chunks"] = chunks
    return op, t


def check_fold(seed=0, shapes=((128, 3, 96), (256, 3, 64))):
    """softmax + fold + pack: W'_b = Wp . blockdiag(A_g) against f64 within the bound of a 32-term f32 chain,
    32 * 2^-24 * sum_i |Wp[o][g32+i]| A_g[i][j] per element; the packed bytes and the scale table bit for bit against
    PlanBuilder.split_f16_b of the f32 W' the kernel stored."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for C, B, N in shapes:
        Gr = C // 32
        qkv = torch.randn(B * N, 3 * C, generator=g)
        qkv[:, :2 * C] *= 1.5 / N ** 0.25                    # logits q^T k / sqrt(N) of order 1: a softmax with structure
        wp = torch.randn(C, C, generator=g) / math.sqrt(C)
        wp[5] = 0.0
        qd, wd = qkv.to(G.DEV), wp.to(G.DEV)
        op, t = _chan_fold_op(qd, wd, B, N, C)
        _launch([op])
        A = t["ws"].cpu().view(B, Gr, t["chunks"], 32, 32)[:, :, 0]                   # softmax output, as the fold kernel read it
        assert torch.allclose(A.sum(-1), torch.ones(B, Gr, 32), atol=1e-5)
        s64 = torch.einsum("bngi,bngj->bgij", qkv[:, :C].double().view(B, N, Gr, 32), qkv[:, C:2 * C].double().view(B, N, Gr, 32)) / math.sqrt(N)
        assert (torch.softmax(s64, -1) - A.double()).abs().max() < 1e-5, "softmax of the scores"
        wf = t["wf"].cpu().view(B, C, C)
        wpg = wp.double().view(C, Gr, 32)
        ref = torch.einsum("ogi,bgij->bogj", wpg, A.double()).reshape(B, C, C)
        bound = 32 * 2.0 ** -24 * torch.einsum("ogi,bgij->bogj", wpg.abs(), A.double()).reshape(B, C, C)
        excess = ((wf.double() - ref).abs() - bound).max().item()
        assert excess <= 0.0, f"fold C={C}: |W' - f64| exceeds the 32-term chain bound by {excess:.3e}"
        worst = ((wf.double() - ref).abs() / bound.clamp_min(1e-300)).max().item()
        wb = t["wb"].cpu().view(B, C * C)
        sc = t["sc"].cpu()
        for b in range(B):
            pk, osc = PlanBuilder.split_f16_b(wf[b])
            assert float(sc[b]) == osc, f"fold C={C} image {b}: 2^-k {float(sc[b])} != {osc}"
            assert torch.equal(wb[b].view(torch.uint8), pk.reshape(-1).view(torch.uint8)), f"fold C={C} image {b}: packed bytes"
        out[C] = {"worst_fraction_of_bound": worst, "scales": sc.tolist()}
    # an all-zero matrix: k = 0, zero bytes
    C, B, N = 128, 2, 64
    qd, wd = torch.randn(B * N, 3 * C, generator=g).to(G.DEV), torch.zeros(C, C).to(G.DEV)
    op, t = _chan_fold_op(qd, wd, B, N, C)
    _launch([op])
    assert t["sc"].cpu().tolist() == [1.0, 1.0] and not t["wb"].cpu().view(torch.int32).any(), "all-zero W': k = 0"
    return out


def check_composition(seed=0, shapes=((512, 128, 3), (1024, 256, 2))):
    """a channel block's tail, B_ + proj(chan_attn(qkv(h))), as today's ops and folded, on the same h, weights and residual: each
    within rel 3e-6 of an f64 evaluation of its operands (check_mlp_fused's bound for 'same error class, different summation
    order'), the q|k slice of qkv bitwise equal between the two."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for N, C, B in shapes:
        Gr, M = C // 32, B * N
        h = torch.randn(M, C, generator=g)
        wqkv = torch.randn(3 * C, C, generator=g) / math.sqrt(C)
        wqkv[:2 * C] *= 1.5 / N ** 0.25                       # q, k rows scaled: softmax logits stay O(1), as the stand-in checkpoint does
        bqkv = torch.randn(3 * C, generator=g) * 0.1
        bqkv[:2 * C] *= 1.0 / N ** 0.25
        wproj = torch.randn(C, C, generator=g) / math.sqrt(C)
        bproj = torch.randn(C, generator=g)
        res = torch.randn(M, C, generator=g)
        pb = PlanBuilder(G.DEV, L.F32)
        hv = _split_view(pb, h, C, 0)
        wp = pb.pack_weight_dma(wqkv)
        bq = pb.upload(bqkv)
        # ---- today's ops
        qkv1 = pb.alloc(1, M, 1, 3 * C)
        att = pb.alloc(1, M, 1, C)
        o1 = View(res.clone().view(1, M, 1, C).to(G.DEV), 0, C)
        pb.conv(hv, wp, bq, qkv1, 1)
        ws1 = torch.zeros(B * Gr * 1024, device=G.DEV)
        pb.add_op(L.make_op(L.OP_CHAN_ATTN, L.F32, p=[qkv1.ptr, None, None, None, att.ptr, ws1.data_ptr()],
                            i={0: B, 1: N, 3: C, 4: Gr, 5: 1024, 6: 1}))
        att.fmt = "split"
        wpp, bpd = pb.pack_weight_dma(wproj), pb.upload(bproj)
        pb.conv(att, wpp, bpd, o1, 1, res=o1)
        # ---- folded
        qkv2 = pb.alloc(1, M, 1, 3 * C)
        o2 = View(res.clone().view(1, M, 1, C).to(G.DEV), 0, C)
        pb.conv(hv, pb.weight_rows(wp, 0, 2 * C), pb.upload(bqkv[:2 * C]), qkv2.slice(0, 2 * C), 1)
        vs = qkv2.slice(2 * C, C)
        pb.conv(hv, pb.weight_rows(wp, 2 * C, C), pb.upload(bqkv[2 * C:]), vs, 1, out_split=True)
        wplain = pb.upload(wproj)
        op, t = _chan_fold_op(qkv2.t, wplain, B, N, C)
        pb.add_op(op)
        pb.conv_per_image(vs, t["wb"], t["sc"], bpd, o2, o2, N)
        _launch(pb.ops)
        q1, q2 = qkv1.t.view(M, 3 * C).cpu(), qkv2.t.view(M, 3 * C).cpu()
        assert torch.equal(q1[:, :2 * C], q2[:, :2 * C]), f"q|k of the two compositions differ (N={N}, C={C})"
        # ---- f64 evaluation of the operands
        hd = split_decode(hv.t.view(M, C).cpu()).double()
        wqd = split_decode(wp.cpu().view(torch.float32).view(3 * C, C)).double() * wp.omni_oscale
        qkv = hd @ wqd.t() + bqkv.double()
        q, k, v = (qkv[:, j * C:(j + 1) * C].view(B, N, Gr, 32) for j in range(3))
        A = torch.softmax(torch.einsum("bngi,bngj->bgij", q, k) / math.sqrt(N), -1)
        a64 = torch.einsum("bgij,bngj->bngi", A, v).reshape(M, C)
        errs = {}
        for name, o, wpd in (("unfolded", o1, split_decode(wpp.cpu().view(torch.float32).view(C, C)).double() * wpp.omni_oscale),
                             ("folded", o2, wproj.double())):
            ref = a64 @ wpd.t() + bproj.double() + res.double()
            errs[name] = G.rel_err(o.t.view(M, C).cpu().double(), ref)
        print(f"chan fold composition N={N} C={C} B={B}: {errs}")
        for name, e in errs.items():
            assert e < 3e-6, f"{name} channel block tail (N={N}, C={C}): rel err {e:.3e} vs f64"
        out[(N, C, B)] = errs
    return out

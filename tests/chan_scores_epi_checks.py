"""Checks of the scores epilogue of the LDS-DMA GEMM (DESIGN 3d "scores in the q|k GEMM's epilogue"): OMNI_OP_CONV i20 = 2 with
i28 = 1 / p7 reduces the q|k tile to channel-attention score partials, OMNI_OP_CHAN_ATTN with i9 = 1 starts at the softmax.  Shared by
the host-emulation test (tests/test_chan_scores_epilogue_emu_cpu.py) and the GPU test (tests/test_gpu_u_chan_scores_epilogue.py); the
device and the synchronisation are those of gpu_checks (which the emulation fixture redirects)."""
import math

import torch

import gpu_checks as G
from chan_fold_checks import _chan_fold_op, _launch, _split_view
from omniparser_amd import _lib as L
from omniparser_amd.planner import PlanBuilder

GUARD = 2048            # floats behind the partials a launch may write
SENTINEL = -77.25


def _inputs(g, B, N, C, kind):
    """h [B * N, C], the q|k rows of a qkv weight [2C, C] and their bias; kind "scales": image 0 all zeros, image 1 scaled by 2^10"""
    h = torch.randn(B * N, C, generator=g)
    if kind == "scales":
        h[:N] = 0.0
        h[N:2 * N] *= 1024.0
    w = torch.randn(2 * C, C, generator=g) / math.sqrt(C)
    b = torch.randn(2 * C, generator=g) * 0.1
    return h, w, b


def _routes(h, w, b, B, N, C, sched):
    """both routes on the same input.  Returns (raw partials of the scores-mode launch, workspace of the standalone route after its
    op, workspace of the new route after its op, fold outputs of both) as CPU tensors; workspaces include the guard band."""
    Gr, M, chunks = C // 32, B * N, N // 256
    n_ws = B * Gr * chunks * 1024
    pb = PlanBuilder(G.DEV, L.F32)
    hv = _split_view(pb, h, C, 0)
    wp = pb.pack_weight_dma(w)                                   # UNpermuted q|k rows
    wplain = pb.upload(torch.eye(C))
    # ---- standalone route: plain q|k launch, then scores kernel + softmax + fold at chunk_tokens = 256
    qkv = pb.alloc(1, M, 1, 3 * C)
    qkv.t.zero_()
    pb.conv(hv, wp, pb.upload(b), qkv.slice(0, 2 * C), 1)
    op1, t1 = _chan_fold_op(qkv.t, wplain, B, N, C, chunk_tokens=256)
    assert t1["chunks"] == chunks
    pb.add_op(op1)
    n_old = len(pb.ops)
    # ---- new route: scores-mode launch on the permuted weight, then the op behind its scores
    ws2 = torch.full((n_ws + GUARD,), SENTINEL, device=G.DEV)
    pb.conv_scores(hv, pb.pack_weight_qk_groups(wp), pb.upload(b[PlanBuilder.qk_group_rows(C)]), ws2, N)
    env = {"OMNI_GEMM_SCHED": sched}
    _launch(pb.ops, env)
    raw = ws2.cpu().clone()
    op2, t2 = _chan_fold_op(qkv.t, wplain, B, N, C, chunk_tokens=256)
    op2.p[5] = ws2.data_ptr()
    op2.i[9] = 1
    _launch([op2], env)
    assert len(pb.ops) == n_old + 1
    fold1 = {k: t1[k].cpu() for k in ("wf", "wb", "sc")}
    fold2 = {k: t2[k].cpu() for k in ("wf", "wb", "sc")}
    return raw, t1["ws"].cpu(), ws2.cpu(), fold1, fold2, qkv.t.view(M, 3 * C).cpu()


def check_scores_bitwise(seed=0, widths=(128, 256), B=3, N=512):
    """ws of the scores-mode launch (permuted weight) against the ws the existing route produces on the same input (plain q|k launch on
    the unpermuted weight, OMNI_OP_CHAN_ATTN at chunk_tokens = 256), bit for bit, for both 256x256 schedules, random images and the
    zero / 2^10 pair.  The existing op's softmax overwrites the chunk-0 slot with A, so the comparison behind the ops is A plus the
    remaining chunk slots; the chunk-0 partial itself is pinned by a second run with every image's tokens rolled by 256 (the
    data of chunk 0 then sits in slot 1, which survives) — a tile's partial does not depend on where the tile lies.  The partials are
    also compared with an f64 evaluation of q|k (rel 1e-5: 256-term f32 sums), so that two equal but wrong results cannot pass."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for C in widths:
        Gr, chunks = C // 32, N // 256
        n_ws = B * Gr * chunks * 1024
        for kind in ("rand", "scales"):
            h, w, b = _inputs(g, B, N, C, kind)
            h_roll = h.view(B, N, C).roll(256, dims=1).reshape(B * N, C).contiguous()
            for sched in (None, "1"):
                raw, ws1, ws2, f1, f2, qkv = _routes(h, w, b, B, N, C, sched)
                assert (raw[n_ws:] == SENTINEL).all() and (ws2[n_ws:] == SENTINEL).all(), f"scores epilogue wrote beyond B*G*chunks partials (C={C})"
                assert torch.equal(ws1.view(torch.int32), ws2[:n_ws].view(torch.int32)), f"A / remaining partials differ (C={C}, {kind}, sched {sched})"
                for k in f1:
                    assert torch.equal(f1[k].view(torch.int32), f2[k].view(torch.int32)), f"fold output {k} differs (C={C}, {kind}, sched {sched})"
                # partials vs f64 of the q|k values the plain launch stored
                q = qkv[:, :C].double().view(B, chunks, 256, Gr, 32)
                k_ = qkv[:, C:2 * C].double().view(B, chunks, 256, Gr, 32)
                ref = torch.einsum("bctgi,bctgj->bgcij", q, k_)
                got = raw[:n_ws].double().view(B, Gr, chunks, 32, 32)
                for img in range(B):
                    e = G.rel_err(got[img], ref[img]) if ref[img].abs().max() > 0 else float(got[img].abs().max())
                    assert e < 1e-5, f"partials of image {img} vs f64: {e:.3e} (C={C}, {kind}, sched {sched})"
                # chunk 0: the rolled run carries its data in slot 1
                raw_r, ws1_r, ws2_r, _, _, _ = _routes(h_roll, w, b, B, N, C, sched)
                assert torch.equal(ws1_r.view(torch.int32), ws2_r[:n_ws].view(torch.int32))
                rr = raw_r[:n_ws].view(B, Gr, chunks, 1024)
                r0 = raw[:n_ws].view(B, Gr, chunks, 1024)
                assert torch.equal(rr[:, :, 1].view(torch.int32), r0[:, :, 0].view(torch.int32)), "a tile's partial depends on its position"
                assert torch.equal(ws1_r.view(B, Gr, chunks, 1024)[:, :, 1].view(torch.int32), r0[:, :, 0].view(torch.int32)), \
                    f"chunk-0 partial differs from the standalone scores kernel (C={C}, {kind}, sched {sched})"
                out[(C, kind, sched)] = True
    return out


def _scores_op(g, B=2, N=256, C=128):
    """a valid scores-mode op and what it points to"""
    h, w, b = _inputs(g, B, N, C, "rand")
    pb = PlanBuilder(G.DEV, L.F32)
    hv = _split_view(pb, h, C, 0)
    ws = torch.full((B * (C // 32) * (N // 256) * 1024 + GUARD,), SENTINEL, device=G.DEV)
    pb.conv_scores(hv, pb.pack_weight_qk_groups(pb.pack_weight_dma(w)), pb.upload(b), ws, N)
    pb.keep.append(hv.t)                                         # the caller holds `pb`: the input lives as long as the op is used
    _launch(pb.ops[:1])                                          # split_convert of the input
    return pb, pb.ops[1], ws


def check_y_not_written(seed=1):
    """p4 = NULL is accepted; a NaN-filled buffer passed as p4 is all NaN afterwards; the workspace behind B*G*chunks partials is untouched"""
    g = torch.Generator().manual_seed(seed)
    B, N, C = 2, 256, 128
    pb, op, ws = _scores_op(g, B, N, C)
    assert not op.p[4]
    _launch([op])
    first = ws.cpu().clone()
    n_ws = B * (C // 32) * (N // 256) * 1024
    assert (first[n_ws:] == SENTINEL).all() and not (first[:n_ws] == SENTINEL).any()
    y = torch.full((B * N, 2 * C), float("nan"), device=G.DEV)
    ws.fill_(SENTINEL)
    op.p[4] = y.data_ptr()
    _launch([op])
    assert torch.isnan(y.cpu()).all(), "the scores-mode launch wrote to p4"
    second = ws.cpu()
    assert torch.equal(first.view(torch.int32), second.view(torch.int32))
    return True


def check_argument_errors(seed=2):
    """each of these comes back as OMNI_E_ARG, never as a launch: rows per image 0, rows per image % 256 != 0, N % 256 != 0, an activation,
    a residual, format-B output, ws = NULL"""
    g = torch.Generator().manual_seed(seed)
    B, N, C = 2, 256, 128
    res = torch.zeros(B * N, 2 * C, device=G.DEV)
    y = torch.zeros(B * N, 2 * C, device=G.DEV)

    def rows0(op): op.i[26] = 0
    def rows128(op): op.i[26] = 128
    def n128(op): op.i[12] = 128; op.i[13] = 128
    def act(op): op.i[15] = L.ACT_GELU
    def residual(op): op.p[3] = res.data_ptr(); op.i[16] = 2 * C
    def osplit(op): op.i[21] = 1; op.p[4] = y.data_ptr()
    def nows(op): op.p[7] = None

    refused = {}
    for mutate in (rows0, rows128, n128, act, residual, osplit, nows):
        pb, op, ws = _scores_op(g, B, N, C)
        mutate(op)
        ok = False
        try:
            _launch([op])
        except L.OmniError as e:
            ok = "-1" in str(e).split(":")[0]                    # OMNI_E_ARG
        assert ok, f"{mutate.__name__}: expected OMNI_E_ARG"
        assert (ws.cpu() == SENTINEL).all(), f"{mutate.__name__}: the refused launch wrote partials"
        refused[mutate.__name__] = True
    return refused


def _seq_sum(p):
    """float32 sum over dim 0 in ascending order, one add per step"""
    s = torch.zeros_like(p[0])
    for c in range(p.shape[0]):
        s = s + p[c]
    return s


def check_softmax_order(seed=3, chunk_counts=(1, 2, 9, 144)):
    """chan_softmax_kernel sums the partials of an element in ascending chunk order.  The kernel's only output is A = softmax(scale * sum),
    so the sum is read through A: the partials are large cancelling terms (+-2^22-sized, every add rounds at 0.25 - 1) plus O(1) terms,
    the logits of the float32 sum in ascending order are O(1), and any other order moves most logits by a sizeable fraction of 1.
    A must equal the f64 softmax of the CPU float32 sum in ascending order within 1e-5 (expf and the normalisation, as in
    chan_fold_checks.check_fold); for 9 and 144 chunks the test also shows that the reversed and the 8-strided orders miss that bound by
    far on this data, so a changed order cannot pass.  Never compared with the kernel's own earlier output."""
    g = torch.Generator().manual_seed(seed)
    B, C = 2, 64
    Gr = C // 32
    out = {}
    for chunks in chunk_counts:
        N = 256 * chunks
        d = torch.randn(chunks + 1, B, Gr, 32, 32, generator=g) * 2.0 ** 22
        d[0] = 0.0
        d[-1] = 0.0
        p = ((d[1:] - d[:-1]) + torch.randn(chunks, B, Gr, 32, 32, generator=g) * (2.0 / math.sqrt(chunks))).float()
        ws = p.permute(1, 2, 0, 3, 4).clone().contiguous().to(G.DEV)     # (a copy: the op overwrites the chunk-0 slots with A)
        qkv = torch.empty(B * N, 3 * C, device=G.DEV)            # p0 of the op: not read behind the scores
        wplain = torch.eye(C, device=G.DEV)
        op, t = _chan_fold_op(qkv, wplain, B, N, C, chunk_tokens=256)
        op.p[5] = ws.data_ptr()
        op.i[9] = 1
        op.f[0] = 1.0                                            # scale: the logits are the sums themselves
        _launch([op])
        A = ws.cpu().view(B, Gr, chunks, 32, 32)[:, :, 0].double()
        ref = torch.softmax(_seq_sum(p).double(), -1)
        err = (A - ref).abs().max().item()
        assert err < 1e-5, f"{chunks} chunks: A differs from softmax(float32 ascending sum) by {err:.3e}"
        if chunks >= 9:
            rev = torch.softmax(_seq_sum(p.flip(0)).double(), -1)
            strided = torch.softmax(sum(_seq_sum(p[u::8]) for u in range(8)).double(), -1)
            assert (rev - ref).abs().max() > 1e-2 and (strided - ref).abs().max() > 1e-2, "the data does not tell the orders apart"
        out[chunks] = err
    return out


# the channel-attention shapes of the captioner's folded stages at the benched 768x768 crops, 2 crops (caption_f64.GPU_TIER's first three)
FOLDED_SHAPES = ((36864, 4), (9216, 8), (2304, 16))


def _chan_op_in_arena(qkv, B, N, G_, chunk, partial, osplit):
    """the plain (apply-pass) op inside caption_f64's guard bands: i5 = chunk, i10 = partial; returns (o, ws) as the op left them"""
    import caption_f64 as CF
    C = 32 * G_
    t = partial or chunk
    slots = B * G_ * ((N + t - 1) // t)
    ar = CF.Arena()
    ar.add("qkv", torch.float32, B * N, 3 * C, data=((0, qkv),)).add("o", torch.float32, B * N, C, out=((0, C),))
    ar.add("ws", torch.float32, slots, 1024, scratch=True)
    ar.build(None)
    L.launch(L.make_op(L.OP_CHAN_ATTN, L.F32, p=[ar.ptr("qkv"), None, None, None, ar.ptr("o"), ar.ptr("ws")],
                       i={0: B, 1: N, 3: C, 4: G_, 5: chunk, 6: osplit, 10: partial}))
    G._sync()
    ar.fetch(f"chan_attn i5={chunk} i10={partial}")              # nothing outside o and the N / t workspace slots was written
    return CF._rows_out(ar, "o", 0, C, osplit), ar.get("ws", 0, 1024)


def check_partial_tokens_bitwise(seed=4):
    """OMNI_OP_CHAN_ATTN i10 (tokens per partial): the op at i5 = 1024, i10 = 256 is the op at i5 = 256 — the same workspace (A and the
    remaining partials) and the same output, bit for bit — also where the last chunk and the last partial are ragged (N = 1400: six
    partials, the last of 120 tokens).  i10 that does not divide i5, i10 % 8 != 0 and a negative i10 are OMNI_E_ARG."""
    g = torch.Generator().manual_seed(seed)
    B, G_ = 2, 4
    for N in (1400, 2048):
        qkv = torch.randn(B * N, 3 * 32 * G_, generator=g)
        o1, ws1 = _chan_op_in_arena(qkv, B, N, G_, 1024, 256, 1)
        o2, ws2 = _chan_op_in_arena(qkv, B, N, G_, 256, 0, 1)
        assert ws1.shape == ws2.shape == (B * G_ * ((N + 255) // 256), 1024)
        assert torch.equal(ws1.view(torch.int32), ws2.view(torch.int32)) and torch.equal(o1.view(torch.int32), o2.view(torch.int32)), N
    refused = 0
    for bad in (384, 100, -256):
        buf = torch.zeros(B * 1024 * 3 * 128 + B * 1024 * 128 + B * G_ * 16 * 1024, device=G.DEV)
        op = L.make_op(L.OP_CHAN_ATTN, L.F32, p=[buf.data_ptr(), None, None, None, buf.data_ptr() + 4 * B * 1024 * 384,
                                                 buf.data_ptr() + 4 * B * 1024 * 512], i={0: B, 1: 1024, 3: 128, 4: G_, 5: 1024, 10: bad})
        try:
            L.launch(op)
        except L.OmniError as e:
            refused += "-1" in str(e).split(":")[0]              # OMNI_E_ARG
        G._sync()
        assert not buf.cpu().any(), f"i10 = {bad}: the refused op wrote"
    assert refused == 3
    return True


def check_partial_tokens_f64(seed=0, shapes=FOLDED_SHAPES):
    """The folded stages' ops carry i5 = 1024, i10 = 256, a setting caption_f64.GPU_TIER (keyed on i5) has no case of: the same shapes,
    formats, scales, f64 reference (plan_interp.chan_attn_ref), segment measure and bound as its chan_attn cases, run with i10 = 256."""
    import caption_f64 as CF
    import plan_interp as PI
    out = {}
    for N, G_ in shapes:
        for osplit in (1, 0):
            for scale in ("unit", "sharp"):
                g = torch.Generator().manual_seed(seed)
                B, C = CF.B2, 32 * G_
                qkv = torch.randn(B, N, 3, C, generator=g)
                qkv[:, :, 0] *= 8.0 if scale == "sharp" else 1.0
                qkv = qkv.reshape(B * N, 3 * C)
                o, _ = _chan_op_in_arena(qkv, B, N, G_, 1024, 256, osplit)
                e, _ = CF.seg_err(o, PI.chan_attn_ref(qkv.view(B, N, 3 * C), G_, 0.0, CF.F64), 32)
                bnd = CF.family_bound("chan_attn", {"scale": scale}, L.F32)
                print(f"chan_attn N={N} G={G_} i5=1024 i10=256 osplit={osplit} {scale}: {e:.2e} (bound {bnd:.1e})")
                assert e <= bnd, (N, G_, osplit, scale, e, bnd)
                out[(N, G_, osplit, scale)] = e
    return out

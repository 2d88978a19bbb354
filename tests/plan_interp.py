"""CPU interpreter of omni_op_t lists (TEST INFRASTRUCTURE ONLY).

Executes the descriptors a PlanBuilder produced with plain torch / numpy ops on the CPU tensors they
point to.  Two uses: (1) check the graph lowering (weight folding, slice bookkeeping, merged GEMMs,
decode-loop wiring) against the oracle models without a GPU; (2) per-op reference for the `gpu` tests.
Semantics are written independently of the HIP kernels, from the reference/hf code each op replaces.
"""
import bisect

import numpy as np
import torch
import torch.nn.functional as F

from omniparser_amd import _lib as L


class Mem:
    """raw address -> (tensor, element offset)."""

    def __init__(self, keep):
        uniq = {}
        for t in keep:
            if isinstance(t, torch.Tensor) and t.numel():
                uniq[t.data_ptr()] = t
        self.starts = sorted(uniq)
        self.tensors = [uniq[s] for s in self.starts]

    def at(self, ptr, dtype=None):
        """flat 1-D view starting at ptr (dtype defaults to the owning tensor's)."""
        if not ptr:
            return None
        i = bisect.bisect_right(self.starts, ptr) - 1
        t = self.tensors[i]
        off = ptr - self.starts[i]
        assert 0 <= off < t.numel() * t.element_size(), "pointer outside every known tensor"
        flat = t.reshape(-1).view(torch.uint8)[off:]
        dt = dtype or t.dtype
        n = flat.numel() // torch.empty((), dtype=dt).element_size()
        return flat[: n * torch.empty((), dtype=dt).element_size()].view(dt)



# ---- "format B" (csrc/gemm_dma.hip): per 16 channels 64 bytes = 16 hi halves then 16 lo halves, value = hi + lo
def _rtz_f16(x: torch.Tensor) -> torch.Tensor:
    """f32 -> f16 rounding toward zero (v_cvt_pkrtz_f16_f32), input already clamped to the f16 range."""
    h = x.to(torch.float16)
    bits = h.view(torch.int16).clone()
    over = h.float().abs() > x.abs()
    bits[over] -= 1                      # one ulp toward zero (sign-magnitude encoding)
    return bits.view(torch.float16)


def split_encode(x: torch.Tensor) -> torch.Tensor:
    """[rows, C] f32 (C % 16 == 0) -> [rows, C] f32-typed buffer holding format B."""
    rows, C = x.shape
    x = x.float().clamp(-65504.0, 65504.0)
    hi = _rtz_f16(x)
    lo = _rtz_f16(x - hi.float())
    out = torch.cat([hi.view(rows, C // 16, 16), lo.view(rows, C // 16, 16)], -1).contiguous()
    return out.view(rows, 2 * C).view(torch.float32)


def split_decode(buf: torch.Tensor) -> torch.Tensor:
    """inverse view: [rows, C] f32-typed buffer in format B -> f32 values."""
    rows, C = buf.shape
    hl = buf.contiguous().view(torch.float16).view(rows, C // 16, 2, 16).float()
    return (hl[:, :, 0] + hl[:, :, 1]).reshape(rows, C)


KPERM16 = (0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15)     # OMNI_OP_MLP_FUSED: K order of w2 inside a 16-group (include/omni_amd.h)


def _tdt(op):
    return torch.float32 if op.dtype == L.F32 else torch.float16


# ---- caption-op semantics: one statement per op family, on LOGICAL tensors (strides / offsets / storage formats resolved by the caller)
# and in a caller-chosen compute dtype.  run_op calls them with float32 (the interpreter's results); the per-op kernel checks
# (tests/caption_f64.py::check_caption_f64) call the same functions with float64.  Every function returns its result in `cd`.
def _nchw(x, cd):
    return x.permute(0, 3, 1, 2).to(cd)


def dwconv3_ref(x, w, b, cd):
    """x + depthwise_conv3x3(x, zero padding) + b.  x [B,H,W,C], w [3,3,C], b [C] -> [B,H,W,C]."""
    C = x.shape[-1]
    xc = _nchw(x, cd)
    wk = w.permute(2, 0, 1).unsqueeze(1).to(cd)
    return (F.conv2d(xc, wk, b.to(cd), padding=1, groups=C) + xc).permute(0, 2, 3, 1)


def dwconv3_ln_ref(x, w, b, g, be, eps, cd):
    """(y1, LayerNorm(y1)) with y1 = dwconv3_ref(...) rounded to x's storage dtype (the kernel stores it, the norm reads what is stored)."""
    y1 = dwconv3_ref(x, w, b, cd).to(x.dtype)
    return y1, F.layer_norm(y1.to(cd), (x.shape[-1],), g.to(cd), be.to(cd), eps)


def layernorm_ref(x, add, g, b, eps, cd):
    """LayerNorm over the last dim of x [rows, C]; add [period, C] (or None) is added to row r as add[r % period] first."""
    rows, C = x.shape
    x = x.to(cd)
    if add is not None:
        x = x + add.to(cd).repeat(rows // add.shape[0], 1)
    return F.layer_norm(x, (C,), g.to(cd), b.to(cd), eps)


def _sdpa(q, k, v, scale):
    return torch.softmax(q @ k.transpose(-2, -1) * scale, -1) @ v


def attn_plain_ref(q, k, v, heads, scale, cd):
    """ATTN_ROWS mode 0: q [G,nq,heads*D], k / v [G,nk,heads*D] -> [G,nq,heads*D] (softmax over all nk keys per head)."""
    G, nq, C = q.shape
    nk, D = k.shape[1], C // heads
    qh, kh, vh = (t.to(cd).reshape(G, -1, heads, D).transpose(1, 2) for t in (q, k, v))
    return _sdpa(qh, kh, vh, scale).transpose(1, 2).reshape(G, nq, C)


def window_partition(t, heads, pad_value=None):
    """[B,H,W,C] -> [B*wy*wx, heads, 144, D]: 12x12 windows, the image padded to whole windows with pad_value (a [C] row) or zeros."""
    B, H, W, C = t.shape
    wy, wx = (H + 11) // 12, (W + 11) // 12
    pad = torch.zeros(B, wy * 12, wx * 12, C, dtype=t.dtype)
    if pad_value is not None:
        pad[:] = pad_value
    pad[:, :H, :W] = t
    return pad.view(B, wy, 12, wx, 12, C).permute(0, 1, 3, 2, 4, 5).reshape(B * wy * wx, 144, heads, C // heads).transpose(1, 2)


def window_merge(o, B, H, W):
    """inverse of window_partition (the padding cropped): [B*wy*wx, heads, 144, D] -> [B,H,W,heads*D]."""
    wy, wx = (H + 11) // 12, (W + 11) // 12
    C = o.shape[1] * o.shape[3]
    o = o.transpose(1, 2).reshape(B, wy, wx, 12, 12, C).permute(0, 1, 3, 2, 4, 5).reshape(B, wy * 12, wx * 12, C)
    return o[:, :H, :W]


def attn_window_ref(q, k, v, kbias, vbias, heads, scale, cd):
    """ATTN_ROWS mode 1 (DaViT window attention): q / k / v [B,H,W,C] (biases already in), attention inside each 12x12 window of the
    image padded to whole windows; a padded key / value position holds kbias / vbias (what the qkv linear makes of a zero token)."""
    B, H, W, C = q.shape
    qw = window_partition(q.to(cd), heads)
    kw = window_partition(k.to(cd), heads, None if kbias is None else kbias.to(cd))
    vw = window_partition(v.to(cd), heads, None if vbias is None else vbias.to(cd))
    return window_merge(_sdpa(qw, kw, vw, scale), B, H, W)


def chan_attn_ref(qkv, G, scale, cd):
    """DaViT channel attention: qkv [B,N,3C] -> [B,N,C]; per group of C/G channels a (C/G)x(C/G) softmax over the N-token products;
    scale 0 means N^-0.5."""
    B, N, C3 = qkv.shape
    C = C3 // 3
    q, k, v = qkv.to(cd).view(B, N, 3, G, C // G).permute(2, 0, 3, 4, 1).unbind(0)          # [B,G,C/G,N]
    s = scale if scale != 0.0 else N ** -0.5
    return _sdpa(q, k, v, s).permute(0, 3, 1, 2).reshape(B, N, C)


def proj_prep_ref(x, pos, tmp, cd):
    """projector input: v = (x + pos) + tmp for x [B,N,C]; out [B,N+1,C] = [mean over tokens of v, v]."""
    v = (x.to(cd) + pos.to(cd)) + tmp.to(cd)
    return torch.cat([v.mean(1, keepdim=True), v], 1)


def embed_step_ref(table, pos_row, ids, C, scale, cd):
    """decoder token embedding: table rows of ids (a flat [V*C] table) * scale (0 means 1) + one position row."""
    rows = torch.stack([table[t * C:(t + 1) * C] for t in ids.tolist()]).to(cd) * (scale if scale != 0.0 else 1.0)
    return rows + pos_row.to(cd)


def attn_decode_ref(q, K, V, heads, scale, cd):
    """one query row per batch row against nk cached keys: q [B,C], K / V [B,nk,C] -> [B,C]."""
    B, nk, C = K.shape
    qh = q.to(cd).view(B, heads, 1, C // heads)
    Kh, Vh = (t.to(cd).view(B, nk, heads, C // heads).transpose(1, 2) for t in (K, V))
    return _sdpa(qh, Kh, Vh, scale).transpose(1, 2).reshape(B, C)


def attn_decode_self_ref(q, Kc, Vc, kn, vn, heads, scale, cd):
    """decoder self-attention at step st: the st cached rows Kc / Vc [B,st,C] plus this step's kn / vn [B,C] (appended to the cache)."""
    return attn_decode_ref(q, torch.cat([Kc, kn.unsqueeze(1)], 1), torch.cat([Vc, vn.unsqueeze(1)], 1), heads, scale, cd)


def greedy_step_ref(logits, bias, ids, fin, st, max_new, ngram, eos, pad, fbos, feos, cd):
    """transformers' greedy step (no-repeat-ngram ban, forced BOS / EOS, finished rows emit pad) on logits [B,V] (+ bias [V]); writes
    ids[:, st + 1] and updates fin in place (ids [B,T] / fin [B] int32); returns the chosen tokens."""
    cur_len = st + 1
    logits = logits.to(cd).clone()
    if bias is not None:
        logits += bias.to(cd)
    toks = []
    for b in range(logits.shape[0]):
        seq = ids[b, :cur_len].tolist()
        if ngram > 0 and cur_len + 1 >= ngram:
            prefix = seq[cur_len - (ngram - 1):]
            for s0 in range(cur_len - ngram + 1):
                if seq[s0:s0 + ngram - 1] == prefix:
                    logits[b, seq[s0 + ngram - 1]] = float("-inf")
        if fbos >= 0 and cur_len == 1:
            tok = fbos
        elif feos >= 0 and cur_len == max_new:
            tok = feos
        else:
            tok = int(torch.argmax(logits[b]))
        if fin[b]:
            tok = pad
        ids[b, st + 1] = tok
        if not fin[b] and tok == eos:
            fin[b] = 1
        toks.append(tok)
    return toks


def run_ops(ops, keep):
    m = Mem(keep)
    for op in ops:
        run_op(op, m)


def run_op(op, m):
    i, p, f = op.i, op.p, op.f
    dt = _tdt(op)
    k = op.kind
    if k == L.OP_CONV and i[20] == 2:
        # pre-split LDS-DMA GEMM: x and w in format B, optional format-B output
        B, H, W, Cin, ldi, icoff = [i[j] for j in range(6)]
        Cout, ldo, ocoff, act, ldr, rcoff = [i[j] for j in range(12, 18)]
        M = B * H * W
        x = split_decode(m.at(p[0], torch.float32)[: M * ldi].view(M, ldi)[:, icoff:icoff + Cin])
        w = split_decode(m.at(p[1], torch.float16)[: 2 * Cout * Cin].view(torch.float32).view(Cout, Cin)) * f[1]
        y = x @ w.t()
        if p[2]:
            y = y + m.at(p[2], torch.float32)[:Cout]
        if act == L.ACT_GELU:
            y = F.gelu(y)
        elif act == L.ACT_SILU:
            y = F.silu(y)
        if p[3]:
            y = y + m.at(p[3], torch.float32)[: M * ldr].view(M, ldr)[:, rcoff:rcoff + Cout]
        out = m.at(p[4], torch.float32)[: M * ldo].view(M, ldo)
        out[:, ocoff:ocoff + Cout] = split_encode(y) if i[21] else y
    elif k == L.OP_MLP_FUSED:
        rows, C, ldi, icoff, hid, ldo, ocoff, ldr, rcoff = i[0] * max(i[1], 1), i[3], i[4], i[5], i[12], i[13], i[14], i[16], i[17]
        x = split_decode(m.at(p[0], torch.float32)[: rows * ldi].view(rows, ldi)[:, icoff:icoff + C])
        w1 = split_decode(m.at(p[1], torch.float16)[: 2 * hid * C].view(torch.float32).view(hid, C)) * f[1]
        w2p = split_decode(m.at(p[5], torch.float16)[: 2 * hid * C].view(torch.float32).view(C, hid)) * f[2]
        inv = [KPERM16.index(j) for j in range(16)]                     # stored position of original channel j inside its 16-group
        w2 = w2p.view(C, hid // 16, 16)[:, :, inv].reshape(C, hid)
        h = F.gelu(x @ w1.t() + m.at(p[2], torch.float32)[:hid])
        h = split_decode(split_encode(h))                               # the kernel hands fc2 the (hi, lo) halves of the activations
        y = h @ w2.t() + m.at(p[6], torch.float32)[:C] + m.at(p[3], torch.float32)[: rows * ldr].view(rows, ldr)[:, rcoff:rcoff + C]
        m.at(p[4], torch.float32)[: rows * ldo].view(rows, ldo)[:, ocoff:ocoff + C] = y
    elif k == L.OP_SPLIT_CONVERT:
        rows, C, ldi, icoff, ldo, ocoff = i[0] * max(i[1], 1), i[3], i[4], i[5], i[13], i[14]
        x = m.at(p[0], torch.float32)[: rows * ldi].view(rows, ldi)[:, icoff:icoff + C].clone()
        m.at(p[4], torch.float32)[: rows * ldo].view(rows, ldo)[:, ocoff:ocoff + C] = split_encode(x)
    elif k == L.OP_CONV:
        B, H, W, Cin, ldi, icoff, KH, KW, s, pad, Ho, Wo, Cout, ldo, ocoff, act, ldr, rcoff = [i[j] for j in range(18)]
        if i[25]:
            # row-patch mode (include/omni_amd.h): a KH x KH convolution over the ldi = 4 stored channels, weights [Cout][KH][8 pixels][4]
            hl = m.at(p[1], torch.float16)[: 2 * Cout * KH * 32].view(Cout, KH * 2, 2, 16).float()
            w = (hl[:, :, 0] + hl[:, :, 1] / 2048.0).reshape(Cout, KH, 8, ldi)
            assert float(w[:, :, KH:].abs().max()) == 0.0
            w = w[:, :, :KH].permute(0, 3, 1, 2)
            x = m.at(p[0], dt)[: B * H * W * ldi].view(B, H, W, ldi).permute(0, 3, 1, 2).float()
            Cin, KW = ldi, KH
        else:
            x = m.at(p[0], dt)[: B * H * W * ldi].view(B, H, W, ldi)[..., icoff:icoff + Cin].permute(0, 3, 1, 2).float()
        if i[25]:
            pass
        elif i[20]:
            hl = m.at(p[1], torch.float16)[: 2 * Cout * KH * KW * Cin].view(Cout, KH * KW * Cin // 16, 2, 16).float()
            w = (hl[:, :, 0] + hl[:, :, 1] / 2048.0).reshape(Cout, KH, KW, Cin).permute(0, 3, 1, 2)
        else:
            w = m.at(p[1], dt)[: Cout * KH * KW * Cin].view(Cout, KH, KW, Cin).permute(0, 3, 1, 2).float()
        b = m.at(p[2], torch.float32)[:Cout] if p[2] else None
        y = F.conv2d(x, w, b, stride=s, padding=pad)
        if f[0] != 0.0:
            y = y * f[0]
        if act == L.ACT_SILU:
            y = F.silu(y)
        elif act == L.ACT_GELU:
            y = F.gelu(y)
        if p[3]:
            y = y + m.at(p[3], dt)[: B * Ho * Wo * ldr].view(B, Ho, Wo, ldr)[..., rcoff:rcoff + Cout].permute(0, 3, 1, 2).float()
        out = m.at(p[4], dt)[: B * Ho * Wo * ldo].view(B, Ho, Wo, ldo)
        out[..., ocoff:ocoff + Cout] = y.permute(0, 2, 3, 1).to(dt)
    elif k in (L.OP_AVGPOOL2, L.OP_MAXPOOL, L.OP_RESIZE_NEAREST):
        B, H, W, C, ldi, icoff = [i[j] for j in range(6)]
        kk, s, pad, Ho, Wo, ldo, ocoff, acc = i[6], i[8], i[9], i[10], i[11], i[13], i[14], i[18]
        x = m.at(p[0], dt)[: B * H * W * ldi].view(B, H, W, ldi)[..., icoff:icoff + C].permute(0, 3, 1, 2).float()
        if k == L.OP_AVGPOOL2:
            y = F.avg_pool2d(x, 2, 1, 0, False, True); Ho, Wo = H - 1, W - 1
        elif k == L.OP_MAXPOOL:
            y = F.max_pool2d(x, kk, s, pad)
        else:
            y = F.interpolate(x, size=(Ho, Wo), mode="nearest")
            if i[17] > 1:                       # CBFuse in one op: ((r(x0) + r(x1)) + ...) with every partial sum rounded to the plan's dtype
                slots = ((19, 20, 21, 22), (23, 24, 25, 26), (27, 28, 29, 30), (7, 12, 15, 16))
                for kx in range(i[17] - 1):
                    Hk, Wk, ldk, cok = (i[j] for j in slots[kx])
                    xk = m.at(p[(1, 2, 3, 5)[kx]], dt)[: B * Hk * Wk * ldk].view(B, Hk, Wk, ldk)[..., cok:cok + C].permute(0, 3, 1, 2).float()
                    y = y.to(dt).float() + F.interpolate(xk, size=(Ho, Wo), mode="nearest")
        out = m.at(p[4], dt)[: B * Ho * Wo * ldo].view(B, Ho, Wo, ldo)
        y = y.permute(0, 2, 3, 1)
        if acc:
            y = out[..., ocoff:ocoff + C].float() + y
        out[..., ocoff:ocoff + C] = y.to(dt)
    elif k == L.OP_DWCONV3:
        B, H, W, C = i[0], i[1], i[2], i[3]
        x = m.at(p[0], dt)[: B * H * W * C].view(B, H, W, C)
        y = dwconv3_ref(x, m.at(p[1], dt)[: 9 * C].view(3, 3, C), m.at(p[2], torch.float32)[:C], torch.float32)
        m.at(p[4], dt)[: B * H * W * C].view(B, H, W, C).copy_(y.to(dt))
    elif k == L.OP_DWCONV3_LN:
        B, H, W, C = i[0], i[1], i[2], i[3]
        x = m.at(p[0], dt)[: B * H * W * C].view(B, H, W, C)
        y1, hn = dwconv3_ln_ref(x, m.at(p[1], dt)[: 9 * C].view(3, 3, C), m.at(p[2], torch.float32)[:C], m.at(p[5], torch.float32)[:C],
                                m.at(p[6], torch.float32)[:C], f[0], torch.float32)
        m.at(p[4], dt)[: B * H * W * C].view(B, H, W, C).copy_(y1)
        m.at(p[3], dt)[: B * H * W * C].view(B, H, W, C).copy_(split_encode(hn.reshape(-1, C)).view(B, H, W, C) if i[6] else hn.to(dt))
    elif k == L.OP_LAYERNORM:
        rows, C, period = i[0] * max(i[1], 1), i[3], i[5]
        x = m.at(p[0], dt)[: rows * C].view(rows, C)
        add = m.at(p[1], dt)[: period * C].view(period, C) if p[1] else None
        y = layernorm_ref(x, add, m.at(p[2], torch.float32)[:C], m.at(p[3], torch.float32)[:C], f[0], torch.float32)
        if i[6] == 1:
            m.at(p[4], dt)[: rows * C].view(rows, C).copy_(split_encode(y))
        else:
            m.at(p[4], dt)[: rows * C].view(rows, C).copy_(y.to(dt))
            if i[6] == 2:
                m.at(p[5], dt)[: rows * C].view(rows, C).copy_(split_encode(y))
    elif k == L.OP_ATTN_ROWS:
        ldq, ldk, ldv, ldo, qoff, koff, voff, ooff, heads, nq, nk, groups, mode, H, W, D = [i[j] for j in range(16)]
        C = heads * D
        if mode == 0:
            rows = groups * nq
            q = m.at(p[0], dt)[: rows * ldq].view(groups, nq, ldq)[..., qoff:qoff + C]
            kx = m.at(p[1], dt)[: groups * nk * ldk].view(groups, nk, ldk)[..., koff:koff + C]
            v = m.at(p[2], dt)[: groups * nk * ldv].view(groups, nk, ldv)[..., voff:voff + C]
            oo = attn_plain_ref(q, kx, v, heads, f[0], torch.float32)
            out = m.at(p[4], dt)[: rows * ldo].view(groups, nq, ldo)
            out[..., ooff:ooff + C] = split_encode(oo.reshape(rows, C)).view(groups, nq, C) if i[16] else oo.to(dt)
        else:
            B = groups // (((H + 11) // 12) * ((W + 11) // 12))
            q, kx, v = (m.at(ptr, dt)[: B * H * W * ld].view(B, H, W, ld)[..., off:off + C]
                        for ptr, ld, off in ((p[0], ldq, qoff), (p[1], ldk, koff), (p[2], ldv, voff)))
            kb = m.at(p[5], torch.float32)[:C] if p[5] else None
            vb = m.at(p[6], torch.float32)[:C] if p[6] else None
            oo = attn_window_ref(q, kx, v, kb, vb, heads, f[0], torch.float32)
            out = m.at(p[4], dt)[: B * H * W * ldo].view(B, H, W, ldo)
            out[..., ooff:ooff + C] = split_encode(oo.reshape(B * H * W, C)).view(B, H, W, C) if i[16] else oo.to(dt)
    elif k == L.OP_CHAN_ATTN:
        B, N, C, G = i[0], i[1], i[3], i[4]
        oo = chan_attn_ref(m.at(p[0], dt)[: B * N * 3 * C].view(B, N, 3 * C), G, f[0], torch.float32)
        m.at(p[4], dt)[: B * N * C].view(B, N, C).copy_(split_encode(oo.reshape(B * N, C)).view(B, N, C) if i[6] else oo.to(dt))
    elif k == L.OP_PROJ_PREP:
        B, N, C = i[0], i[1], i[3]
        y = proj_prep_ref(m.at(p[0], dt)[: B * N * C].view(B, N, C), m.at(p[1], torch.float32)[: N * C].view(N, C),
                          m.at(p[2], torch.float32)[:C], torch.float32)
        m.at(p[4], dt)[: B * (N + 1) * C].view(B, N + 1, C).copy_(y.to(dt))
    elif k == L.OP_ASSEMBLE:
        B, n_img, n_txt, C = i[0], i[1], i[2], i[3]
        out = m.at(p[4], dt)[: B * (n_img + n_txt) * C].view(B, n_img + n_txt, C)
        out[:, :n_img] = m.at(p[0], dt)[: B * n_img * C].view(B, n_img, C)
        out[:, n_img:] = m.at(p[1], dt)[: n_txt * C].view(n_txt, C)
    elif k == L.OP_EMBED_STEP:
        B, C, T, off = i[0], i[3], i[4], i[5]
        st = int(m.at(p[6], torch.int32)[0])
        ids = m.at(p[2], torch.int32)[: B * T].view(B, T)[:, st].long()
        y = embed_step_ref(m.at(p[0], dt), m.at(p[1], dt)[(st + off) * C:(st + off + 1) * C], ids, C, f[0], torch.float32)
        m.at(p[4], dt)[: B * C].view(B, C).copy_(y.to(dt))
    elif k == L.OP_ATTN_DECODE:
        ldq, qoff, ldn, koff, voff, ldo, heads, nk_fixed, cap, C, B, ldc = [i[j] for j in range(12)]
        ldc = ldc or C
        q = m.at(p[0], dt)[: B * ldq].view(B, ldq)[:, qoff:qoff + C]
        kc = m.at(p[3], dt)[: B * cap * ldc - 0].view(-1)
        vc = m.at(p[5], dt).view(-1)
        # cache row r of batch b starts at (b*cap + r)*ldc
        def rows(buf, nk):
            n_el = (B * cap - 1) * ldc + C
            t = buf[:n_el]
            idx = (torch.arange(B).view(B, 1) * cap + torch.arange(nk).view(1, nk)) * ldc
            if nk == 0:
                return t.new_zeros(B, 0, C)
            return torch.stack([torch.stack([t[o:o + C] for o in row.tolist()]) for row in idx])   # [B,nk,C]
        if nk_fixed > 0:
            o = attn_decode_ref(q, rows(kc, nk_fixed), rows(vc, nk_fixed), heads, f[0], torch.float32)
        else:
            st = int(m.at(p[6], torch.int32)[0])
            kn = m.at(p[1], dt)[: B * ldn].view(B, ldn)[:, koff:koff + C]
            vn = m.at(p[2], dt)[: B * ldn].view(B, ldn)[:, voff:voff + C]
            o = attn_decode_self_ref(q, rows(kc, st), rows(vc, st), kn, vn, heads, f[0], torch.float32)
            for b in range(B):
                r = (b * cap + st) * ldc
                kc[r:r + C] = kn[b]; vc[r:r + C] = vn[b]
        m.at(p[4], dt)[: B * ldo].view(B, ldo)[:, :C] = o.to(dt)
    elif k == L.OP_GREEDY_STEP:
        B, V, ldl, T, max_new, ngram, bos, eos, pad, fbos, feos, inc = [i[j] for j in range(12)]
        step = m.at(p[6], torch.int32)
        st = int(step[0])
        logits = m.at(p[0], dt)[: B * ldl].view(B, ldl)[:, :V]
        bias = m.at(p[1], torch.float32)[:V] if p[1] else None
        ids = m.at(p[2], torch.int32)[: B * T].view(B, T)
        fin = m.at(p[3], torch.int32)[:B]
        greedy_step_ref(logits, bias, ids, fin, st, max_new, ngram, eos, pad, fbos, feos, torch.float32)
        if inc:
            step[0] = st + 1
    elif k == L.OP_CROP_RESIZE:
        from oracle import preprocess_ref as PR
        n, H, W, R, ks, ldo = i[0], i[1], i[2], i[3], i[4], i[13]
        img = m.at(p[0], torch.uint8)[: H * W * 3].view(H, W, 3).numpy()
        boxes = m.at(p[1], torch.int32)[: n * 4].view(n, 4).tolist()
        out = m.at(p[4], dt)[: n * R * R * ldo].view(n, R, R, ldo)
        mean = np.array([f[0], f[1], f[2]], dtype=np.float32); std = np.array([f[3], f[4], f[5]], dtype=np.float32)
        for j, (x0, y0, x1, y1) in enumerate(boxes):
            out[j] = 0
            out[j, :, :, :3] = torch.from_numpy(PR.caption_pixel_values(img, (x0, y0, x1, y1), R, mean, std)).to(dt)
    else:
        raise NotImplementedError(f"interp: op kind {k}")

"""The per-segment bounds of tests/caption_f64.py are tight enough to matter and loose enough to hold (pure torch, no kernels).

For every caption-op family a DEFECT MODEL — a plausible way for a rewritten kernel to be subtly wrong — is fed to the same comparison
the kernel checks use (`seg_err` against the float64 reference of tests/plan_interp.py) in place of the kernel's output: the bound must
reject it.  The float32 interpreter (the same reference functions in float32) must be accepted, so no bound sits below float noise.
Each test also records whether the old whole-tensor check (`gpu_checks._cmp` at the tolerance check_caption_ops uses for that family)
would have accepted the defect."""
import pytest
import torch

import caption_f64 as CF
import plan_interp as PI
from omniparser_amd import _lib as L

F64 = torch.float64
OLD_TOL = {"attn_window": 1e-4, "attn_mha": 1e-4, "chan_attn": 2e-4, "layernorm": 1e-4, "dwconv3": 2e-5, "attn_decode": 1e-4}


def _old_accepts(y, ref, tol):
    """gpu_checks._cmp: largest error over the tensor / largest reference value over the tensor."""
    return float((y.double() - ref.double()).abs().max() / ref.double().abs().max()) <= tol


def _split(x):
    """the kernels' split-f16 operand: x = hi + lo, both f16 (rounded toward zero, as v_cvt_pkrtz_f16_f32)."""
    x = x.float()
    hi = PI._rtz_f16(x).double()
    lo = PI._rtz_f16((x.double() - hi).float()).double()
    return hi, lo


def _dropped_cross(a, b):
    """a @ b^T from split operands with the lo(a) x hi(b) product left out: hi.hi + hi.lo only."""
    ah, al = _split(a)
    bh, bl = _split(b)
    return ah @ bh.transpose(-2, -1) + ah @ bl.transpose(-2, -1)


def _judge(family, ref, defect, f32, seg, dtype=L.F32, scale="unit"):
    bnd = CF.family_bound(family.replace("_1e3", ""), {"scale": "offset" if family.endswith("_1e3") else scale}, dtype)
    e_def, _ = CF.seg_err(defect, ref, seg)
    e_f32, _ = CF.seg_err(f32, ref, seg)
    old = _old_accepts(defect, ref, OLD_TOL[family.replace("_1e3", "")])
    print(f"{family}: defect {e_def:.2e}, f32 interpreter {e_f32:.2e}, bound {bnd:.1e}, old check accepts the defect: {old}")
    assert e_f32 <= bnd, (family, e_f32, bnd)
    assert e_def > bnd, (family, e_def, bnd)
    return old


def _qkv_window(g, B, H, C, sharp):
    q = torch.randn(B, H, H, C, generator=g) * sharp
    return q, torch.randn(B, H, H, C, generator=g), torch.randn(B, H, H, C, generator=g), torch.randn(C, generator=g), torch.randn(C, generator=g)


def test_window_attention_dropped_cross_product_is_rejected():
    g = torch.Generator().manual_seed(0)
    B, H, heads, D = 2, 24, 4, 32
    q, k, v, kb, vb = _qkv_window(g, B, H, heads * D, 1.0)
    ref = PI.attn_window_ref(q, k, v, kb, vb, heads, D ** -0.5, F64)
    qw, kw, vw = PI.window_partition(q.double(), heads), PI.window_partition(k.double(), heads), PI.window_partition(v.double(), heads)
    s = _dropped_cross(qw, kw) * D ** -0.5
    defect = PI.window_merge(torch.softmax(s, -1) @ vw, B, H, H)
    _judge("attn_window", ref, defect, PI.attn_window_ref(q, k, v, kb, vb, heads, D ** -0.5, torch.float32), D)


def test_channel_attention_dropped_cross_product_is_rejected():
    g = torch.Generator().manual_seed(1)
    B, N, G = 2, 2304, 4
    qkv = torch.randn(B, N, 3 * 32 * G, generator=g)
    ref = PI.chan_attn_ref(qkv, G, 0.0, F64)
    q, k, v = qkv.double().view(B, N, 3, G, 32).permute(2, 0, 3, 4, 1).unbind(0)
    defect = (torch.softmax(_dropped_cross(q, k) * N ** -0.5, -1) @ v).permute(0, 3, 1, 2).reshape(B, N, 32 * G)
    _judge("chan_attn", ref, defect, PI.chan_attn_ref(qkv, G, 0.0, torch.float32), 32)


def test_exp2_with_a_rounded_log2e_is_rejected():
    """softmax as exp2(s * log2(e)) with log2(e) rounded to 1.4427 (a 3.4e-6 relative error in every exponent), O(1) scores (with
    sharp scores the float32 rounding of the scores themselves is of the same size as this defect)."""
    g = torch.Generator().manual_seed(2)
    B, S, heads, D = 2, 585, 12, 64
    q, k, v = torch.randn(B, S, heads * D, generator=g), torch.randn(B, S, heads * D, generator=g), torch.randn(B, S, heads * D, generator=g)
    ref = PI.attn_plain_ref(q, k, v, heads, D ** -0.5, F64)
    qh, kh, vh = (t.double().view(B, S, heads, D).transpose(1, 2) for t in (q, k, v))
    s = qh @ kh.transpose(-2, -1) * D ** -0.5
    p = torch.exp2((s - s.amax(-1, keepdim=True)) * 1.4427)
    defect = ((p / p.sum(-1, keepdim=True)) @ vh).transpose(1, 2).reshape(B, S, heads * D)
    _judge("attn_mha", ref, defect, PI.attn_plain_ref(q, k, v, heads, D ** -0.5, torch.float32), D)


def test_cut_window_with_zero_padded_keys_is_rejected():
    """a cut window (H = 13: one row / column of a second window) whose padded key / value positions hold 0 instead of the biases."""
    g = torch.Generator().manual_seed(3)
    B, H, heads, D = 2, 13, 4, 32
    q, k, v, kb, vb = _qkv_window(g, B, H, heads * D, 1.0)
    ref = PI.attn_window_ref(q, k, v, kb, vb, heads, D ** -0.5, F64)
    defect = PI.attn_window_ref(q, k, v, None, None, heads, D ** -0.5, F64)
    _judge("attn_window", ref, defect, PI.attn_window_ref(q, k, v, kb, vb, heads, D ** -0.5, torch.float32), D)


def test_channel_attention_f16_chunk_partials_are_rejected():
    """the partial scores of every 1024-token chunk rounded to f16 before the chunks are combined (N = 36864: 36 chunks)."""
    g = torch.Generator().manual_seed(4)
    B, N, G = 1, 36864, 4
    qkv = torch.randn(B, N, 3 * 32 * G, generator=g)
    ref = PI.chan_attn_ref(qkv, G, 0.0, F64)
    q, k, v = qkv.double().view(B, N, 3, G, 32).permute(2, 0, 3, 4, 1).unbind(0)
    s = sum((q[..., c:c + 1024] @ k[..., c:c + 1024].transpose(-2, -1)).half().double() for c in range(0, N, 1024))
    defect = (torch.softmax(s * N ** -0.5, -1) @ v).permute(0, 3, 1, 2).reshape(B, N, 32 * G)
    _judge("chan_attn", ref, defect, PI.chan_attn_ref(qkv, G, 0.0, torch.float32), 32)


def test_one_pass_layernorm_variance_is_rejected():
    """var = E[x^2] - E[x]^2 in f32 on rows with mean 1e3 and standard deviation 1."""
    g = torch.Generator().manual_seed(5)
    rows, C = 64, 768
    x = torch.randn(rows, C, generator=g) + 1e3
    gg, b = torch.randn(C, generator=g), torch.randn(C, generator=g)
    ref = PI.layernorm_ref(x, None, gg, b, 1e-5, F64)
    mean = x.mean(1, keepdim=True)
    var = (x * x).mean(1, keepdim=True) - mean * mean
    defect = (x - mean) * torch.rsqrt(var.clamp_min(0) + 1e-5) * gg + b
    _judge("layernorm_1e3", ref, defect, PI.layernorm_ref(x, None, gg, b, 1e-5, torch.float32), C)


def test_dwconv_clamped_last_column_is_rejected():
    """the depthwise conv clamps (replicates the last column) instead of zero-padding at the right border."""
    g = torch.Generator().manual_seed(6)
    B, H, W, C = 2, 24, 24, 256
    x, w, b = torch.randn(B, H, W, C, generator=g), torch.randn(3, 3, C, generator=g) * 0.3, torch.randn(C, generator=g)
    ref = PI.dwconv3_ref(x, w, b, F64)
    xd = x.double().permute(0, 3, 1, 2)
    xp = torch.nn.functional.pad(xd, (1, 1, 1, 1))
    xp[..., 1:-1, -1] = xd[..., -1]
    y = torch.nn.functional.conv2d(xp, w.double().permute(2, 0, 1).unsqueeze(1), b.double(), groups=C) + xd
    _judge("dwconv3", ref, y.permute(0, 2, 3, 1), PI.dwconv3_ref(x, w, b, torch.float32), C)


@pytest.mark.parametrize("st", [1, 10, 19])
def test_decode_self_attention_without_the_new_row_is_rejected(st):
    g = torch.Generator().manual_seed(7 + st)
    B, heads = 3, 12
    C = 64 * heads
    q, kn, vn = (torch.randn(B, C, generator=g) for _ in range(3))
    kc, vc = torch.randn(B, st, C, generator=g), torch.randn(B, st, C, generator=g)
    ref = PI.attn_decode_self_ref(q, kc, vc, kn, vn, heads, 0.125, F64)
    defect = PI.attn_decode_ref(q, kc, vc, heads, 0.125, F64)
    _judge("attn_decode", ref, defect, PI.attn_decode_self_ref(q, kc, vc, kn, vn, heads, 0.125, torch.float32), 64)


def test_segment_metric_reports_a_defect_confined_to_one_head():
    """an error in one head of one token, 1 % of the tensor's scale: invisible to a whole-tensor max / max at 1e-4, found and located
    by seg_err."""
    g = torch.Generator().manual_seed(9)
    ref = torch.randn(2, 50, 4, 32, generator=g).double()
    ref[1, 17, 2] *= 0.01
    y = ref.clone()
    y[1, 17, 2] *= 1 + 5e-3
    e, i = CF.seg_err(y, ref, 32)
    assert CF.where(i, (2, 50, 4)) == (1, 17, 2) and e > 1e-3
    assert _old_accepts(y, ref, 1e-4)


def test_gpu_tier_covers_every_benched_caption_op():
    """The GPU tier's case list cannot drift from the plans: every distinct dispatch-relevant signature of the caption ops in the
    captioner's plans at the benched 768x768 crops (2 crops, built on the CPU) must be a case of caption_f64.GPU_TIER."""
    import caption_checks as CC
    from tools.make_weights import ensure_caption_checkpoint
    cap, cp = CC.build_cpu_plans(ensure_caption_checkpoint(0), CF.B2, 768)
    plan = {CF.op_signature(op, CF.B2) for op in list(cp.encode_plan.ops) + list(cp.step_plan.ops)} - {None}
    cases = {CF.case_signature(f, p) for f, p in CF.GPU_TIER}
    missing = sorted(map(str, plan - cases))
    assert not missing, missing
    assert len(plan) >= 25, sorted(map(str, plan))

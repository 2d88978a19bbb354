"""`-m gpu`: channel-attention scores computed in the q|k GEMM's epilogue (Florence2Captioner.chan_scores_in_gemm) on the MI355X."""
import pytest

pytestmark = pytest.mark.gpu


def test_scores_epilogue_bitwise_vs_standalone_scores():
    import chan_scores_epi_checks as C
    r = C.check_scores_bitwise()
    assert len(r) == 8 and all(r.values())


def test_scores_epilogue_writes_no_y_and_stays_inside_ws():
    import chan_scores_epi_checks as C
    assert C.check_y_not_written()


def test_scores_epilogue_argument_errors():
    import chan_scores_epi_checks as C
    assert len(C.check_argument_errors()) == 7


def test_softmax_sums_partials_in_ascending_chunk_order():
    import chan_scores_epi_checks as C
    assert set(C.check_softmax_order()) == {1, 2, 9, 144}


def test_tokens_per_partial_is_the_op_at_that_chunk():
    import chan_scores_epi_checks as C
    assert C.check_partial_tokens_bitwise()


def test_tokens_per_partial_vs_f64_at_the_benched_shapes():
    """the folded stages' channel-attention shapes at 768x768, 2 crops, with the plans' i5 = 1024, i10 = 256 (caption_f64's bound)"""
    import chan_scores_epi_checks as C
    assert len(C.check_partial_tokens_f64()) == 12


def test_captioner_r768_scores_in_gemm_on_and_off():
    """One captioner at 768x768, 2 crops, same pixels, with chan_scores_in_gemm on and off: img_feat is torch.equal, the greedy ids are
    equal (both sides sum their scores over the same 256-token partials, i5 = 1024 with i10 = 256, in the same order).  With the switch on, every fold-mode
    OMNI_OP_CHAN_ATTN of DaViT stages 0-2 carries the skip flag (i9 = 1: no scores launch) and every channel block of those stages has
    one scores-mode GEMM (OMNI_OP_CONV i28 = 1); with the switch off the plan has neither."""
    import torch
    from omniparser_amd import _lib as L
    from omniparser_amd.florence import Florence2Captioner
    from tools.make_weights import ensure_caption_checkpoint
    R, n, max_new = 768, 2, 20
    d = ensure_caption_checkpoint(0)
    g = torch.Generator().manual_seed(23 + R)
    pix = torch.randn(n, 3, R, R, generator=g)
    cap = Florence2Captioner(d, "cuda", precision="f32", resolution=R)
    got = {}
    for on in (True, False):
        cap.chan_scores_in_gemm = on
        ids = cap.generate(pixel_values=pix, max_new_tokens=max_new)
        cp = cap.plans(cap.bucket(n), R, max_new)
        ops = cp.encode_plan.ops
        chan = [op for op in ops if op.kind == L.OP_CHAN_ATTN]
        got[on] = {"ids": ids.cpu(), "feat": cp.img_feat.t[:n, :, 0, :].clone().cpu(), "stages": list(cp.fold_stages),
                   "chan": [(op.i[3], op.i[8], op.i[9], (op.i[5], op.i[10])) for op in chan],
                   "scores_gemms": [op.i[12] // 2 for op in ops if op.kind == L.OP_CONV and op.i[20] == 2 and op.i[28] == 1]}
        del cp
        torch.cuda.synchronize()
        cap.clear_plans()
    assert got[True]["stages"] == [0, 1, 2] == got[False]["stages"]
    folded_on = [c for c in got[True]["chan"] if c[1] == 1]
    assert folded_on and all(skip == 1 and ct == (1024, 256) for _, _, skip, ct in folded_on), got[True]["chan"]
    assert all(skip == 0 for _, fold, skip, _ in got[True]["chan"] if fold == 0)
    assert sorted(got[True]["scores_gemms"]) == sorted(c for c, _, _, _ in folded_on), (got[True]["scores_gemms"], folded_on)
    assert got[False]["scores_gemms"] == [] and all(skip == 0 for _, _, skip, _ in got[False]["chan"])
    assert all(ct == ((1024, 256) if fold == 1 else (1024, 0)) for on in got for _, fold, _, ct in got[on]["chan"])
    assert torch.equal(got[True]["feat"], got[False]["feat"]), "img_feat differs between the two sides of chan_scores_in_gemm"
    assert torch.equal(got[True]["ids"], got[False]["ids"]), (got[True]["ids"], got[False]["ids"])

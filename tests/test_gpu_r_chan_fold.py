"""`-m gpu`: channel attention folded into a per-image projection GEMM (Florence2Captioner.fold_chan_proj) on the MI355X."""
import pytest

pytestmark = pytest.mark.gpu


def test_gemm_with_per_image_weights_vs_f64():
    import chan_fold_checks as C
    r = C.check_gemm_per_image()
    assert r["worst_rel_err"] < 2e-6 and all(r["bitwise_same_matrix"].values())


def test_fold_kernels_chain_bound_and_packed_bits():
    import chan_fold_checks as C
    C.check_fold()


def test_channel_block_tail_folded_and_unfolded_vs_f64():
    import chan_fold_checks as C
    C.check_composition()


def test_captioner_r768_fold_on_and_off():
    """One captioner at 768x768, 2 crops, with the fold on and off: equal greedy ids; img_feat of both within 2e-5 (max-norm relative)
    of a float64 evaluation of the network (the transformers model in double precision on the same pixels); the folded plan has no
    channel-attention apply launch in DaViT stages 0-2 (every OMNI_OP_CHAN_ATTN of those stages is in fold mode and writes no `att`),
    the unfolded plan has no fold.
    Bound: 2e-5.  The project's records hold no img_feat difference between two equivalent 768x768 compositions, only distances to the
    f32 CPU model (4.7e-6 - 6.8e-6: profiles/r4_s2_candidates_parity.json, profiles/r3_bisect.jsonl), so the fixed figure is the one
    they support.  Measured on the MI355X against the f64 model (this test's own print): 2.41e-6 folded, 2.29e-6 unfolded, 1.65e-6 between
    the two compositions."""
    import torch
    import gpu_checks as G
    from omniparser_amd import _lib as L
    from omniparser_amd.florence import Florence2Captioner
    from tools.make_weights import ensure_caption_checkpoint, shared_random_captioner
    R, n, max_new = 768, 2, 20
    d = ensure_caption_checkpoint(0)
    g = torch.Generator().manual_seed(11 + R)
    pix = torch.randn(n, 3, R, R, generator=g)
    model = shared_random_captioner(0)
    with torch.inference_mode():
        m64 = model.model.double()
        try:
            ref = m64.get_image_features(pix.double()).pooler_output.clone()
        finally:
            model.model.float()
    cap = Florence2Captioner(d, "cuda", precision="f32", resolution=R)
    got = {}
    for fold in (True, False):
        cap.fold_chan_proj = fold
        ids = cap.generate(pixel_values=pix, max_new_tokens=max_new)
        cp = cap.plans(cap.bucket(n), R, max_new)
        chan = [op for op in cp.encode_plan.ops if op.kind == L.OP_CHAN_ATTN]
        got[fold] = {"ids": ids.cpu(), "feat": cp.img_feat.t[:n, :, 0, :].double().cpu(), "stages": list(cp.fold_stages),
                     "modes": [(op.i[3], op.i[8], bool(op.p[4])) for op in chan]}
        del cp
        torch.cuda.synchronize()
        cap.clear_plans()
    errs = {fold: G.rel_err(v["feat"], ref) for fold, v in got.items()}
    print({"img_feat_rel_err_vs_f64": errs, "fold_vs_unfolded": G.rel_err(got[True]["feat"], got[False]["feat"])})
    assert got[True]["stages"] == [0, 1, 2] and got[False]["stages"] == []
    widths = sorted({c for c, _, _ in got[True]["modes"]})
    for c, mode, has_att in got[True]["modes"]:
        assert (mode == 1 and not has_att) if c in widths[:3] else (mode == 0 and has_att), got[True]["modes"]
    assert all(mode == 0 and has_att for _, mode, has_att in got[False]["modes"])
    assert torch.equal(got[True]["ids"], got[False]["ids"]), (got[True]["ids"], got[False]["ids"])
    for fold, e in errs.items():
        assert e < 2e-5, f"fold_chan_proj={fold}: img_feat rel err {e:.3e} vs the f64 model"

"""`-m gpu`: Wv folded into channel attention's per-image projection (Florence2Captioner.fold_chan_v) on the MI355X."""
import pytest

pytestmark = pytest.mark.gpu


def test_bias_table_chain_bound_and_scale_product():
    import chan_vfold_checks as C
    C.check_bias_table_and_scale()


def test_fold_gemm_vs_f64_and_repacked_bits():
    import chan_vfold_checks as C
    print(C.check_fold_gemm())


def test_gemm_with_per_image_bias():
    import chan_vfold_checks as C
    assert C.check_per_image_bias()["worst_rel_err"] < 2e-6


def test_channel_block_tail_three_forms_vs_f64():
    import chan_vfold_checks as C
    C.check_block_tail()


def test_captioner_r768_fold_chan_v_on_and_off():
    """One captioner at 768x768, 2 crops, the pixels and the float64 model of test_captioner_r768_fold_on_and_off, with fold_chan_v on and
    off: equal greedy ids; img_feat of both sides within 2e-5 (max-norm relative, that test's bound) of the float64 model; with the
    switch on no OMNI_OP_CONV of stages 0-2 writes a v slice and there is one fold GEMM per folded channel block (11), with it off there
    is none and no op carries a new slot.
    Measured on the MI355X against the f64 model (this test's own print): 2.10e-6 with the switch on, 2.12e-6 off, 1.50e-6 between the two."""
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
    for on in (True, False):
        cap.fold_chan_v = on
        ids = cap.generate(pixel_values=pix, max_new_tokens=max_new)
        cp = cap.plans(cap.bucket(n), R, max_new)
        ops = list(cp.encode_plan.ops)
        got[on] = {"ids": ids.cpu(), "feat": cp.img_feat.t[:n, :, 0, :].double().cpu(), "stages": list(cp.fold_stages),
                   "fold_gemms": sum(1 for op in ops if op.kind == L.OP_CONV and op.i[20] == 2 and op.i[26] > 0 and op.i[27] == 0 and op.i[28] == 0),
                   "v_writes": sum(1 for op in ops if op.kind == L.OP_CONV and op.i[21] == 1 and op.i[13] == 3 * op.i[12]),
                   "new_slots": sum(1 for op in ops if (op.kind == L.OP_CONV and op.i[29]) or (op.kind == L.OP_CHAN_ATTN and op.i[11])
                                    or (op.kind == L.OP_SPLIT_CONVERT and op.i[6]))}
        del cp
        torch.cuda.synchronize()
        cap.clear_plans()
    errs = {on: G.rel_err(v["feat"], ref) for on, v in got.items()}
    print({"img_feat_rel_err_vs_f64": errs, "on_vs_off": G.rel_err(got[True]["feat"], got[False]["feat"])})
    assert got[True]["stages"] == [0, 1, 2] and got[False]["stages"] == [0, 1, 2]
    assert (got[True]["fold_gemms"], got[True]["v_writes"], got[True]["new_slots"]) == (11, 0, 33), got[True]
    assert (got[False]["fold_gemms"], got[False]["v_writes"], got[False]["new_slots"]) == (0, 11, 0), got[False]
    assert torch.equal(got[True]["ids"], got[False]["ids"]), (got[True]["ids"], got[False]["ids"])
    for on, e in errs.items():
        assert e < 2e-5, f"fold_chan_v={on}: img_feat rel err {e:.3e} vs the f64 model"

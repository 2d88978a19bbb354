"""`-m gpu`: visual embeddings and exemplar matching on the MI355X — OMNI_OP_VISUAL_MATCH case by case against f64 (mode 0 from f32
and f16 sources; modes 1 + 2 under the default and a forced split, bit-equal to each other), Florence2Captioner.embed against
transformers in f64 (f32 and f16 plans), the embed plan and the equality of the entry points at 64x64 and at 768x768, the unchanged
defaults, and the public surface (match_elements, track_elements, ScreenParser, Omniparser.find_similar).  Helpers and bounds:
tests/match_checks.py; the host-emulation twin: tests/test_visual_match_emu_cpu.py."""
import pytest
import torch

from omniparser_amd import _lib as L

pytestmark = pytest.mark.gpu
SRC = pytest.mark.parametrize("f16", [False, True])


def _dev():
    import gpu_checks as G
    return G.DEV, G._sync


# ---------------------------------------------------------------------------------------------- kernel, one launch per case
@SRC
def test_embed_rows_vs_f64(f16):
    import match_checks as MC
    dev, sync = _dev()
    MC.check_embed(L, dev, f16, sync=sync)


@SRC
def test_embed_rows_at_layernorm_scale(f16):
    import match_checks as MC
    dev, sync = _dev()
    MC.check_embed(L, dev, f16, sigma=1.0, sync=sync)


@pytest.mark.parametrize("k", [8, 1])
def test_match_vs_f64_under_both_splits(k):
    import match_checks as MC
    dev, sync = _dev()
    MC.check_match(L, dev, k, sync=sync)


@pytest.mark.parametrize("k", [8, 1])
def test_ties_go_to_the_lower_index(k):
    import match_checks as MC
    dev, sync = _dev()
    MC.check_match(L, dev, k, sync=sync, ties=True)


def test_short_gallery_pads_with_minus_one():
    import match_checks as MC
    dev, sync = _dev()
    MC.check_short_gallery(L, dev, sync=sync)


def test_two_query_groups():
    import match_checks as MC
    dev, sync = _dev()
    MC.check_two_groups(L, dev, sync=sync)


def test_odd_width_wide_rows_and_default_slices():
    import match_checks as MC
    dev, sync = _dev()
    MC.check_odd_width(L, dev, sync=sync)


def test_argument_errors():
    import match_checks as MC
    dev, sync = _dev()
    seen = MC.check_argument_errors(L, dev, sync=sync)
    assert all("visual_match" in msg for _, msg in seen), seen


# ---------------------------------------------------------------------------------------------- captioner
@pytest.mark.parametrize("seed", [403, 404, 405, 406])
def test_embed_matches_transformers_f64(seed):
    """4 crops at 64x64, f32 plans: gpu_checks.rel_err against transformers in f64 below the bound the project holds img_feat to"""
    import match_checks as MC
    assert seed in MC.EMBED_SEEDS
    e = MC.embed_vs_f64(MC.captioner(), seed, device_pixels=True)
    assert e < MC.TOL_EMBED_F32, e


def test_embed_f16_plans_match_transformers_f64():
    """f16 plans, the same quantity over the same seeds: each figure is printed, then held to twice the worst value measured on the
    MI355X (match_checks.MEASURED_F16, profiles/visual_match_f16_vs_f64.txt)"""
    import match_checks as MC
    cap = MC.captioner("f16")
    errs = [MC.embed_vs_f64(cap, seed, device_pixels=True) for seed in MC.EMBED_SEEDS]
    print(f"f16 plans vs f64: {errs}")
    assert MC.TOL_EMBED_F16 is not None, "no measured bound recorded in match_checks.MEASURED_F16"
    assert max(errs) <= MC.TOL_EMBED_F16, (errs, MC.TOL_EMBED_F16)


def test_embed_plan_r64():
    import match_checks as MC
    MC.check_embed_plan(MC.captioner(), L, device_pixels=True)


def test_entry_points_agree_r64():
    import match_checks as MC
    MC.check_entry_points(MC.captioner())


def test_embed_plan_and_entry_points_r768():
    """the equality checks at the benched resolution, 2 crops; the plans are dropped afterwards (tens of GB at 768x768)"""
    import match_checks as MC
    cap = MC.captioner("f32", 768)
    try:
        MC.check_embed_plan(cap, L, R=768, n=2, device_pixels=True)
        MC.check_entry_points(cap, R=768, n_boxes=2, beams=False)
    finally:
        torch.cuda.synchronize()
        cap.clear_plans()
        MC._CAPS.pop(("f32", 768), None)


def test_defaults_build_no_embed_plan():
    import match_checks as MC
    MC.check_unchanged_defaults(MC.captioner(), device_pixels=True)


# ---------------------------------------------------------------------------------------------- public surface
def test_public_surface():
    import match_checks as MC
    from omniparser_amd.util import utils as U
    MC.check_public_surface(MC.captioner(), U.FlorenceProcessor(None))


def test_match_on_device_tensors_and_limits():
    """match on device tensors: i64 indices, the f32 scores of the kernel; a leading shape beyond [m, D] is flattened; ValueErrors"""
    import match_checks as MC
    cap = MC.captioner()
    Q, G = MC.match_inputs(9, 70, MC.D_MODEL)
    idx, score = cap.match(Q.cuda(), G.cuda(), top_k=5)
    assert idx.dtype == torch.long and score.dtype == torch.float32 and idx.is_cuda and tuple(idx.shape) == (9, 5)
    MC.check_against_reference(Q, G, 5, idx.cpu().int(), score.cpu(), "Florence2Captioner.match")
    idx3, score3 = cap.match(Q.view(3, 3, -1).cuda(), G.cuda(), top_k=5)
    assert torch.equal(idx3, idx) and torch.equal(score3, score)
    for kw in (dict(top_k=0), dict(top_k=9), dict(top_k=True)):
        with pytest.raises(ValueError):
            cap.match(Q.cuda(), G.cuda(), **kw)
    with pytest.raises(ValueError):
        cap.match(Q.cuda(), G[:, :764].contiguous().cuda())
    with pytest.raises(ValueError):
        cap.match(Q[:0].cuda(), G.cuda())


def test_omniparser_find_similar_agrees_with_match_elements():
    """Omniparser.find_similar = parse + match_elements: the same elements as parse, the same matches as match_elements on them"""
    import base64
    import io
    import os
    import numpy as np
    from PIL import Image
    from omniparser_amd.synth import synthetic_ocr, synthetic_screenshot
    from omniparser_amd.util import utils as U
    from omniparser_amd.util.omniparser import Omniparser
    from tools.make_weights import ensure_blob, ensure_caption_checkpoint

    def b64(arr):
        buf = io.BytesIO()
        Image.fromarray(arr).save(buf, format="PNG")
        return base64.b64encode(buf.getvalue()).decode("ascii")
    os.environ["OMNI_CAPTION_RES"] = "64"
    try:
        cfg = {"som_model_path": str(ensure_blob(seed=0, nc=1, width=0.5)), "caption_model_name": "florence2",
               "caption_model_path": str(ensure_caption_checkpoint(0)), "BOX_TRESHOLD": 0.05,
               "ocr_provider": lambda image: synthetic_ocr(2, image.size[0], image.size[1], 24)}
        img = synthetic_screenshot(2, 1280, 800)
        op = Omniparser(cfg)
        _png, plain = op.parse(b64(img))
        H, W = img.shape[:2]
        px = U.crop_boxes_px([e["bbox"] for e in plain[:2]], W, H)
        assert len(px) == 2
        exemplars = [np.ascontiguousarray(img[y0:y1, x0:x1]) for x0, y0, x1, y1 in px]
        elements, matches = op.find_similar(b64(img), [b64(e) for e in exemplars], top_k=4)
        want = U.match_elements(np.asarray(img), elements, op.caption_model_processor, exemplars, top_k=4)
    finally:
        os.environ.pop("OMNI_CAPTION_RES", None)
    assert elements == plain and matches == want and len(matches) == 2
    import match_checks as MC
    for e, r in enumerate(matches):
        own = [x for x in r if x["index"] == e]
        assert own and own[0]["score"] >= MC.SELF_SCORE and abs(own[0]["score"] - r[0]["score"]) <= MC.SAME_SCORE, (e, r)

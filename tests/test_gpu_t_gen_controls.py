"""`-m gpu`: generation controls of greedy decoding on the MI355X — OMNI_OP_GREEDY_CTRL_STEP at the full vocabulary case by case
against transformers' own logits processors, generate() with each of the seven settings on both stand-in checkpoints against
transformers on the CPU, the plan / default-path rules and the public surface (describe_image, Omniparser).  Helpers and bounds:
tests/gen_ctrl_checks.py; the host-emulation twin: tests/test_gen_controls_emu_cpu.py."""
import base64
import io
import os

import pytest
import torch

from omniparser_amd import _lib as L

pytestmark = pytest.mark.gpu
V_FULL = 51289
BOTH = pytest.mark.parametrize("f16,scores", [(False, False), (False, True), (True, False), (True, True)])


def _dev():
    import gpu_checks as G
    return G.DEV, G._sync


# ---------------------------------------------------------------------------------------------- kernel, one launch per case
@BOTH
def test_repetition_penalty_once_per_seen_token(f16, scores):
    import gen_ctrl_checks as GC
    dev, sync = _dev()
    print(f"worst logp error {GC.check_repetition_penalty(L, dev, V_FULL, f16, scores, sync=sync):.3f} of the bound")


@BOTH
def test_min_new_tokens_on_both_sides_of_the_boundary(f16, scores):
    import gen_ctrl_checks as GC
    dev, sync = _dev()
    GC.check_min_new_tokens(L, dev, V_FULL, f16, scores, sync=sync)


@BOTH
def test_suppress_and_begin_suppress(f16, scores):
    import gen_ctrl_checks as GC
    dev, sync = _dev()
    GC.check_suppress(L, dev, V_FULL, f16, scores, sync=sync)


@BOTH
def test_bad_words(f16, scores):
    import gen_ctrl_checks as GC
    dev, sync = _dev()
    GC.check_bad_words(L, dev, V_FULL, f16, scores, sync=sync)


@BOTH
def test_ngram_size_comes_from_the_block(f16, scores):
    import gen_ctrl_checks as GC
    dev, sync = _dev()
    GC.check_ngram_from_block(L, dev, V_FULL, f16, scores, sync=sync)


@BOTH
def test_everything_at_once_forced_positions_and_finished_rows(f16, scores):
    import gen_ctrl_checks as GC
    dev, sync = _dev()
    GC.check_everything_and_forced(L, dev, V_FULL, f16, scores, sync=sync)


def test_degenerate_rows_neutral_block_and_short_block():
    import gen_ctrl_checks as GC
    dev, sync = _dev()
    GC.check_degenerate_rows(L, dev, V_FULL, sync=sync)
    for f16 in (False, True):
        GC.check_neutral_equals_greedy_step(L, dev, V_FULL, f16, sync=sync)
    seen = GC.check_short_block(L, dev, V_FULL, sync=sync)
    assert all("control block" in m or "allocation" in m for m in seen), seen


# ---------------------------------------------------------------------------------------------- whole captioner
@pytest.mark.parametrize("eos_prone", [False, True])
@pytest.mark.parametrize("name", ["repetition_penalty", "min_new_tokens", "suppress_tokens", "begin_suppress_tokens", "bad_words_ids",
                                  "no_repeat_ngram_size", "all"])
def test_controlled_captions_match_transformers_r64(name, eos_prone):
    """4 crops at 64x64, seed 403, max_new_tokens = 32, f32 plans: ids equal transformers' with the same setting (no row excused),
    token log-probabilities within long_checks.TOL_LOGP_LONG"""
    import gen_ctrl_checks as GC
    GC.captioner_vs_hf(eos_prone, name, device_pixels=True)


def test_reference_outputs_differ_from_the_default():
    import gen_ctrl_checks as GC
    GC.check_not_vacuous()


def test_plans_and_defaults():
    import gen_ctrl_checks as GC
    GC.check_plans_and_defaults(GC.captioner(False), device_pixels=True)


# ---------------------------------------------------------------------------------------------- public surface
def _screenshot_b64(seed=2, W=1280, H=800):
    from PIL import Image
    from omniparser_amd.synth import synthetic_screenshot
    arr = synthetic_screenshot(seed, W, H)
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, format="PNG")
    return arr, base64.b64encode(buf.getvalue()).decode("ascii")


def _omniparser_cfg():
    from omniparser_amd.synth import synthetic_ocr
    from tools.make_weights import ensure_blob, ensure_caption_checkpoint
    return {"som_model_path": str(ensure_blob(seed=0, nc=1, width=0.5)), "caption_model_name": "florence2",
            "caption_model_path": str(ensure_caption_checkpoint(0)), "BOX_TRESHOLD": 0.05,
            "ocr_provider": lambda image: synthetic_ocr(2, image.size[0], image.size[1], 24)}


def test_describe_image_and_omniparser_with_generation_controls():
    """describe_image(generation=...) and Omniparser({"caption_generation": ...}) return batch_decode of the ids that generate /
    caption_crops give with those controls; generation=None / no config key: the elements and the PNG bytes of the call as it was"""
    from PIL import Image
    from omniparser_amd.util import utils as U
    from omniparser_amd.util.omniparser import Omniparser, overlay_style
    arr, b64 = _screenshot_b64()
    cfg = _omniparser_cfg()
    gen = {"repetition_penalty": 1.3, "no_repeat_ngram_size": 2, "min_new_tokens": 8}
    os.environ["OMNI_CAPTION_RES"] = "64"
    try:
        op = Omniparser(cfg)
        opg = Omniparser({**cfg, "caption_generation": gen})
    finally:
        os.environ.pop("OMNI_CAPTION_RES", None)
    cmp_ = op.caption_model_processor
    cap, proc = cmp_["model"], cmp_["processor"]
    img = Image.fromarray(arr)
    # describe
    plain_text = U.describe_image(img, cmp_, task="<CAPTION>", max_new_tokens=48)
    text, ids = U.describe_image(img, cmp_, task="<CAPTION>", max_new_tokens=48, generation=gen, return_ids=True)
    small = img.convert("RGB").resize((64, 64), Image.Resampling.BICUBIC)
    inputs = proc(images=small, text="<CAPTION>", return_tensors="pt", do_resize=False)
    want = cap.generate(input_ids=inputs["input_ids"], pixel_values=inputs["pixel_values"], max_new_tokens=48, **gen)
    assert torch.equal(ids, want[0]) and text == proc.batch_decode(want, skip_special_tokens=True)[0].strip()
    assert text != plain_text
    assert op.describe(b64, task="<CAPTION>", max_new_tokens=48) == plain_text == U.describe_image(img, cmp_, task="<CAPTION>", max_new_tokens=48, generation=None)
    assert op.describe(b64, task="<CAPTION>", max_new_tokens=48, generation=gen) == text == opg.describe(b64, task="<CAPTION>", max_new_tokens=48)
    # parse
    png0, plain = op.parse(b64)
    texts, boxes = op._ocr(img)
    kw = dict(BOX_TRESHOLD=0.05, ocr_bbox=boxes, ocr_text=texts, draw_bbox_config=overlay_style(img.size),
              caption_model_processor=cmp_, output_coord_in_ratio=True, use_local_semantics=True, iou_threshold=0.7, scale_img=False,
              batch_size=128)
    png1, _, elems1 = U.get_som_labeled_img(img, op.som_model, **kw, generation=None)
    assert png1 == png0 and elems1 == plain
    pngg, ctl = opg.parse(b64)
    assert pngg == png0 and len(ctl) == len(plain)
    strip = lambda es: [{k: v for k, v in e.items() if k != "content"} for e in es]
    assert strip(ctl) == strip(plain)
    icon_boxes = [e["bbox"] for e in plain if e["source"] == "box_yolo_content_yolo"]
    assert icon_boxes
    frame = torch.from_numpy(arr).cuda()
    px = U.crop_boxes_px(torch.tensor(icon_boxes).tolist(), arr.shape[1], arr.shape[0])
    got = opg.caption_model_processor["model"].caption_crops(frame, px, controls=gen)
    want = [t.strip() for t in proc.batch_decode(got, skip_special_tokens=True)]
    assert [e["content"] for e in ctl if e["source"] == "box_yolo_content_yolo"] == want
    assert want != [e["content"] for e in plain if e["source"] == "box_yolo_content_yolo"]
    png2, again = op.parse(b64)
    assert png2 == png0 and again == plain

"""`-m gpu`: long-form greedy decoding on the MI355X — the long-history form of OMNI_OP_GREEDY_STEP at the full vocabulary, the
split-key self-attention of OMNI_OP_ATTN_DECODE, generate(max_new_tokens=128) inside the captured step graph against transformers
on the CPU, and the public surface (utils.describe_image, Omniparser.describe, max_new_tokens of get_som_labeled_img / Omniparser).
Helpers, bounds and tolerance: tests/long_checks.py; the host-emulation twin: tests/test_long_decode_emu_cpu.py."""
import base64
import io
import os
import shutil
from pathlib import Path

import pytest
import torch

from omniparser_amd import _lib as L

pytestmark = pytest.mark.gpu
V_FULL = 51289


# ---------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("scores", [False, True])
def test_greedy_step_bans_every_repeated_ngram_of_a_long_history(f16, scores):
    """the emulation test's case at V = 51289: 40 banned followers that are the row's 40 largest logits (a 32-slot list lets the
    last eight through), no ban, a finished row, a repeated follower, ngram 2, forced EOS, ngram 0"""
    import gpu_checks as G
    import long_checks as LC
    worst = LC.check_greedy_long(L, G.DEV, V_FULL, f16, scores, sync=G._sync)
    print(f"f16={f16} scores={scores}: worst logp error {worst:.3f} of the bound")


def test_greedy_step_long_form_degenerate_rows_and_routing_boundary():
    import gpu_checks as G
    import long_checks as LC
    LC.check_degenerate_rows_long(L, G.DEV, V_FULL, sync=G._sync)
    for f16 in (False, True):
        LC.check_routing_boundary(L, G.DEV, V_FULL, f16, sync=G._sync)


@pytest.mark.parametrize("scale", ["unit", "sharp"])
@pytest.mark.parametrize("cap", [65, 130, 1025])
def test_split_key_self_attention_matches_f64(cap, scale):
    import gpu_checks as G
    import long_checks as LC
    worst = LC.check_self_attn(L, G.DEV, L.F32, cap, scale, sync=G._sync)
    print(f"cap={cap} {scale}: worst {worst:.3f} of the bound")


@pytest.mark.parametrize("dtype,ldpad", [("f32", 2), ("f16", 64)])
def test_self_attention_routed_to_the_generic_kernel_keeps_the_bound(dtype, ldpad):
    import gpu_checks as G
    import long_checks as LC
    for scale in ("unit", "sharp"):
        LC.check_self_attn(L, G.DEV, L.F32 if dtype == "f32" else L.F16, 130, scale, ldpad=ldpad, sync=G._sync)


# ---------------------------------------------------------------------------------------------- whole captioner
def test_long_captions_match_transformers_r64_full_length():
    """case 1: 4 crops, stock EOS, max_new_tokens = 128: every row runs to full length and has more than 32 banned tokens from
    position 101 on; no row excused"""
    import long_checks as LC
    cap, out, worst, ref = LC.captioner_long_vs_hf(1, device_pixels=True)
    assert out.sequences.shape[1] == 129 and cap.last_steps == 128
    cp = cap.plans(cap.bucket(4), 64, 128, scores=True)
    assert cp.T == 129 and tuple(cp.self_k[0].t.shape[:2]) == (cp.B, 129)
    assert cap.plan_cache_bytes() >= 2 * cp.B * 129 * cap.w.d_model * 4 * 2 * cap.w.dec_layers      # both long plans are counted


def test_long_captions_match_transformers_r64_eos_prone():
    """case 2: EOS-prone checkpoint: rows end at several lengths, the early-exit poll stops the long plan"""
    import long_checks as LC
    cap, out, worst, ref = LC.captioner_long_vs_hf(2, device_pixels=True)
    assert cap.last_steps < 128 and out.sequences.shape[1] == ref.shape[1]


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


def test_describe_image_and_omniparser_describe(tmp_path):
    """describe_image(task="<CAPTION>", max_new_tokens=64) on a 1280x800 screenshot = batch_decode(generate(processor(Pillow-resized
    image))); Omniparser.describe gives the same string; with the golden tokenizer next to the processor <MORE_DETAILED_CAPTION>
    runs and its ids are transformers' for the same prompt"""
    import prompt_checks as P
    from PIL import Image
    from omniparser_amd.util import utils as U
    from omniparser_amd.util.omniparser import Omniparser
    from tools.make_weights import shared_random_captioner
    arr, b64 = _screenshot_b64()
    os.environ["OMNI_CAPTION_RES"] = "64"
    try:
        op = Omniparser(_omniparser_cfg())
    finally:
        os.environ.pop("OMNI_CAPTION_RES", None)
    cmp_ = op.caption_model_processor
    cap, proc = cmp_["model"], cmp_["processor"]
    img = Image.fromarray(arr)
    text = U.describe_image(img, cmp_, task="<CAPTION>", max_new_tokens=64)
    small = img.convert("RGB").resize((64, 64), Image.Resampling.BICUBIC)
    inputs = proc(images=small, text="<CAPTION>", return_tensors="pt", do_resize=False)
    ids = cap.generate(input_ids=inputs["input_ids"], pixel_values=inputs["pixel_values"], max_new_tokens=64)
    assert isinstance(text, str) and text == proc.batch_decode(ids, skip_special_tokens=True)[0].strip()
    assert ids.shape[1] > 21                                   # longer than the 20-token plans could give
    assert op.describe(b64, task="<CAPTION>", max_new_tokens=64) == text
    assert U.describe_image([img, arr], cmp_, task="<CAPTION>", max_new_tokens=64) == [text, text]
    t2, ids2 = U.describe_image(img, cmp_, task="<CAPTION>", max_new_tokens=64, return_ids=True)
    assert t2 == text and torch.equal(ids2, ids[0])
    with pytest.raises(ValueError, match="tokenizer.json"):
        U.describe_image(img, cmp_)                            # the default task needs the tokenizer
    with pytest.raises(ValueError, match="1024"):
        U.describe_image(img, cmp_, task="<CAPTION>", max_new_tokens=1025)
    # with a tokenizer: the task sentence as the prompt, token-exact against transformers
    shutil.copy(Path(__file__).resolve().parent / "golden" / "tokenizer_synth" / "tokenizer.json", tmp_path / "tokenizer.json")
    proc_t = U.FlorenceProcessor(tmp_path, image_token_id=proc.image_token_id, special_ids=(cap.w.bos, cap.w.pad, cap.w.eos, 3))
    _, got = U.describe_image(img, {"model": cap, "processor": proc_t}, task="<MORE_DETAILED_CAPTION>", max_new_tokens=64, return_ids=True)
    row = proc_t.prompt_ids("<MORE_DETAILED_CAPTION>")
    ref, margins = P.oracle_generate(shared_random_captioner(0), inputs["pixel_values"], [row], max_new=64)
    print(f"<MORE_DETAILED_CAPTION>: {got.shape[0] - 1} tokens, oracle margin {margins[0]:.3e}")
    P.assert_margins(margins, "describe")
    assert P._trim(got) == P._trim(ref[0]), (got.tolist(), ref[0].tolist())


def test_caption_max_new_tokens_through_get_som_labeled_img_and_omniparser():
    """max_new_tokens=None / no config key: the elements and the PNG of the call as it was; caption_max_new_tokens=40: captions whose
    first 20 generated ids are the default call's wherever that did not end on its forced EOS"""
    from PIL import Image
    from omniparser_amd.util import utils as U
    from omniparser_amd.util.omniparser import Omniparser, overlay_style
    arr, b64 = _screenshot_b64()
    cfg = _omniparser_cfg()
    os.environ["OMNI_CAPTION_RES"] = "64"
    try:
        op = Omniparser(cfg)
        op40 = Omniparser({**cfg, "caption_max_new_tokens": 40})
    finally:
        os.environ.pop("OMNI_CAPTION_RES", None)
    png0, plain = op.parse(b64)
    img = Image.fromarray(arr)
    texts, boxes = op._ocr(img)
    kw = dict(BOX_TRESHOLD=0.05, ocr_bbox=boxes, ocr_text=texts, draw_bbox_config=overlay_style(img.size),
              caption_model_processor=op.caption_model_processor, output_coord_in_ratio=True, use_local_semantics=True,
              iou_threshold=0.7, scale_img=False, batch_size=128)
    png1, _, elems1 = U.get_som_labeled_img(img, op.som_model, **kw, max_new_tokens=None)
    png2, _, elems2 = U.get_som_labeled_img(img, op.som_model, **kw, max_new_tokens=20)
    assert png1 == png0 == png2 and elems1 == plain == elems2
    png40, long = op40.parse(b64)
    assert png40 == png0 and len(long) == len(plain)
    assert [{k: v for k, v in e.items() if k != "content"} for e in long] == [{k: v for k, v in e.items() if k != "content"} for e in plain]
    # the ids behind the captions: 20 vs 40 new tokens on the same crops
    cap = op.caption_model_processor["model"]
    icon_boxes = [e["bbox"] for e in plain if e["source"] == "box_yolo_content_yolo"]
    assert icon_boxes
    frame = torch.from_numpy(arr).cuda()
    px = U.crop_boxes_px(torch.tensor(icon_boxes).tolist(), arr.shape[1], arr.shape[0])      # f32 ratios, as get_parsed_content_icon sees them
    a, b = cap.caption_crops(frame, px, max_new_tokens=20), cap.caption_crops(frame, px, max_new_tokens=40)
    free = 0
    for ra, rb in zip(a, b):
        ra = ra.tolist() + [cap.w.pad] * (21 - a.shape[1])
        rb = torch.tensor(rb.tolist() + [cap.w.pad] * (21 - b.shape[1]))
        ended_on_forced_eos = ra[20] == cap.w.eos and cap.w.eos not in ra[1:20]
        n = 20 if ended_on_forced_eos else 21
        assert rb.tolist()[:n] == ra[:n], (ra, rb.tolist())
        free += not ended_on_forced_eos
    print(f"{len(px)} icons, {free} ended before the 20-token limit")
    proc = op.caption_model_processor["processor"]
    want = [t.strip() for t in proc.batch_decode(b, skip_special_tokens=True)]
    assert [e["content"] for e in long if e["source"] == "box_yolo_content_yolo"] == want

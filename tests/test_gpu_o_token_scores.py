"""`-m gpu`: per-token log-probabilities of greedy decoding on the MI355X — OMNI_OP_GREEDY_STEP p4 against an f64 log-softmax of
transformers' processed scores at the full vocabulary, Florence2Captioner.generate(output_scores=True) against transformers'
generate(output_scores=True) + compute_transition_scores(normalize_logits=True) on the CPU, and the caption confidence through
ScreenParser.parse_batch / parse_stream (merged decode) and the Omniparser facade.  Helpers, bound and tolerance:
tests/score_checks.py; the host-emulation twin: tests/test_token_scores_emu_cpu.py."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("B", [4, 130])
def test_greedy_step_token_logprobs_match_f64_full_vocab(B, f16):
    """V = 51289 (no multiple of 256), B = 4 and B = 130 blocks, ngram 3, forced tokens and bias: the kernel case of the emulation test
    with the same f64 reference and bound; 6 steps, so that the n-gram ban removes a row's largest logit from the sum"""
    import gpu_checks as G
    import score_checks as SC
    from omniparser_amd import _lib as L
    r = SC.check_kernel_case(L, G.DEV, B, 51289, 6, 3, True, True, f16, seed=B + f16, sync=G._sync)
    print(f"B={B} f16={f16}: max err {r['max_err']:.3e} = {r['max_bound_ratio']:.3f} of the bound")
    assert r["banned_max"] >= 1 and r["finished_early"] >= 1 and r["unfinished"] >= 1, r
    SC.check_degenerate_rows(L, G.DEV, G._sync)


def test_captioner_token_logprobs_match_transformers_r64():
    """8 seeded 64x64 crops, max_new_tokens=20, EOS-prone checkpoint (rows end at several lengths): token_logprobs within
    score_checks.TOL_LOGP of transformers on the CPU up to each row's EOS; sequences bit-equal to generate() without scores"""
    import score_checks as SC
    cap, pix, out, _ = SC.captioner_vs_hf(8, 211, True, 20, device_pixels=True)
    assert torch.equal(cap.generate(pixel_values=pix, max_new_tokens=20), out.sequences)
    assert bool((out.token_logprobs <= 0).all())


@pytest.fixture(scope="module")
def models():
    from omniparser_amd.florence import Florence2Captioner
    from omniparser_amd.util.yolov9 import YOLOv9Detector
    from tools.make_weights import ensure_blob, ensure_caption_checkpoint
    det = YOLOv9Detector(model_path=ensure_blob(seed=0, nc=1, width=0.5), device="cuda", precision="f32")
    cap = Florence2Captioner(ensure_caption_checkpoint(0), "cuda", precision="f32", resolution=64)
    return det, cap


def _without_confidence(elems):
    return [[{k: v for k, v in e.items() if k != "confidence"} for e in f] for f in elems]


def _confidences(elems):
    return [[e.get("confidence") for e in f] for f in elems]


def _close(a, b, tol):
    return (a is None and b is None) or (a is not None and b is not None and abs(math.log(a) - math.log(b)) <= tol)


def test_parse_batch_and_stream_confidence_on_the_merged_decode(models):
    """one synthetic 1080p frame, batch_size = 8: its crops take the merged decode.  return_confidence=True changes nothing but the
    new key; every confidence is caption_confidence of caption_crops(return_scores=True) on the same crop (a mean of log-probabilities,
    so the model tolerance applies to its logarithm); parse_stream over two such batches and return_image=True give the same"""
    import score_checks as SC
    from omniparser_amd.florence import caption_confidence
    from omniparser_amd.pipeline import ScreenParser
    from omniparser_amd.synth import synthetic_ocr, synthetic_screenshot
    det, cap = models
    sp = ScreenParser(det, cap, box_threshold=0.05, iou_threshold=0.7, nms_iou=0.1, max_det=300, imgsz=640, batch_size=8)
    W, H = 1920, 1080
    frames = [torch.from_numpy(synthetic_screenshot(7, W, H)).cuda()]
    ocr = [synthetic_ocr(7, W, H, 40)]
    plain = sp.parse_batch(frames, ocr)
    got, ids = sp.parse_batch(frames, ocr, return_ids=True, return_confidence=True)
    crops = sp.last_crops[0]
    assert len(crops) > 8 and any(k[0] == "dec" and k[-1] == "scores" for k in cap._plans)        # the merged decode ran
    assert _without_confidence(got) == plain
    captioned = [e for e in got[0] if e["source"] == "box_yolo_content_yolo"]
    assert len(captioned) == len(crops) == len(ids[0])
    assert all("confidence" not in e for e in got[0] if e["source"] != "box_yolo_content_yolo")
    assert any(e["source"] != "box_yolo_content_yolo" for e in got[0])
    c_ids, c_logp = cap.caption_crops(frames[0], crops, return_scores=True)
    w = cap.w
    want = [caption_confidence(r, lp, w.eos, w.forced_bos, w.forced_eos, 20) for r, lp in zip(c_ids, c_logp)]
    have = [e["confidence"] for e in captioned]
    same_ids = [r.tolist() == c[:len(r)].tolist() for r, c in zip(ids[0], c_ids)]
    worst = max(abs(math.log(a) - math.log(b)) for a, b, s in zip(have, want, same_ids) if s)
    print(f"{len(crops)} crops, {sum(same_ids)} with the ids of caption_crops, max |dlog confidence| = {worst:.3e}, "
          f"confidence range {min(have):.4f} .. {max(have):.4f}")
    assert all(same_ids)
    assert all(isinstance(c, float) and 0.0 < c <= 1.0 for c in have)
    assert all(_close(a, b, SC.TOL_LOGP) for a, b in zip(have, want))
    # the pipelined stream, two such batches
    streamed = list(sp.parse_stream([(frames, ocr), (frames, ocr)], return_confidence=True))
    assert len(streamed) == 2
    for res in streamed:
        assert _without_confidence(res) == plain
        assert all(_close(a, b, SC.TOL_LOGP) for a, b in zip(_confidences(res)[0], _confidences(got)[0]))
    # together with the annotated image
    el_img, marked = sp.parse_batch(frames, ocr, return_image=True, return_confidence=True)
    el_plain, marked_plain = sp.parse_batch(frames, ocr, return_image=True)
    assert el_img == got and el_plain == plain and marked[0][0] == marked_plain[0][0]
    sp.release_annotate_scratch()


def test_omniparser_caption_confidence():
    """Omniparser with caption_confidence=True: captioned icons carry a float in (0, 1], OCR elements and icons with OCR text no such
    key; without the key the output is what it always was"""
    import base64
    import io
    import os
    from PIL import Image
    from omniparser_amd.synth import synthetic_ocr, synthetic_screenshot
    from omniparser_amd.util.omniparser import Omniparser
    from tools.make_weights import ensure_blob, ensure_caption_checkpoint
    os.environ["OMNI_CAPTION_RES"] = "64"
    try:
        cfg = {"som_model_path": str(ensure_blob(seed=0, nc=1, width=0.5)), "caption_model_name": "florence2",
               "caption_model_path": str(ensure_caption_checkpoint(0)), "BOX_TRESHOLD": 0.05,
               "ocr_provider": lambda image: synthetic_ocr(2, image.size[0], image.size[1], 24)}
        buf = io.BytesIO()
        Image.fromarray(synthetic_screenshot(2, 1280, 800)).save(buf, format="PNG")
        b64 = base64.b64encode(buf.getvalue()).decode("ascii")
        png0, plain = Omniparser(cfg).parse(b64)
        op = Omniparser({**cfg, "caption_confidence": True})
        assert op.caption_model_processor["model"].token_scores is True
        png1, scored = op.parse(b64)
        with pytest.raises(ValueError):
            Omniparser({**cfg, "caption_confidence": 1})
    finally:
        os.environ.pop("OMNI_CAPTION_RES", None)
    assert all("confidence" not in e for e in plain)
    assert _without_confidence([scored])[0] == plain and png1 == png0
    icons = [e for e in scored if e["source"] == "box_yolo_content_yolo"]
    assert icons and all(isinstance(e["confidence"], float) and 0.0 < e["confidence"] <= 1.0 for e in icons)
    others = [e for e in scored if e["source"] != "box_yolo_content_yolo"]
    assert others and all("confidence" not in e for e in others)

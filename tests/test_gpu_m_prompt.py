"""`-m gpu`: the caller's prompt in the Florence-2 captioner on the MI355X — OMNI_OP_ASSEMBLE's device gather, the per-row key counts
of the encoder self-attention (OMNI_OP_ATTN_ROWS p7) and the decoder cross-attention (OMNI_OP_ATTN_DECODE p7) inside the captured
graphs, against transformers on the CPU (tests/prompt_checks.py: prompts, margin rule), and the prompt through ScreenParser.
Reference calls being replaced: ref:util/utils.py:88-132 (`get_parsed_content_icon(..., prompt=)` -> `processor(text=[prompt] * n)`
-> `model.generate(input_ids=...)`)."""
import pytest
import torch

from omniparser_amd import _lib as L

pytestmark = pytest.mark.gpu


def test_prompt_kernels_on_device():
    """the new op slots at the plans' shapes (S = 13, 69, 641), all kernels that serve them, against f64 inside the guard bands of
    tests/caption_f64.py; a full table is bit-identical to no table"""
    import prompt_checks as P
    for dtype in (L.F32, L.F16):
        P.check_assemble_gather(dtype)
        for D, tile in ((32, 48), (64, 64 if dtype == L.F32 else 32)):
            for n_img, n_txt, heads, groups in ((5, 8, 12, 4), (5, 64, 12, 5), (577, 64, 12, 3)):
                P.check_attn_rows_masked(dtype, D, heads, n_img, n_txt, groups, tile)
        for aligned in ((True, False) if dtype == L.F32 else (True,)):
            for kv_div in (1, 3):
                for n_img, n_txt, heads, crops in ((5, 8, 12, 4), (5, 64, 12, 5), (577, 64, 12, 3)):
                    P.check_attn_decode_cross_masked(dtype, heads, n_img, n_txt, crops, kv_div, aligned)


@pytest.mark.parametrize("R", [64, 768])
def test_uniform_prompts_token_exact(R):
    """two non-default prompts of different text capacities on real crops, f32, token-exact against transformers; no crop below
    the margin (asserted on the oracle's own margins)"""
    import prompt_checks as P
    out, _ = P.check_uniform_prompts(R)
    print(out)


def test_ragged_batch_token_exact_and_equal_solo():
    """16 prompts of 5 .. 64 tokens in one batch at R = 64 (capacity 64, attention mask): transformers' ids, and every row equals
    its solo run"""
    import prompt_checks as P
    out, _ = P.check_ragged_batch()
    print(out)


def _parser(R, max_det):
    from omniparser_amd.florence import Florence2Captioner
    from omniparser_amd.pipeline import ScreenParser
    from omniparser_amd.util.yolov9 import YOLOv9Detector
    from tools.make_weights import ensure_blob, ensure_caption_checkpoint
    det = YOLOv9Detector(model_path=ensure_blob(seed=0, nc=1, width=1.0), device="cuda", precision="f32")
    cap = Florence2Captioner(ensure_caption_checkpoint(0), "cuda", precision="f32", resolution=R)
    return ScreenParser(det, cap, box_threshold=0.05, iou_threshold=0.7, nms_iou=0.1, max_det=max_det, imgsz=640), cap


def _frames(seeds):
    from omniparser_amd.synth import synthetic_ocr, synthetic_screenshot
    imgs = [synthetic_screenshot(s, 1920, 1080) for s in seeds]
    return [torch.from_numpy(a).cuda() for a in imgs], [synthetic_ocr(s, 1920, 1080, 40) for s in seeds]


def _lists(ids):
    return [[[int(v) for v in r] for r in f] for f in ids]


def test_parse_batch_prompt_equals_caption_crops():
    """parse_batch(prompt=ids) gives, crop by crop, what caption_crops(prompt_ids=ids) gives on the crop rectangles it reports (one
    frame, at most 96 crops: both run the same plan of one micro-batch, bit for bit); the prompt changes the captions; a prompt
    given as text goes through the parser's processor"""
    import prompt_checks as P
    sp, cap = _parser(64, 96)
    frames, ocr = _frames((3,))
    prompt = P.PROMPTS[29]
    _, ids_d = sp.parse_batch(frames, ocr, return_ids=True)
    _, ids_p = sp.parse_batch(frames, ocr, return_ids=True, prompt=prompt)
    crops = sp.last_crops[0]
    assert 16 <= len(crops) <= 96, len(crops)
    want = cap.caption_crops(frames[0], crops, prompt_ids=prompt)
    got = _lists(ids_p)[0]
    assert len(got) == len(crops)
    for k, row in enumerate(got):
        assert P._trim(torch.tensor(row)) == P._trim(want[k]), (k, row, want[k].tolist())
    changed = sum(a != b for a, b in zip(got, _lists(ids_d)[0]))
    assert changed > len(crops) // 2, f"the prompt changed {changed} of {len(crops)} captions"
    from omniparser_amd.florence import PROMPT_IDS
    assert sp.prompt_ids("<CAPTION>") == PROMPT_IDS and sp.prompt_ids(None) is None          # text goes through the parser's processor
    _, ids_c = sp.parse_batch(frames, ocr, return_ids=True, prompt="<CAPTION>")
    assert _lists(ids_c) == _lists(ids_d)
    assert L.overflow_count() == 0


def test_parse_stream_prompt_equals_parse_batch():
    """the pipelined stream with a prompt (two encode lanes, exact-row twins of the remainder micro-batch, merged decode with the
    merged key-count table on its own stream) reproduces parse_batch(prompt=) on every crop of three batches of four frames"""
    import prompt_checks as P
    sp, cap = _parser(64, 300)
    frames, ocr = _frames((3, 4, 5, 6))
    prompt = P.PROMPTS[11]
    elems, ids = sp.parse_batch(frames, ocr, return_ids=True, prompt=prompt)
    crops = sp.last_crops
    assert sum(len(c) for c in crops) > 128, [len(c) for c in crops]           # more than one micro-batch: the merged decode path
    _, ids_d = sp.parse_batch(frames, ocr, return_ids=True)
    assert _lists(ids) != _lists(ids_d)
    n = 0
    for el_s, ids_s in sp.parse_stream(iter([(frames, ocr)] * 3), return_ids=True, prompt=prompt):
        assert sp.last_crops == crops and el_s == elems
        bad = sum(a != b for fa, fb in zip(_lists(ids_s), _lists(ids)) for a, b in zip(fa, fb))
        assert bad == 0, f"batch {n}: {bad} crops differ from parse_batch"
        n += 1
    assert n == 3
    # the default prompt afterwards: the stream's default plans, the ids parse_batch gave without a prompt
    for el_s, ids_s in sp.parse_stream(iter([(frames, ocr)]), return_ids=True):
        assert _lists(ids_s) == _lists(ids_d)
    assert L.overflow_count() == 0


def test_default_prompt_unchanged():
    """generate(input_ids=<the default ids>), generate() and caption_crops() run the same default plan: identical ids, no plan with
    a text capacity is built, the split-f16 range guard stays silent"""
    import prompt_checks as P
    from omniparser_amd.florence import PROMPT_IDS, Florence2Captioner
    from tools.make_weights import ensure_caption_checkpoint, shared_random_captioner
    R, n = 64, 16
    pix, img, boxes = P.real_pixels(R, n)
    cap = Florence2Captioner(ensure_caption_checkpoint(0), "cuda", precision="f32", resolution=R)
    ids, mask = P.hf_inputs(shared_random_captioner(0), R, [PROMPT_IDS] * n)
    a = cap.generate(pixel_values=pix.cuda(), max_new_tokens=20)
    b = cap.generate(input_ids=ids, pixel_values=pix.cuda(), max_new_tokens=20)
    c = cap.generate(input_ids=ids, attention_mask=mask, pixel_values=pix.cuda(), max_new_tokens=20)
    frame = torch.from_numpy(img).cuda()
    d = cap.caption_crops(frame, boxes)
    e = cap.caption_crops(frame, boxes, prompt_ids=PROMPT_IDS)
    assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, d) and torch.equal(d, e)
    assert all(not (isinstance(k[-1], tuple) and k[-1][:1] == ("txt",)) for k in cap._plans), list(cap._plans)
    cp = cap.plans(cap.bucket(n), R, 20)
    assert cp.nkeys is None and cp.prompt_ids is None
    assert L.overflow_count() == 0

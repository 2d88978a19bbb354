"""Beam-search decoding of the captioner on the MI355X (OMNI_OP_BEAM_STEP + the position-table / shared-cross-K/V forms of
OMNI_OP_ATTN_DECODE, inside the captured step graph) against transformers' generate(num_beams=3) on the CPU, under the margin rule of
tests/beam_checks.py; caption_crops / ScreenParser / Omniparser with beams; early exit on the frozen flags."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _gen_vs_hf(R, n, seed, eos_prone, nrs=1, max_new=20):
    import beam_checks as BC
    from omniparser_amd.florence import Florence2Captioner
    from tools.make_weights import ensure_caption_checkpoint
    pix = torch.randn(n, 3, R, R, generator=torch.Generator().manual_seed(seed))
    model = BC.oracle_model(0, eos_prone)
    try:
        ref, rep = BC.hf_generate_beams(model, pix, 3, max_new, nrs=nrs)
    finally:
        model.generation_config.eos_token_id = 2
    d = BC.eos_prone_checkpoint(0) if eos_prone else ensure_caption_checkpoint(0)
    cap = Florence2Captioner(d, "cuda", precision="f32", resolution=R)
    out = cap.generate(pixel_values=pix.cuda(), max_new_tokens=max_new, num_beams=3, num_return_sequences=nrs,
                       return_dict_in_generate=True)
    n_c, below, failures = BC.compare_crops(out.sequences, out.sequences_scores, ref.sequences, ref.sequences_scores, rep.gaps, nrs,
                                            cap.w.pad, 1e-4)
    print(f"R={R} eos_prone={eos_prone} nrs={nrs}: {n_c} crops compared, {below} below the margin, hf lengths "
          f"{sorted(rep.lengths[:, 0].tolist())}")
    assert not failures, failures[:3]
    return cap, pix, out


@pytest.mark.parametrize("eos_prone", [False, True])
def test_beam_generate_matches_transformers_r64(eos_prone):
    _gen_vs_hf(64, 32, 101, eos_prone)


def test_beam_generate_num_return_sequences_r64():
    _gen_vs_hf(64, 8, 102, True, nrs=3)


def test_beam_generate_matches_transformers_r768():
    _gen_vs_hf(768, 4, 103, False)


def _crop_pixels(cap, frame_dev, boxes):
    """the device-preprocessed pixels of every crop (OMNI_OP_CROP_RESIZE into a plan's input), NCHW on the device"""
    import gpu_checks as G
    out = []
    for s in range(0, len(boxes), 128):
        chunk = boxes[s:s + 128]
        cp = cap.plans(cap.bucket(len(chunk)), cap.resolution, 20)
        G._fill_rows(cap, cp, frame_dev, chunk, list(range(len(chunk))))
        out.append(cp.x_in.t[:len(chunk), :, :, :3].permute(0, 3, 1, 2).float().clone())
    return torch.cat(out)


def _strip(row, pad):
    row = list(row)
    while row and row[-1] == pad:
        row.pop()
    return row


def test_caption_crops_and_merged_decode_equal_generate():
    """caption_crops(num_beams=3) returns, crop for crop, the best hypothesis generate(num_beams=3) returns on the same pixels (same
    plans: bit for bit), a repeated call (graph replay) the same ids.  ScreenParser.caption with cap.num_beams = 3 decodes the 141
    crops in ONE merged plan (128 + a remainder micro-batch, 160 x 3 decoder rows): the split-K choice of its step GEMMs depends on
    the row count, so the last bits of its logits differ from the 128 x 3-row plans of generate and near-ties of the beam scores may
    resolve differently — a few crops may differ, the rest must agree; the merged path must be deterministic over repeats."""
    import gpu_checks as G
    from omniparser_amd.florence import Florence2Captioner
    from omniparser_amd.pipeline import ScreenParser
    from omniparser_amd.synth import synthetic_screenshot
    from tools.make_weights import ensure_caption_checkpoint
    cap = Florence2Captioner(ensure_caption_checkpoint(0), "cuda", precision="f32", resolution=64)
    frame = torch.from_numpy(synthetic_screenshot(5)).cuda()
    boxes = G.real_crop_boxes(5, 141)
    want = cap.generate(pixel_values=_crop_pixels(cap, frame, boxes), num_beams=3)
    got = cap.caption_crops(frame, boxes, num_beams=3)
    assert torch.equal(got, want)
    assert torch.equal(cap.caption_crops(frame, boxes, num_beams=3), got)
    greedy = cap.caption_crops(frame, boxes)
    assert not torch.equal(greedy[:, :want.shape[1]], want[:, :greedy.shape[1]])     # beams change the captions of this model
    cap.num_beams = 3
    sp = ScreenParser(None, cap)
    runs = []
    for _ in range(2):
        rows = [_strip(r.tolist(), cap.w.pad) for _, r in sp.caption([frame], [boxes])[0]]
        assert len(rows) == len(boxes)
        runs.append(rows)
    assert runs[0] == runs[1]
    differ = sum(r != _strip(w.tolist(), cap.w.pad) for r, w in zip(runs[0], want))
    print(f"merged decode vs generate: {differ} of {len(boxes)} crops differ")
    assert differ <= len(boxes) // 20


def test_beam_early_exit_on_frozen_flags():
    """EOS-prone checkpoint: every crop's search freezes before max_new_tokens, so generate issues fewer step replays — with the same
    ids as a run of all max_new_tokens steps (early_exit_every = 0)"""
    import beam_checks as BC
    from omniparser_amd.florence import Florence2Captioner
    cap = Florence2Captioner(BC.eos_prone_checkpoint(0), "cuda", precision="f32", resolution=64)
    pool = torch.randn(16, 3, 64, 64, generator=torch.Generator().manual_seed(3)).cuda()
    quick = []
    for i in range(16):                                  # crops whose own search freezes early
        cap.generate(pixel_values=pool[i:i + 1], max_new_tokens=20, num_beams=3)
        if cap.last_steps < 20:
            quick.append(i)
    assert len(quick) >= 2, quick
    pix = pool[quick]
    out = cap.generate(pixel_values=pix, max_new_tokens=20, num_beams=3, return_dict_in_generate=True)
    early = cap.last_steps
    cap.early_exit_every = 0
    full = cap.generate(pixel_values=pix, max_new_tokens=20, num_beams=3, return_dict_in_generate=True)
    assert cap.last_steps == 20
    print(f"early exit after {early} of 20 steps")
    assert early < 20
    assert torch.equal(out.sequences, full.sequences) and torch.equal(out.sequences_scores, full.sequences_scores)


def test_omniparser_caption_num_beams():
    """Omniparser with caption_num_beams=3 parses a frame with beam captions; the same frame without the key is exactly today's
    greedy output"""
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
        _, greedy = Omniparser(cfg).parse(b64)
        op_beam = Omniparser({**cfg, "caption_num_beams": 3})
        assert op_beam.caption_model_processor["model"].num_beams == 3
        _, beams = op_beam.parse(b64)
        _, greedy2 = Omniparser(cfg).parse(b64)
        with pytest.raises(ValueError):
            Omniparser({**cfg, "caption_num_beams": 9})
    finally:
        os.environ.pop("OMNI_CAPTION_RES", None)
    assert greedy2 == greedy
    assert [(e["type"], e["bbox"], e["source"]) for e in beams] == [(e["type"], e["bbox"], e["source"]) for e in greedy]
    icons = [i for i, e in enumerate(greedy) if e["source"] == "box_yolo_content_yolo"]
    assert icons and any(beams[i]["content"] != greedy[i]["content"] for i in icons)

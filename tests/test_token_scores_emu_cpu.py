"""Per-token log-probabilities of greedy decoding (OMNI_OP_GREEDY_STEP p4, Florence2Captioner.generate(output_scores=True),
caption_crops(return_scores=True), florence.caption_confidence, ScreenParser / Omniparser confidence) on the host emulation of the HIP
kernels (tests/emu): the kernel against an f64 log-softmax of transformers' processed scores, the captioner against transformers'
generate(output_scores=True) + compute_transition_scores(normalize_logits=True).  Helpers, bound and tolerance: tests/score_checks.py."""
import itertools
import math
import re
from pathlib import Path

import pytest
import torch

from omniparser_amd import _lib as L

KERNEL_CASES = list(itertools.product((2003, 51289), (3, 0), (True, False), (True, False), (False, True)))


@pytest.mark.parametrize("V,ngram,forced,with_bias,f16", KERNEL_CASES)
def test_greedy_step_token_logprobs_match_f64(emu, V, ngram, forced, with_bias, f16):
    """B = 6, T = 17: 16 steps of scripted logits (3 at the full vocabulary) — logp within the derived bound of the f64 log-softmax of
    the processed row at the chosen id, 0.0 at forced positions, behind a row's EOS and in column 0; ids / finished / step bit-equal
    to the p4 = NULL run and equal to transformers' greedy ids; rows finish at several lengths and some never do."""
    import score_checks as SC
    steps = 16 if V == 2003 else 3
    r = SC.check_kernel_case(L, torch.device("cpu"), 6, V, steps, ngram, forced, with_bias, f16, seed=V % 1000 + 10 * ngram + forced)
    print(f"V={V} ngram={ngram} forced={forced} bias={with_bias} f16={f16}: max err {r['max_err']:.3e} = {r['max_bound_ratio']:.3f} "
          f"of the bound, {r['banned_max']} steps with the largest logit banned")
    if ngram and steps == 16:
        assert r["banned_max"] >= 1                    # the sum did leave out a banned maximum
    assert r["finished_early"] >= 1 and r["unfinished"] >= 1, r


def test_greedy_step_degenerate_rows_with_scores(emu):
    import score_checks as SC
    SC.check_degenerate_rows(L, torch.device("cpu"))


@pytest.mark.parametrize("eos_prone", [False, True])
def test_captioner_token_logprobs_match_transformers_r64(emu, eos_prone):
    """generate(output_scores=True, return_dict_in_generate=True, max_new_tokens=4) on 2 crops at 64x64 vs transformers; sequences
    bit-equal to generate() without scores; the default plan's greedy op has p4 = NULL, as many ops as the scores plan, and is
    another cache entry."""
    import score_checks as SC
    cap, pix, out, _ = SC.captioner_vs_hf(2, 31, eos_prone, 4)
    plain = cap.generate(pixel_values=pix, max_new_tokens=4)
    assert torch.equal(plain, out.sequences)
    p0 = cap.plans(cap.bucket(2), 64, 4)
    p1 = cap.plans(cap.bucket(2), 64, 4, scores=True)
    assert p0 is not p1 and len(cap._plans) == 2 and p0.logp is None and tuple(p1.logp.shape) == (p1.B, 5)
    g0 = [op for op in p0.step_plan.ops if op.kind == L.OP_GREEDY_STEP]
    g1 = [op for op in p1.step_plan.ops if op.kind == L.OP_GREEDY_STEP]
    assert len(g0) == len(g1) == 1 and g0[0].p[4] is None and g1[0].p[4] == p1.logp.data_ptr()
    assert len(p0.step_plan.ops) == len(p1.step_plan.ops)
    assert [op.kind for op in p0.step_plan.ops] == [op.kind for op in p1.step_plan.ops]
    if eos_prone:
        return
    # caption_crops hands the same numbers out, and caption_confidence reads them (once: every call is an emulated encode)
    from omniparser_amd.florence import caption_confidence
    frame = torch.randint(0, 255, (96, 128, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1))
    boxes = [[3, 5, 40, 44], [50, 10, 120, 90]]
    ids, logp = cap.caption_crops(frame, boxes, max_new_tokens=4, return_scores=True)
    assert torch.equal(ids, cap.caption_crops(frame, boxes, max_new_tokens=4))
    assert tuple(logp.shape) == (2, ids.shape[1] - 1) and bool((logp <= 0).all())
    cap.token_scores = True
    ids2, logp2 = cap.caption_crops(frame, boxes, max_new_tokens=4)
    assert torch.equal(ids2, ids) and torch.equal(logp2, logp)
    w = cap.w
    for r, lp in zip(ids, logp):
        c = caption_confidence(r, lp, w.eos, w.forced_bos, w.forced_eos, 4)
        assert c is not None and 0.0 < c <= 1.0


def test_screen_parser_confidence_merged_and_single(emu, monkeypatch):
    """ScreenParser.caption(scores=True): (text, ids, confidence) per crop on the merged decode and on the per-micro-batch decode,
    the ids those paths return without scores; the merged batch's encode-only plans are the ones it always used"""
    from conftest import small_vocab_caption_checkpoint
    from omniparser_amd.florence import Florence2Captioner
    from omniparser_amd.pipeline import ScreenParser
    from omniparser_amd.synth import synthetic_screenshot
    import omniparser_amd.florence as FL
    cap = Florence2Captioner(small_vocab_caption_checkpoint(0), "cuda", precision="f32", resolution=64)
    monkeypatch.setattr(Florence2Captioner, "decode_bucket", staticmethod(lambda n: 8))
    monkeypatch.setattr(FL, "_BUCKETS", (2, 128))
    frame = torch.from_numpy(synthetic_screenshot(3, 640, 480))
    rects = [[[10, 20, 60, 70], [300, 200, 340, 260], [500, 100, 620, 140]], [[40, 40, 90, 80], [200, 300, 280, 360]]]
    got = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("OMNI_MERGED_DECODE", mode)
        sp = ScreenParser(None, cap, batch_size=2)
        sp.max_new_tokens = 3
        scored = sp.caption([frame, frame], rects, scores=True)
        if mode == "1":                  # (one comparison with the call without scores: every call is an emulated encode)
            plain = sp.caption([frame, frame], rects)
            assert [[r.tolist() for _, r in f] for f in plain] == [[r.tolist() for _, r, _ in f] for f in scored]
        got[mode] = [[c for _, _, c in f] for f in scored]
        assert all(c is not None and 0.0 < c <= 1.0 for f in got[mode] for c in f)
    keys = list(cap._plans)
    assert ("dec", 8, 64, 3) in keys and any(k[0] == "dec" and k[-1] == "scores" for k in keys)
    assert sum(1 for k in keys if k[0] != "dec" and k[-1] == "scores") == 1          # the per-micro-batch decode's 2-row plan only
    import score_checks as SC
    for a, b in zip(got["1"], got["0"]):
        assert len(a) == len(b) and all(abs(math.log(x) - math.log(y)) <= SC.TOL_LOGP for x, y in zip(a, b))
    cap.num_beams = 3
    with pytest.raises(ValueError):
        ScreenParser(None, cap, batch_size=2).caption([frame, frame], rects, scores=True)


def test_caption_confidence_definition():
    from omniparser_amd.florence import caption_confidence
    lp = [-0.5, -1.0, -2.0, -4.0]
    # forced BOS only: position 1 is left out, the rest counts (no EOS: all of them)
    assert caption_confidence([2, 0, 11, 12, 13], lp, 2, 0, -1, 4) == pytest.approx(math.exp(-(1.0 + 2.0 + 4.0) / 3))
    # forced EOS reached at max_new: left out as well
    assert caption_confidence([2, 0, 11, 12, 2], lp, 2, 0, 2, 4) == pytest.approx(math.exp(-(1.0 + 2.0) / 2))
    # a chosen EOS at position 2 ends the caption and counts; what follows (pad, log-prob 0) does not
    assert caption_confidence([2, 0, 2, 1, 1], [-0.5, -1.0, 0.0, 0.0], 2, 0, 2, 4) == pytest.approx(math.exp(-1.0))
    assert caption_confidence([2, 9, 2, 1, 1], [-0.5, -1.0, 0.0, 0.0], 2, -1, -1, 4) == pytest.approx(math.exp(-0.75))
    # nothing unforced
    assert caption_confidence([2, 0], [0.0], 2, 0, 2, 1) is None
    assert caption_confidence([2, 0, 2], [0.0, 0.0], 2, 0, 2, 2) is None
    assert caption_confidence([2], [], 2, 0, 2, 4) is None
    # tensors work as rows
    assert caption_confidence(torch.tensor([2, 0, 11]), torch.tensor([0.0, -0.25]), 2, 0, 2, 20) == pytest.approx(math.exp(-0.25))


def test_output_scores_argument_validation(emu):
    from omniparser_amd.florence import Florence2Captioner
    from tools.make_weights import ensure_caption_checkpoint
    cap = Florence2Captioner(ensure_caption_checkpoint(0), "cuda", precision="f32", resolution=64)
    assert cap.token_scores is False
    pix = torch.zeros(1, 3, 64, 64)
    with pytest.raises(ValueError):
        cap.generate(pixel_values=pix, output_scores=True)
    with pytest.raises(ValueError):
        cap.generate(pixel_values=pix, output_scores=True, return_dict_in_generate=True, num_beams=3)
    with pytest.raises(ValueError):
        cap.caption_crops(torch.zeros(64, 64, 3, dtype=torch.uint8), [[0, 0, 8, 8]], num_beams=3, return_scores=True)
    assert cap._plans == {}                  # nothing was built for a refused call


def test_omniparser_rejects_a_non_bool_caption_confidence(monkeypatch):
    import types
    from omniparser_amd.util import omniparser as F
    from omniparser_amd.util import utils as U
    model = types.SimpleNamespace(token_scores=False)
    monkeypatch.setattr(U, "get_yolo_model", lambda model_path, device: object())
    monkeypatch.setattr(U, "get_caption_model_processor", lambda model_name, model_name_or_path, device: {"model": model, "processor": None})
    cfg = {"som_model_path": "x", "caption_model_name": "florence2", "caption_model_path": "y", "BOX_TRESHOLD": 0.05}
    for bad in (1, "yes", 0.5):
        with pytest.raises(ValueError):
            F.Omniparser({**cfg, "caption_confidence": bad})
    assert model.token_scores is False
    F.Omniparser({**cfg, "caption_confidence": True})
    assert model.token_scores is True
    F.Omniparser(cfg)
    assert model.token_scores is True        # no key: the model is left as it is


def test_header_documents_the_token_score_slot():
    hdr = (Path(__file__).resolve().parents[1] / "include" / "omni_amd.h").read_text()
    doc = re.search(r"/\* greedy decoding step.*?\*/\s*OMNI_OP_GREEDY_STEP = 16,", hdr, re.S)
    assert doc and re.search(r"\bp4 f32 \[B, T\]", doc.group(0)) and "p4 NULL" in doc.group(0)
    assert "#define OMNI_ABI_VERSION 3" in hdr

"""`-m gpu`: scoring candidate texts with a teacher-forced decode on the MI355X — the target-score form of OMNI_OP_GREEDY_STEP (p5)
against an f64 log-softmax at the full vocabulary, Florence2Captioner.score against transformers' teacher-forced forward pass on the
CPU, score_crops, rank_elements, ScreenParser.rank and Omniparser.ground.  Helpers, bound and tolerance: tests/target_checks.py; the
host-emulation twin: tests/test_target_scores_emu_cpu.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("B", [4, 130])
def test_score_step_matches_f64_full_vocab(B, f16):
    """V = 51289 (odd: a row is aligned to its element only, so the 16-byte loads are peeled in front and behind), B = 4 and B = 130
    workgroups, bias, 6 steps: the kernel case of the emulation test with the same f64 reference and bound"""
    import gpu_checks as G
    import target_checks as TC
    from omniparser_amd import _lib as L
    TC.check_kernel_case(L, G.DEV, B, 51289, 6, True, f16, seed=B + f16, sync=G._sync)
    TC.check_degenerate_rows(L, G.DEV, G._sync)


def test_score_step_bad_arguments_are_errors():
    """p5 with p4 = NULL and p7 without p5 are OMNI_E_ARG; a wild p5 / p7 is OMNI_E_ARG through the pointer check of omni_op_launch
    and omni_plan_create (an error code, never a fault), and so is a p7 that runs off its allocation"""
    import os
    import gpu_checks as G
    import target_checks as TC
    from omniparser_amd import _lib as L
    TC.check_argument_errors(L, G.DEV)
    if os.environ.get("OMNI_CHECK_PTRS", "1")[:1] == "0":
        return                                                  # the pointer check is switched off here: a wild pointer WOULD fault
    B, V, T = 2, 64, 3
    t = {"logits": torch.zeros(B, V, device=G.DEV), "ids": torch.zeros(B, T, dtype=torch.int32, device=G.DEV),
         "step": torch.zeros(1, dtype=torch.int32, device=G.DEV), "logp": torch.zeros(B, T, device=G.DEV),
         "tlen": torch.zeros(B, dtype=torch.int32, device=G.DEV), "top1": torch.zeros(B, T, dtype=torch.int32, device=G.DEV)}
    good = TC.score_op(L, L.F32, t["logits"], None, t["ids"], t["step"], t["logp"], t["tlen"], t["top1"], B, V, T)
    L.launch(good); G._sync()
    wild = 0x00007AB000001000
    seen = {}
    for name, slot in (("wild_p5", 5), ("wild_p7", 7)):
        op = TC.score_op(L, L.F32, t["logits"], None, t["ids"], t["step"], t["logp"], t["tlen"], t["top1"], B, V, T)
        op.p[slot] = wild
        for how in ("launch", "plan"):
            with pytest.raises(L.OmniError, match="not inside any device allocation") as e:
                L.launch(op) if how == "launch" else L.Plan([good, op])
            assert "error -1" in str(e.value)
            seen[f"{name}/{how}"] = str(e.value)[:120]
    G._sync()
    L.launch(good); G._sync()                                   # the process is alive and the library still launches
    assert int(t["step"].cpu()[0]) == 2 and len(seen) == 4


@pytest.fixture(scope="module")
def cap():
    import target_checks as TC
    return TC.make_captioner()


def test_score_matches_transformers_one_pass(cap):
    """8 crops x 5 labels (the crop's own greedy caption + 4 random labels, lengths 2..16): one pass, M padded to 8; scoring a label
    alone (M = 1) and scoring shared labels agree with the joint per-image call"""
    import target_checks as TC
    px, per, shared, out, _ = TC.captioner_vs_hf(cap, 8, [2, 5, 9, 16], 311, 12, device_pixels=True)
    assert cap.score_stats == {"encodes": 1, "passes": 1, "steps": 16}
    forced = [k for k in cap._plans if isinstance(k[-1], tuple) and k[-1][0] == "force"]
    assert [k[-1] for k in forced] == [("force", 8, 16)]
    alone = cap.score(px, [shared[1]])                               # M = 1
    assert tuple(alone.token_logprobs.shape) == (8, 1, 5) and cap.score_stats["steps"] == 5
    d1 = float((alone.token_logprobs[:, 0] - out.token_logprobs[:, 2, :5]).abs().max())
    together = cap.score(px, shared)                                 # shared labels, M = 4
    d2 = float((together.token_logprobs - out.token_logprobs[:, 1:]).abs().max())
    print(f"M = 1 vs together: {d1:.3e}; shared vs per-image: {d2:.3e}")
    assert d1 <= TC.TOL_TARGET_LOGP and d2 <= TC.TOL_TARGET_LOGP
    assert torch.equal(together.lengths, out.lengths[:, 1:])


def test_score_matches_transformers_two_passes_over_one_encode(cap):
    """8 crops x 11 labels: two passes of the step loop (8 + 3 labels) over ONE encode of the micro-batch"""
    import target_checks as TC
    TC.captioner_vs_hf(cap, 8, [2, 3, 4, 5, 6, 7, 9, 11, 13, 16], 312, 10, device_pixels=True)
    assert cap.score_stats["encodes"] == 1 and cap.score_stats["passes"] == 2


def test_score_crops_rank_elements_and_the_facades(cap):
    """seeded 1280x800 frame: score_crops = score on the pixels of the same crops; rank_elements orders the elements as transformers'
    scores do; top_k cuts; ScreenParser.rank gives the same lists"""
    import target_checks as TC
    from omniparser_amd.pipeline import ScreenParser
    from omniparser_amd.util import utils as U
    frame, elements, queries = TC.frame_and_queries()
    index, boxes, pix, scores, _ = TC.oracle_ranking(cap, frame, elements, queries)
    assert 4 not in index and len(index) == len(elements) - 1
    gap = TC.smallest_oracle_gap(scores)
    print(f"oracle: smallest score gap between two elements {gap:.3e} (2 tol = {2 * TC.TOL_TARGET_LOGP:.3e})")
    assert gap >= 2 * TC.TOL_TARGET_LOGP, "choose another frame seed: the oracle itself has a near tie"
    a = cap.score_crops(frame.cuda(), boxes, queries)
    b = cap.score(pix.cuda(), queries)
    d = float((a.token_logprobs - b.token_logprobs).abs().max())
    print(f"score_crops vs score: {d:.3e}")
    assert d <= TC.TOL_TARGET_LOGP and torch.equal(a.lengths, b.lengths)
    proc = U.FlorenceProcessor(cap.w.dir)
    cmp_ = {"model": cap, "processor": proc}
    ranked = U.rank_elements(frame.numpy(), elements, cmp_, queries)
    TC.check_ranking(ranked, index, scores, TC.TOL_TARGET_LOGP)
    top = U.rank_elements(frame.numpy(), elements, cmp_, queries, top_k=3)
    assert [len(r) for r in top] == [3, 3, 3] and [[e["index"] for e in r] for r in top] == [[e["index"] for e in r[:3]] for r in ranked]
    sp = ScreenParser(None, cap, processor=proc)
    via_sp = sp.rank(frame.cuda(), elements, queries, top_k=3)
    assert [[e["index"] for e in r] for r in via_sp] == [[e["index"] for e in r] for r in top]
    assert all(abs(x["score"] - y["score"]) <= TC.TOL_TARGET_LOGP for r, s in zip(via_sp, top) for x, y in zip(r, s))
    if proc.tok is None:
        with pytest.raises(ValueError, match="tokenizer"):
            U.rank_elements(frame.numpy(), elements, cmp_, ["the save button"])


def test_omniparser_ground_ranks_the_parsed_elements():
    """Omniparser.ground = parse + rank_elements: the same elements as parse, the same ranking as rank_elements on them"""
    import base64
    import io
    import os
    import numpy as np
    from PIL import Image
    import target_checks as TC
    from omniparser_amd.synth import synthetic_ocr, synthetic_screenshot
    from omniparser_amd.util import utils as U
    from omniparser_amd.util.omniparser import Omniparser
    from tools.make_weights import ensure_blob, ensure_caption_checkpoint
    os.environ["OMNI_CAPTION_RES"] = "64"
    try:
        cfg = {"som_model_path": str(ensure_blob(seed=0, nc=1, width=0.5)), "caption_model_name": "florence2",
               "caption_model_path": str(ensure_caption_checkpoint(0)), "BOX_TRESHOLD": 0.05,
               "ocr_provider": lambda image: synthetic_ocr(2, image.size[0], image.size[1], 24)}
        img = synthetic_screenshot(2, 1280, 800)
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, format="PNG")
        b64 = base64.b64encode(buf.getvalue()).decode("ascii")
        op = Omniparser(cfg)
        queries = TC.random_labels((3, 6), 5)
        elements, rankings = op.ground(b64, queries, top_k=4)
        _png, plain = op.parse(b64)
        want = U.rank_elements(np.asarray(img), elements, op.caption_model_processor, queries, top_k=4)
    finally:
        os.environ.pop("OMNI_CAPTION_RES", None)
    assert elements == plain and len(rankings) == 2 and all(len(r) == 4 for r in rankings)
    assert [[e["index"] for e in r] for r in rankings] == [[e["index"] for e in r] for r in want]
    assert all(abs(x["score"] - y["score"]) <= TC.TOL_TARGET_LOGP for r, s in zip(rankings, want) for x, y in zip(r, s))
    assert all(r[k]["score"] >= r[k + 1]["score"] for r in rankings for k in range(3))

"""Scoring candidate texts with a teacher-forced decode (the target-score form of OMNI_OP_GREEDY_STEP, p5; Florence2Captioner.score /
score_crops, florence.sequence_score, util.utils.rank_elements, ScreenParser.rank, Omniparser.ground) on the host emulation of the HIP
kernels (tests/emu): the kernel against an f64 log-softmax of the raw logits, the captioner against transformers' teacher-forced
forward pass.  Helpers, bound and tolerance: tests/target_checks.py."""
import itertools
import re
from pathlib import Path

import pytest
import torch

from omniparser_amd import _lib as L

KERNEL_CASES = list(itertools.product((2003, 51289), (True, False), (False, True)))


@pytest.mark.parametrize("V,with_bias,f16", KERNEL_CASES)
def test_score_step_matches_f64(emu, V, with_bias, f16):
    """B = 6 rows with tlen in {0, 1, mid, T - 1}, 16 steps of scripted logits (3 at the full vocabulary): logp within the derived
    bound of the f64 log-softmax at the given token (-inf for a -inf target), top1 the f64 arg-max, ids bit-equal, p4 / p7 untouched in
    column 0 and behind tlen, step incremented."""
    import target_checks as TC
    steps = 16 if V == 2003 else 3
    r = TC.check_kernel_case(L, torch.device("cpu"), 6, V, steps, with_bias, f16, seed=V % 1000 + with_bias)
    assert r["scored"] >= 6


def test_score_step_degenerate_rows(emu):
    import target_checks as TC
    TC.check_degenerate_rows(L, torch.device("cpu"))


def test_score_step_argument_errors(emu):
    import target_checks as TC
    seen = TC.check_argument_errors(L, torch.device("cpu"))
    assert "p4" in seen["p5_without_p4"] and "p5" in seen["p7_without_p5"]


def test_header_documents_the_target_score_form():
    hdr = (Path(__file__).resolve().parents[1] / "include" / "omni_amd.h").read_text()
    doc = re.search(r"/\* greedy decoding step.*?\*/\s*OMNI_OP_GREEDY_STEP = 16,", hdr, re.S)
    assert doc and re.search(r"\bp5 tlen i32 \[B\]", doc.group(0)) and "p7 top1 i32 [B, T]" in doc.group(0)
    assert "#define OMNI_ABI_VERSION 3" in hdr
    assert re.search(r"OMNI_OP_BEAM_STEP,\s*OMNI_OP__COUNT", hdr)


def test_score_matches_transformers_r64_and_leaves_the_other_plans_alone(emu):
    """2 crops x 3 labels of lengths 2, 5 and 8 (the 8-token one is the crop's own greedy caption) at 64x64 against transformers;
    a label scored alone (M = 1) and shared labels agree with the joint per-image call; the default plan and a scores plan keep
    p5 = p7 = NULL, and the force plan has their op kinds in their order"""
    import target_checks as TC
    cap = TC.make_captioner()
    px, per, shared, out, _ = TC.captioner_vs_hf(cap, 2, [2, 5], 31, 8)
    assert sorted(len(r) for r in per[0]) == [2, 5, 8]
    assert cap.score_stats == {"encodes": 1, "passes": 1, "steps": 8}
    alone = cap.score(px, [shared[1]])                                # M = 1; one encode, 5 steps
    d1 = float((alone.token_logprobs[:, 0] - out.token_logprobs[:, 2, :5]).abs().max())
    together = cap.score(px, shared)                                  # shared labels on the plan of the joint call
    d2 = float((together.token_logprobs - out.token_logprobs[:, 1:, :5]).abs().max())
    print(f"M = 1 vs together: {d1:.3e}; shared vs per-image: {d2:.3e}")
    assert d1 <= TC.TOL_TARGET_LOGP and d2 <= TC.TOL_TARGET_LOGP
    forced = [k[-1] for k in cap._plans if isinstance(k[-1], tuple) and k[-1][0] == "force"]
    assert sorted(forced) == [("force", 1, 8), ("force", 4, 8)] and len(cap._plans) == 2
    pf = cap.plans(cap.bucket(2), 64, 8, force=4)
    p0 = cap.plans(cap.bucket(2), 64, 8)
    p1 = cap.plans(cap.bucket(2), 64, 8, scores=True)
    greedy = lambda p: [op for op in p.step_plan.ops if op.kind == L.OP_GREEDY_STEP]
    for p in (p0, p1):
        assert len(greedy(p)) == 1 and greedy(p)[0].p[5] is None and greedy(p)[0].p[7] is None and p.force is None
    assert greedy(p0)[0].p[4] is None and greedy(p1)[0].p[4] == p1.logp.data_ptr()
    g = greedy(pf)[0]
    assert g.p[3] is None and g.p[4] == pf.logp.data_ptr() and g.p[5] == pf.tlen.data_ptr() and g.p[7] == pf.top1.data_ptr()
    assert [op.kind for op in pf.step_plan.ops] == [op.kind for op in p0.step_plan.ops]
    assert [op.kind for op in pf.encode_plan.ops] == [op.kind for op in p0.encode_plan.ops]
    assert tuple(pf.ids.shape) == (pf.B * 4, 9) and tuple(pf.tlen.shape) == (pf.B * 4,) and pf.logp.dtype == torch.float32
    cross = [op for op in pf.step_plan.ops if op.kind == L.OP_ATTN_DECODE and op.i[7] > 0]
    self_ = [op for op in pf.step_plan.ops if op.kind == L.OP_ATTN_DECODE and op.i[7] == 0]
    assert cross and all(op.i[12] == 4 for op in cross) and self_ and all(op.p[7] is None for op in self_)


def test_score_label_validation(emu):
    """the ValueError cases of score / score_crops: no label, an empty label, more than 32 tokens, an id outside the vocabulary,
    per-image lists that do not match the images; nothing is built for a refused call"""
    import target_checks as TC
    cap = TC.make_captioner()
    pix = torch.zeros(2, 3, 64, 64)
    frame = torch.zeros(64, 64, 3, dtype=torch.uint8)
    for bad in ([], [[]], [[0, 5, 2], []], [[0] + [7] * 31 + [2]], [[0, cap.w.vocab, 2]], [[0, -1, 2]], [[[0, 2]]], [[[0, 2]], []],
                [[[0, 2]], [[0, 2], [0, 3, 2]]]):
        with pytest.raises(ValueError):
            cap.score(pix, bad)
        with pytest.raises(ValueError):
            cap.score_crops(frame, [[0, 0, 8, 8], [8, 8, 32, 32]], bad)
    assert cap._plans == {}
    assert cap._check_labels([[0] + [7] * 30 + [2]], 2)[1:] == (1, True)              # 32 tokens are allowed
    assert cap._check_labels([[[0, 2]], [[0, 9, 2]]], 2)[1:] == (1, False)


def test_sequence_score_definition():
    from omniparser_amd.florence import sequence_score
    lp = torch.tensor([[[-0.5, -1.0, -2.0, 0.0], [-0.25, -4.0, 0.0, 0.0]]])
    ln = torch.tensor([[3, 2]])
    labels = [[[0, 11, 2], [9, 2]]]
    assert sequence_score(lp, ln, normalize="sum").tolist() == [[-3.5, -4.25]]
    assert sequence_score(lp, ln).tolist() == [[pytest.approx(-3.5 / 3), -2.125]]
    # the checkpoint's forced BOS at position 0 says nothing about the text: left out where the label starts with it
    assert sequence_score(lp, ln, labels=labels, forced_bos=0).tolist() == [[-1.5, -2.125]]
    assert sequence_score(lp, ln, labels=labels, normalize="sum", forced_bos=0).tolist() == [[-3.0, -4.25]]
    assert sequence_score(lp, ln, forced_bos=0).tolist() == [[-1.5, -4.0]]             # without labels: every label starts with it
    assert sequence_score(lp, ln, labels=labels, forced_bos=-1).tolist() == sequence_score(lp, ln).tolist()
    assert sequence_score(lp[0, 0], ln[0, 0], labels=[0, 11, 2], forced_bos=0).item() == -1.5
    assert sequence_score(torch.tensor([-0.5]), torch.tensor(1), forced_bos=0).item() == 0.0
    with pytest.raises(ValueError):
        sequence_score(lp, ln, normalize="max")


def test_rank_elements_orders_by_score_and_validates(monkeypatch):
    """rank_elements on a stand-in model: descending scores, ties to the lower index, empty crops skipped, top_k cuts, string
    queries without a tokenizer.json raise the processor's ValueError before anything runs"""
    import types
    import numpy as np
    import target_checks as TC
    from omniparser_amd.util import utils as U
    elements = TC.frame_elements()
    table = {0: -2.0, 1: -1.0, 2: -1.0, 3: -3.0, 5: -0.5, 6: -4.0, 7: -1.0, 8: -2.5}
    calls = []

    def score_crops(img, boxes_px, labels, **kw):
        calls.append((tuple(img.shape), len(boxes_px), [list(l) for l in labels], kw))
        lp = torch.zeros(len(boxes_px), len(labels), 3)
        kept = [k for k in range(len(elements)) if k != 4]
        for b, k in enumerate(kept):
            lp[b, :, 1] = table[k]
            lp[b, 1, 1] = -table[k] - 10.0                       # the second query ranks the other way round
        return types.SimpleNamespace(token_logprobs=lp, lengths=torch.full((len(boxes_px), len(labels)), 3), top1=lp.long())
    model = types.SimpleNamespace(score_crops=score_crops, device="cpu", w=types.SimpleNamespace(forced_bos=0))
    cmp_ = {"model": model, "processor": U.FlorenceProcessor(None)}
    frame = np.zeros((TC.FRAME_H, TC.FRAME_W, 3), np.uint8)
    queries = [[0, 11, 2], [0, 12, 2]]
    ranked = U.rank_elements(frame, elements, cmp_, queries)
    assert [r["index"] for r in ranked[0]] == [5, 1, 2, 7, 0, 8, 3, 6] and [r["index"] for r in ranked[1]] == [6, 3, 8, 0, 1, 2, 7, 5]
    assert ranked[0][0]["score"] == -0.25 and calls[0][:3] == ((TC.FRAME_H, TC.FRAME_W, 3), 8, queries) and calls[0][3] == {}
    assert [r["index"] for r in U.rank_elements(frame, elements, cmp_, queries, top_k=2)[0]] == [5, 1]
    assert U.rank_elements(frame, elements, cmp_, queries, normalize="sum")[0][0]["score"] == -0.5
    n = len(calls)
    with pytest.raises(ValueError, match="tokenizer.json"):
        U.rank_elements(frame, elements, cmp_, ["the save button"])
    for bad in (0, -1, True, 2.5):
        with pytest.raises(ValueError):
            U.rank_elements(frame, elements, cmp_, queries, top_k=bad)
    with pytest.raises(ValueError):
        U.rank_elements(frame, elements, cmp_, [])
    assert len(calls) == n

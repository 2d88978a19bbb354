"""`-m gpu`: closed-vocabulary greedy decoding on the MI355X — OMNI_OP_GREEDY_VOCAB_STEP at the full vocabulary case by case against
transformers' own logits processors, generate(vocabulary=...) on both stand-in checkpoints against transformers'
generate(prefix_allowed_tokens_fn=...) on the CPU, caption_crops against generate, the plan / default-path rules and
get_parsed_content_icon.  Helpers and bounds: tests/vocab_checks.py; the host-emulation twin: tests/test_caption_vocabulary_emu_cpu.py."""
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
def test_wide_node_first_last_and_wrapped_child(f16, scores):
    import vocab_checks as VC
    dev, sync = _dev()
    print(f"worst logp error {VC.check_wide_node(L, dev, V_FULL, f16, scores, sync=sync):.3f} of the bound")


@BOTH
def test_single_child_and_equal_children(f16, scores):
    import vocab_checks as VC
    dev, sync = _dev()
    VC.check_single_child_and_ties(L, dev, V_FULL, f16, scores, sync=sync)


@BOTH
def test_ngram_ban_removes_one_child_and_every_child(f16, scores):
    import vocab_checks as VC
    dev, sync = _dev()
    VC.check_ngram_ban(L, dev, V_FULL, f16, scores, sync=sync)


@BOTH
def test_leaf_left_trie_and_finished_row(f16, scores):
    import vocab_checks as VC
    dev, sync = _dev()
    VC.check_leaf_and_outside(L, dev, V_FULL, f16, scores, sync=sync)


@BOTH
def test_forced_positions_move_the_node(f16, scores):
    import vocab_checks as VC
    dev, sync = _dev()
    VC.check_forced_positions(L, dev, V_FULL, f16, scores, sync=sync)


@BOTH
def test_edge_token_beyond_the_vocabulary_is_skipped(f16, scores):
    import vocab_checks as VC
    dev, sync = _dev()
    VC.check_edge_token_beyond_vocabulary(L, dev, V_FULL, f16, scores, sync=sync)


def test_short_trie_block_is_an_argument_error():
    import vocab_checks as VC
    dev, sync = _dev()
    seen = VC.check_short_block(L, dev, V_FULL, sync=sync)
    assert all("trie block" in m for m in seen), seen


# ---------------------------------------------------------------------------------------------- whole captioner
@pytest.mark.parametrize("eos_prone", [False, True])
def test_constrained_captions_match_transformers_r64(eos_prone):
    """4 crops at 64x64, pixel seed vocab_checks.SEED, 64 labels, max_new_tokens = the longest label + 2, f32 plans: ids equal
    transformers' with the same labels as prefix_allowed_tokens_fn (no row excused), every row one label, token log-probabilities
    within long_checks.TOL_LOGP_LONG"""
    import vocab_checks as VC
    VC.captioner_vs_hf(eos_prone, device_pixels=True)


@pytest.mark.parametrize("eos_prone", [False, True])
def test_caption_crops_equals_generate(eos_prone):
    import gen_ctrl_checks as GC
    import vocab_checks as VC
    VC.check_caption_crops(GC.captioner(eos_prone))


def test_plans_and_defaults():
    import gen_ctrl_checks as GC
    import vocab_checks as VC
    VC.check_plans_and_defaults(GC.captioner(False), device_pixels=True)


# ---------------------------------------------------------------------------------------------- public surface
def test_get_parsed_content_icon_with_a_vocabulary():
    """contents are batch_decode of the ids caption_crops(vocabulary=...) gives for the same boxes, every one of them a label;
    confidences are caption_confidence of the constrained log-probabilities; vocabulary=None is the call as it was"""
    import gen_ctrl_checks as GC
    import vocab_checks as VC
    from omniparser_amd.florence import caption_confidence
    from omniparser_amd.synth import synthetic_screenshot
    from omniparser_amd.util import utils as U
    cap = GC.captioner(False)
    proc = U.FlorenceProcessor(None)
    cmp_ = {"model": cap, "processor": proc}
    arr = synthetic_screenshot(5)
    boxes = torch.tensor([[0.1, 0.1, 0.2, 0.2], [0.3, 0.3, 0.5, 0.4], [0.6, 0.2, 0.8, 0.5]])
    labels = VC.labels_for(cap.w.eos)
    px = U.crop_boxes_px(boxes.tolist(), arr.shape[1], arr.shape[0])
    ids, lp = cap.caption_crops(torch.from_numpy(arr).cuda(), px, vocabulary=labels, return_scores=True)
    VC.check_rows_are_labels(ids, torch.tensor([VC.vocabulary(labels).label_index(r[1:], cap.w.eos) for r in ids.tolist()]), labels,
                             cap.w.eos, cap.w.pad, cap.w.start)
    want = [t.strip() for t in proc.batch_decode(ids, skip_special_tokens=True)]
    assert U.get_parsed_content_icon(boxes, 0, arr, cmp_, vocabulary=labels) == want
    pairs = U.get_parsed_content_icon(boxes, 0, arr, cmp_, vocabulary=labels, return_confidence=True)
    w = cap.w
    assert pairs == [(t, caption_confidence(r, l, w.eos, w.forced_bos, w.forced_eos, 20)) for t, r, l in zip(want, ids, lp)]
    plain = U.get_parsed_content_icon(boxes, 0, arr, cmp_)
    assert plain == U.get_parsed_content_icon(boxes, 0, arr, cmp_, vocabulary=None) and plain != want

"""Closed-vocabulary greedy decoding on the host emulation of the HIP kernels (tests/emu) and on the host alone:
OMNI_OP_GREEDY_VOCAB_STEP case by case against transformers' own logits processors, generate(vocabulary=...) against transformers'
generate(prefix_allowed_tokens_fn=...), the plan / default-path rules, the argument checks and the packed trie block.  Helpers and
bounds: tests/vocab_checks.py; the MI355X twin: tests/test_gpu_v_caption_vocabulary.py."""
import re
import types
from pathlib import Path

import pytest
import torch

from omniparser_amd import _lib as L

CPU = torch.device("cpu")
V_EMU = 1037                    # no multiple of 32 or 256
BOTH = pytest.mark.parametrize("f16,scores", [(False, False), (False, True), (True, False), (True, True)])


# ---------------------------------------------------------------------------------------------- kernel, one launch per case
@BOTH
def test_wide_node_first_last_and_wrapped_child(emu, f16, scores):
    import vocab_checks as VC
    print(f"worst logp error {VC.check_wide_node(L, CPU, V_EMU, f16, scores):.3f} of the bound")


@BOTH
def test_single_child_and_equal_children(emu, f16, scores):
    import vocab_checks as VC
    VC.check_single_child_and_ties(L, CPU, V_EMU, f16, scores)


@BOTH
def test_ngram_ban_removes_one_child_and_every_child(emu, f16, scores):
    import vocab_checks as VC
    VC.check_ngram_ban(L, CPU, V_EMU, f16, scores)


@BOTH
def test_leaf_left_trie_and_finished_row(emu, f16, scores):
    import vocab_checks as VC
    VC.check_leaf_and_outside(L, CPU, V_EMU, f16, scores)


@BOTH
def test_forced_positions_move_the_node(emu, f16, scores):
    import vocab_checks as VC
    VC.check_forced_positions(L, CPU, V_EMU, f16, scores)


@BOTH
def test_edge_token_beyond_the_vocabulary_is_skipped(emu, f16, scores):
    import vocab_checks as VC
    VC.check_edge_token_beyond_vocabulary(L, CPU, V_EMU, f16, scores)


def test_short_trie_block_is_an_argument_error(emu):
    import vocab_checks as VC
    seen = VC.check_short_block(L, CPU, V_EMU)
    assert all("trie block" in m for m in seen), seen


# ---------------------------------------------------------------------------------------------- whole captioner
def test_constrained_captions_match_transformers_r64(emu):
    """the stock checkpoint only, without the caption_crops twin: emulated steps are slow"""
    import vocab_checks as VC
    VC.captioner_vs_hf(False)


def test_plans_and_defaults(emu):
    import gen_ctrl_checks as GC
    import vocab_checks as VC
    VC.check_plans_and_defaults(GC.captioner(False), full=False)


# ---------------------------------------------------------------------------------------------- host side, no device
@pytest.fixture(scope="module")
def host_cap():
    """a captioner object without a device: the argument checks run before anything touches one"""
    from omniparser_amd.florence import Florence2Captioner, FlorenceWeights
    from tools.make_weights import ensure_caption_checkpoint
    cap = Florence2Captioner.__new__(Florence2Captioner)
    cap.w = FlorenceWeights(ensure_caption_checkpoint(0))
    cap.num_beams, cap.token_scores, cap.resolution, cap._plans = 1, False, 64, {}
    return cap


GOOD = [[0, 7, 8, 2], [0, 7, 2]]
BAD = {
    "no label": [],
    "an empty label": [[0, 7, 2], []],
    "65 tokens": [[0] + list(range(100, 163)) + [2]],
    "an id below 0": [[0, -7, 2]],
    "not ids": [[0, 7.0, 2]],
    "a bool": [[0, True, 2]],
    "a string": "close",
    "no list": 7,
    "an id outside the vocabulary": [[0, 51290, 2]],
    "no EOS at the end": [[0, 7, 8]],
    "EOS inside": [[0, 7, 2, 8, 2]],
    "no forced BOS": [[7, 8, 2]],
    "longer than max_new_tokens": [[0] + list(range(100, 120)) + [2]],
    "a dead end": [[0, 7, 8, 7, 8, 7, 2]],        # behind 2 0 7 8 7 8 the 3-gram (7 8 7) is banned, and 7 is the only child
}


@pytest.mark.parametrize("name", list(BAD))
def test_bad_vocabularies_are_value_errors_before_any_device_work(host_cap, name):
    cap = host_cap
    assert cap.w.vocab == 51290 and (cap.w.eos, cap.w.forced_bos, cap.w.forced_eos, cap.w.ngram, cap.w.start) == (2, 0, 2, 3, 2)
    pix = torch.zeros(1, 3, 64, 64)
    frame = torch.zeros(64, 64, 3, dtype=torch.uint8)
    with pytest.raises(ValueError):
        cap.generate(pixel_values=pix, max_new_tokens=20, vocabulary=BAD[name])
    with pytest.raises(ValueError):
        cap.caption_crops(frame, [[0, 0, 8, 8]], max_new_tokens=20, vocabulary=BAD[name])
    assert cap._plans == {}


def test_too_many_nodes_is_a_value_error():
    from omniparser_amd.florence import VOCAB_MAX_NODES, CaptionVocabulary
    rows = [[0, 100 + a, 100 + b, 2] for a in range(182) for b in range(182)]       # 1 + 1 + 182 + 2 * 182^2 nodes
    assert 2 + 182 + 2 * 182 * 182 > VOCAB_MAX_NODES
    with pytest.raises(ValueError, match="nodes"):
        CaptionVocabulary(rows)
    assert CaptionVocabulary(rows[:32000]).n_nodes <= VOCAB_MAX_NODES


def test_dead_end_names_the_prefix_and_forced_eos_rule():
    from omniparser_amd.florence import CaptionVocabulary
    v = CaptionVocabulary([[0, 7, 8, 7, 8, 7, 2], [0, 7, 9, 2]])
    with pytest.raises(ValueError, match=r"dead end behind the prefix \[2, 0, 7, 8, 7, 8\]"):
        v.check(51290, 20, 2, 0, 2, 3, 2)
    assert v.check(51290, 20, 2, 0, 2, 0, 2) is v                      # no ban, no dead end
    assert v.check(51290, 20, 2, 0, 2, 4, 2) is v
    # a second child that is not banned: no dead end
    assert CaptionVocabulary([[0, 7, 8, 7, 8, 7, 2], [0, 7, 8, 7, 8, 9, 2]]).check(51290, 20, 2, 0, 2, 3, 2)
    # the decoder start token is part of the prefix: behind 5 | 5 6 5 the 2-gram rule bans 5 (from "5 5") and 6 (from "5 6")
    with pytest.raises(ValueError, match=r"dead end behind the prefix \[5, 5, 6, 5\]"):
        CaptionVocabulary([[5, 6, 5, 6, 2]]).check(51290, 20, 2, -1, 2, 2, 5)
    assert CaptionVocabulary([[5, 6, 7, 6, 2]]).check(51290, 20, 2, -1, 2, 2, 5)    # "5 5" and "6 7" ban 5 and 7, never the child
    # a forced EOS that is not the EOS token bites only where it is the last token of a longest label
    w = CaptionVocabulary([[0, 7, 13840], [0, 7, 8, 13840]])
    with pytest.raises(ValueError, match="forces token 2"):
        w.check(51290, 4, 13840, 0, 2, 3, 2)
    assert w.check(51290, 5, 13840, 0, 2, 3, 2) is w
    with pytest.raises(ValueError, match="below the longest label"):
        w.check(51290, 3, 13840, 0, 2, 3, 2)


def test_vocabulary_with_beams_or_controls_is_refused(host_cap):
    cap = host_cap
    pix = torch.zeros(1, 3, 64, 64)
    frame = torch.zeros(64, 64, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="beam search"):
        cap.generate(pixel_values=pix, num_beams=3, vocabulary=GOOD)
    with pytest.raises(ValueError, match="beam search"):
        cap.caption_crops(frame, [[0, 0, 8, 8]], num_beams=3, vocabulary=GOOD)
    for kw in (dict(repetition_penalty=1.3), dict(no_repeat_ngram_size=3), dict(no_repeat_ngram_size=0), dict(min_new_tokens=2),
               dict(suppress_tokens=[9]), dict(begin_suppress_tokens=[9]), dict(bad_words_ids=[[9, 10]])):
        with pytest.raises(ValueError, match="generation controls"):
            cap.generate(pixel_values=pix, vocabulary=GOOD, **kw)
        with pytest.raises(ValueError, match="generation controls"):
            cap.caption_crops(frame, [[0, 0, 8, 8]], vocabulary=GOOD, controls=kw)
    with pytest.raises(ValueError):
        cap.plans(8, 64, 20, beam=(3, 1.0, False), vocab=True)
    with pytest.raises(ValueError):
        cap.plans(8, 64, 20, controls=True, vocab=True)
    with pytest.raises(ValueError):
        cap.decode_plans(8, 64, 20, beam=(3, 1.0, False), vocab=True)
    assert cap._plans == {}
    # neutral controls are no controls; the checked object comes back
    from omniparser_amd.florence import CaptionVocabulary
    v = cap.caption_vocabulary(GOOD, 20, None, cap.generation_controls(dict(repetition_penalty=1.0), 20))
    assert isinstance(v, CaptionVocabulary) and v.labels == ((0, 7, 8, 2), (0, 7, 2))
    assert cap.caption_vocabulary(None, 20) is None and cap.caption_vocabulary(v, 20) is v
    assert CaptionVocabulary.of(None) is None and CaptionVocabulary.of(v) is v and CaptionVocabulary.of(GOOD).labels == v.labels


def test_packed_block_word_for_word():
    import vocab_checks as VC
    VC.check_packed_block()


def _fake_models(monkeypatch):
    from omniparser_amd.util import utils as U
    model = types.SimpleNamespace(token_scores=False)
    monkeypatch.setattr(U, "get_yolo_model", lambda model_path, device: object())
    monkeypatch.setattr(U, "get_caption_model_processor", lambda model_name, model_name_or_path, device: {"model": model, "processor": None})
    return {"som_model_path": "x", "caption_model_name": "florence2", "caption_model_path": "y", "BOX_TRESHOLD": 0.05}


def test_omniparser_validates_caption_vocabulary(monkeypatch):
    from omniparser_amd.util import omniparser as F
    cfg = _fake_models(monkeypatch)
    for bad in ("close", [], {}, 7, [7], [["close"]], [""], [[0, -1, 2]], [[]], ["close", 7]):
        with pytest.raises(ValueError):
            F.Omniparser({**cfg, "caption_vocabulary": bad})
    with pytest.raises(ValueError, match="caption_generation"):
        F.Omniparser({**cfg, "caption_vocabulary": ["close"], "caption_generation": {"repetition_penalty": 1.3}})
    assert F.Omniparser(cfg).caption_vocabulary is None
    assert F.Omniparser({**cfg, "caption_vocabulary": None}).caption_vocabulary is None
    good = ["close", "settings", [0, 7, 2]]
    assert F.Omniparser({**cfg, "caption_vocabulary": good}).caption_vocabulary == good


def test_get_parsed_content_icon_passes_the_vocabulary_through():
    """a fake model: strings are tokenised by the processor, caption_crops gets the CaptionVocabulary, contents are the strings as
    given, confidences come from the constrained log-probabilities"""
    import numpy as np
    from omniparser_amd.florence import CaptionVocabulary, caption_confidence
    from omniparser_amd.util import utils as U
    table = {"close": [0, 7, 2], "settings": [0, 8, 9, 2]}
    calls = []

    def caption_crops(img, boxes, max_new_tokens=20, batch_size=128, return_scores=False, **kw):
        calls.append(dict(kw, max_new_tokens=max_new_tokens))
        ids = torch.tensor([[2, 0, 8, 9, 2], [2, 0, 7, 2, 1], [2, 0, 5, 2, 1]][:len(boxes)])
        lp = torch.tensor([[0.0, -0.5, 0.0, -0.25], [0.0, -1.0, 0.0, 0.0], [0.0, -2.0, 0.0, 0.0]][:len(boxes)])
        return (ids, lp) if return_scores else ids
    model = types.SimpleNamespace(device=torch.device("cpu"), caption_crops=caption_crops,
                                  w=types.SimpleNamespace(eos=2, forced_bos=0, forced_eos=2))
    processor = types.SimpleNamespace(prompt_ids=lambda s: table[s],
                                      batch_decode=lambda ids, skip_special_tokens=True: [f"<{' '.join(map(str, r.tolist()))}>" for r in ids])
    cmp_ = {"model": model, "processor": processor}
    img = np.zeros((64, 64, 3), dtype=np.uint8)
    boxes = torch.tensor([[0.1, 0.1, 0.4, 0.4], [0.5, 0.5, 0.9, 0.9], [0.2, 0.5, 0.4, 0.9]])
    out = U.get_parsed_content_icon(boxes, 0, img, cmp_, vocabulary=["close", "settings", [0, 5, 2], "close"])
    v = calls[0]["vocabulary"]
    assert isinstance(v, CaptionVocabulary) and v.labels == ((0, 7, 2), (0, 8, 9, 2), (0, 5, 2)) and "controls" not in calls[0]
    assert out == ["settings", "close", "<2 0 5 2 1>"]                 # the id-list label has no string: the decoded text
    pairs = U.get_parsed_content_icon(boxes, 0, img, cmp_, vocabulary=["close", "settings", [0, 5, 2]], return_confidence=True)
    assert [p[0] for p in pairs] == out
    want = caption_confidence(torch.tensor([2, 0, 8, 9, 2]), torch.tensor([0.0, -0.5, 0.0, -0.25]), 2, 0, 2, 20)
    assert pairs[0][1] == want
    U.get_parsed_content_icon(boxes, 0, img, cmp_)
    assert "vocabulary" not in calls[-1] and calls[-1]["max_new_tokens"] == 20
    long_ = [0] + list(range(100, 125)) + [2]
    U.get_parsed_content_icon(boxes, 0, img, cmp_, vocabulary=[long_])
    assert calls[-1]["max_new_tokens"] == len(long_)                  # None = 20, or the longest label when that is longer
    for bad in ("close", 7, [7], [[]], []):
        with pytest.raises(ValueError):
            U.get_parsed_content_icon(boxes, 0, img, cmp_, vocabulary=bad)
    nofile = types.SimpleNamespace(prompt_ids=U.FlorenceProcessor(None).prompt_ids, batch_decode=processor.batch_decode)
    with pytest.raises(ValueError, match="tokenizer.json"):
        U.get_parsed_content_icon(boxes, 0, img, {"model": model, "processor": nofile}, vocabulary=["close"])


def test_header_and_python_agree_on_the_op_and_its_block():
    from omniparser_amd import florence as FL
    hdr = (Path(__file__).resolve().parents[1] / "include" / "omni_amd.h").read_text()
    assert re.search(r"OMNI_OP_GREEDY_CTRL_STEP = OMNI_OP__COUNT,\s*/\*.*?\*/\s*/\*.*?\*/\s*OMNI_OP_GREEDY_VOCAB_STEP = OMNI_OP_GREEDY_CTRL_STEP \+ 1,\s*/\* 27\b.*?\*/\s*OMNI_OP__END\s*\}", hdr, re.S)
    assert L.OP_GREEDY_VOCAB_STEP == 27 == L.OP_GREEDY_CTRL_STEP + 1
    # tests/test_host_cpu.py pins the LITERALLY numbered kinds to 1..24: kinds behind OMNI_OP__COUNT are spelled relative to it
    assert len(re.findall(r"\b(OMNI_OP_[A-Z0-9_]+) = (\d+),", hdr)) == 24
    assert "#define OMNI_ABI_VERSION 3" in hdr
    doc = re.search(r"/\* greedy decoding step over a CLOSED VOCABULARY.*?\*/\s*OMNI_OP_GREEDY_VOCAB_STEP = OMNI_OP_GREEDY_CTRL_STEP \+ 1,", hdr, re.S).group(0)
    assert "greedy_vocab_step_kernel" in doc and "p7 trie block" in doc and "i12" in doc and "p5 node" in doc
    assert f"#define OMNI_VOCAB_HEADER_BYTES {4 * FL.VOCAB_HEADER_WORDS}" in hdr
    assert re.search(rf"#define OMNI_VOCAB_MAX_NODES {FL.VOCAB_MAX_NODES}\b", hdr) and FL.VOCAB_MAX_NODES == 65536
    assert re.search(rf"#define OMNI_VOCAB_MAX_LABEL {FL.VOCAB_MAX_LABEL}\b", hdr) and FL.VOCAB_MAX_LABEL == 64
    fields = re.search(r"typedef struct omni_vocab_trie \{(.*?)\} omni_vocab_trie_t;", hdr, re.S).group(1)
    names = re.findall(r"int32_t\s+(\w+)", fields)
    assert names == list(FL.VOCAB_TRIE_FIELDS)

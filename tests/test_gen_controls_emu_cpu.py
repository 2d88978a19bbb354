"""Generation controls of greedy decoding on the host emulation of the HIP kernels (tests/emu) and on the host alone:
OMNI_OP_GREEDY_CTRL_STEP case by case against transformers' own logits processors, generate(repetition_penalty=..., ...) against
transformers' generate, the plan / default-path rules, the argument checks and the packed control block.  Helpers and bounds:
tests/gen_ctrl_checks.py; the MI355X twin: tests/test_gpu_t_gen_controls.py."""
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
def test_repetition_penalty_once_per_seen_token(emu, f16, scores):
    import gen_ctrl_checks as GC
    print(f"worst logp error {GC.check_repetition_penalty(L, CPU, V_EMU, f16, scores):.3f} of the bound")


@BOTH
def test_min_new_tokens_on_both_sides_of_the_boundary(emu, f16, scores):
    import gen_ctrl_checks as GC
    GC.check_min_new_tokens(L, CPU, V_EMU, f16, scores)


@BOTH
def test_suppress_and_begin_suppress(emu, f16, scores):
    import gen_ctrl_checks as GC
    GC.check_suppress(L, CPU, V_EMU, f16, scores)


@BOTH
def test_bad_words(emu, f16, scores):
    import gen_ctrl_checks as GC
    GC.check_bad_words(L, CPU, V_EMU, f16, scores)


@BOTH
def test_ngram_size_comes_from_the_block(emu, f16, scores):
    import gen_ctrl_checks as GC
    GC.check_ngram_from_block(L, CPU, V_EMU, f16, scores)


@BOTH
def test_everything_at_once_forced_positions_and_finished_rows(emu, f16, scores):
    import gen_ctrl_checks as GC
    GC.check_everything_and_forced(L, CPU, V_EMU, f16, scores)


def test_degenerate_rows_give_token_zero(emu):
    import gen_ctrl_checks as GC
    GC.check_degenerate_rows(L, CPU, V_EMU)


@pytest.mark.parametrize("f16", [False, True])
def test_neutral_block_is_bit_identical_to_greedy_step(emu, f16):
    import gen_ctrl_checks as GC
    GC.check_neutral_equals_greedy_step(L, CPU, V_EMU, f16)


def test_short_control_block_is_an_argument_error(emu):
    import gen_ctrl_checks as GC
    seen = GC.check_short_block(L, CPU, V_EMU)
    assert all("control block" in m for m in seen), seen


# ---------------------------------------------------------------------------------------------- whole captioner
# the two cheapest settings that together cover all six controls (emulated steps are slow): every control at once on the EOS-prone
# checkpoint, and the repetition penalty alone on it
@pytest.mark.parametrize("name", ["all", "repetition_penalty"])
def test_controlled_captions_match_transformers_r64_eos_prone(emu, name):
    import gen_ctrl_checks as GC
    GC.captioner_vs_hf(True, name)


def test_reference_outputs_differ_from_the_default(emu):
    import gen_ctrl_checks as GC
    GC.check_not_vacuous()


def test_plans_and_defaults(emu):
    """the MI355X test's plan rules at 8 new tokens: default, two settings on one plan, default again (every call is an emulated
    encode + decode; the neutral call and caption_crops(controls=...) against generate run on the MI355X only)"""
    import gen_ctrl_checks as GC
    GC.check_plans_and_defaults(GC.captioner(True), MAX_NEW=8, n_boxes=0)


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


BAD = [dict(repetition_penalty=0.0), dict(repetition_penalty=-1.3), dict(repetition_penalty=True), dict(repetition_penalty="1.3"),
       dict(repetition_penalty=float("nan")), dict(repetition_penalty=float("inf")),
       dict(no_repeat_ngram_size=-1), dict(no_repeat_ngram_size=2.0), dict(no_repeat_ngram_size=True),
       dict(min_new_tokens=-1), dict(min_new_tokens=21), dict(min_new_tokens=1.0), dict(min_new_tokens=False),
       dict(suppress_tokens=[-1]), dict(suppress_tokens=[51290]), dict(suppress_tokens=[1.0]), dict(suppress_tokens=7),
       dict(suppress_tokens=[True]), dict(begin_suppress_tokens=[51290]), dict(begin_suppress_tokens="7"),
       dict(bad_words_ids=[[]]), dict(bad_words_ids=[[5, 51290]]), dict(bad_words_ids=[list(range(3, 12))]), dict(bad_words_ids=[5]),
       dict(bad_words_ids=[[3 + k, 9] for k in range(65)]),
       dict(suppress_tokens=[2]), dict(suppress_tokens=[0]), dict(begin_suppress_tokens=[2]), dict(begin_suppress_tokens=[0]),
       dict(bad_words_ids=[[2]]), dict(bad_words_ids=[[0]])]


@pytest.mark.parametrize("kw", BAD, ids=[f"{next(iter(d))}-{n}" for n, d in enumerate(BAD)])
def test_bad_controls_are_value_errors_before_any_device_work(host_cap, kw):
    cap = host_cap
    assert cap.w.vocab == 51290 and (cap.w.eos, cap.w.forced_bos, cap.w.forced_eos) == (2, 0, 2)
    pix = torch.zeros(1, 3, 64, 64)
    frame = torch.zeros(64, 64, 3, dtype=torch.uint8)
    with pytest.raises(ValueError):
        cap.generate(pixel_values=pix, max_new_tokens=20, **kw)
    with pytest.raises(ValueError):
        cap.caption_crops(frame, [[0, 0, 8, 8]], max_new_tokens=20, controls=kw)
    assert cap._plans == {}


def test_limits_that_are_still_allowed(host_cap):
    from omniparser_amd.florence import GenerationControls
    cap = host_cap
    gc = cap.generation_controls(dict(repetition_penalty=1, min_new_tokens=20, bad_words_ids=[[3 + k, 9] for k in range(63)] + [[k] for k in range(3, 200)]
                                      + [list(range(3, 11))], suppress_tokens=torch.tensor([51289])), 20)
    assert isinstance(gc, GenerationControls) and gc.repetition_penalty == 1.0 and not gc.neutral
    assert cap.generation_controls(None, 20) is None and cap.generation_controls({}, 20) is None
    assert cap.generation_controls(dict(repetition_penalty=1.0, min_new_tokens=0, suppress_tokens=[], bad_words_ids=[]), 20) is None
    assert cap.generation_controls(dict(no_repeat_ngram_size=0), 20) is not None          # 0 switches the checkpoint's ban off
    with pytest.raises(ValueError, match="unknown generation control"):
        cap.generation_controls(dict(temperature=0.7), 20)
    with pytest.raises(ValueError):
        cap.generation_controls([1.3], 20)


def test_beam_search_with_controls_is_refused(host_cap):
    cap = host_cap
    pix = torch.zeros(1, 3, 64, 64)
    with pytest.raises(ValueError, match="beam search"):
        cap.generate(pixel_values=pix, num_beams=3, repetition_penalty=1.3)
    with pytest.raises(ValueError, match="beam search"):
        cap.caption_crops(torch.zeros(64, 64, 3, dtype=torch.uint8), [[0, 0, 8, 8]], num_beams=3, controls=dict(min_new_tokens=3))
    with pytest.raises(ValueError):
        cap.plans(8, 64, 20, beam=(3, 1.0, False), controls=True)
    assert cap._plans == {}


def _fake_models(monkeypatch):
    from omniparser_amd.util import utils as U
    model = types.SimpleNamespace(token_scores=False)
    monkeypatch.setattr(U, "get_yolo_model", lambda model_path, device: object())
    monkeypatch.setattr(U, "get_caption_model_processor", lambda model_name, model_name_or_path, device: {"model": model, "processor": None})
    return {"som_model_path": "x", "caption_model_name": "florence2", "caption_model_path": "y", "BOX_TRESHOLD": 0.05}


def test_omniparser_validates_caption_generation(monkeypatch):
    from omniparser_amd.util import omniparser as F
    cfg = _fake_models(monkeypatch)
    for bad in ("{}", [1.3], 1.3, {"temperature": 1.0}, {"repetition_penalty": 0}, {"bad_words_ids": [[]]}, {"min_new_tokens": True}):
        with pytest.raises(ValueError):
            F.Omniparser({**cfg, "caption_generation": bad})
    assert F.Omniparser(cfg).caption_generation is None
    assert F.Omniparser({**cfg, "caption_generation": None}).caption_generation is None
    good = {"repetition_penalty": 1.3, "bad_words_ids": [[5, 6]]}
    assert F.Omniparser({**cfg, "caption_generation": good}).caption_generation == good


def test_describe_image_passes_generation_to_generate_and_refuses_bad_ones():
    from PIL import Image
    from omniparser_amd.util import utils as U
    calls = []
    proc = types.SimpleNamespace(
        __call__=None, batch_decode=lambda ids, skip_special_tokens=True: ["x"] * len(ids))
    processor = lambda images, text, return_tensors, do_resize: {"input_ids": torch.zeros(1, 4), "pixel_values": torch.zeros(1, 3, 64, 64),
                                                                 "attention_mask": torch.ones(1, 4)}
    processor.batch_decode = proc.batch_decode
    model = types.SimpleNamespace(resolution=64, generate=lambda **k: calls.append(k) or torch.zeros(1, 3, dtype=torch.long))
    cmp_ = {"model": model, "processor": processor}
    img = Image.new("RGB", (32, 24))
    for bad in ({"temperature": 1.0}, {"repetition_penalty": -1}, "x", [1]):
        with pytest.raises(ValueError):
            U.describe_image(img, cmp_, task="<CAPTION>", generation=bad)
    assert calls == []
    U.describe_image(img, cmp_, task="<CAPTION>", generation={"repetition_penalty": 1.3, "min_new_tokens": 4})
    U.describe_image(img, cmp_, task="<CAPTION>")
    assert calls[0]["repetition_penalty"] == 1.3 and calls[0]["min_new_tokens"] == 4
    assert "repetition_penalty" not in calls[1] and set(calls[1]) == set(calls[0]) - {"repetition_penalty", "min_new_tokens"}


def test_packed_block_word_for_word():
    import gen_ctrl_checks as GC
    GC.check_packed_block()


def test_header_and_python_agree_on_the_op_and_its_block():
    from omniparser_amd import florence as FL
    hdr = (Path(__file__).resolve().parents[1] / "include" / "omni_amd.h").read_text()
    assert re.search(r"OMNI_OP_BEAM_STEP,\s*OMNI_OP__COUNT,\s*/\*.*?\*/\s*/\*.*?\*/\s*OMNI_OP_GREEDY_CTRL_STEP = OMNI_OP__COUNT,\s*/\*.*?\*/\s*OMNI_OP__END\s*\}", hdr, re.S)
    assert L.OP_GREEDY_CTRL_STEP == 26 == L.OP_BEAM_STEP + 1
    assert "#define OMNI_ABI_VERSION 3" in hdr
    doc = re.search(r"/\* greedy decoding step WITH GENERATION CONTROLS.*?\*/\s*OMNI_OP_GREEDY_CTRL_STEP = OMNI_OP__COUNT,", hdr, re.S).group(0)
    assert "greedy_ctrl_step_kernel" in doc and "p7 control block" in doc and "i12" in doc
    assert f"#define OMNI_GEN_CTRL_HEADER_BYTES {4 * FL.GEN_CTRL_HEADER_WORDS}" in hdr
    assert re.search(rf"#define OMNI_GEN_CTRL_MAX_BAD {FL.GEN_CTRL_MAX_BAD}\b", hdr)
    assert re.search(rf"#define OMNI_GEN_CTRL_MAX_BAD_LEN {FL.GEN_CTRL_MAX_BAD_LEN}\b", hdr)
    fields = re.search(r"typedef struct omni_gen_ctrl \{(.*?)\} omni_gen_ctrl_t;", hdr, re.S).group(1)
    names = re.findall(r"(?:float|int32_t)\s+(\w+)", fields)
    assert names == ["penalty", "ngram", "min_new_tokens", "begin_index", "n_bad", "bad_stride", "reserved"]

"""The caller's prompt in the Florence-2 captioner, on the host emulation of the kernels: the OMNI_OP_ASSEMBLE gather, the
per-row key counts of OMNI_OP_ATTN_ROWS (mode 0) and OMNI_OP_ATTN_DECODE (cross), the captioner against transformers with uniform
and ragged prompts (greedy and beam search), and the host side of the public interface.  Helpers, prompts and the margin rule:
tests/prompt_checks.py.  The full-vocabulary lm_head costs the emulation 15 G multiply-adds per decode step, so the end-to-end
cases are small (as tests/test_models_emu_cpu.py::test_captioner_token_exact_r64); the 21-token loops over real crop batches run on
the MI355X (tests/test_gpu_m_prompt.py)."""
from pathlib import Path

import pytest
import torch

from omniparser_amd import _lib as L

MAX_NEW = 4          # steps 1 and 2 are free arg-maxes (0: forced bos, 3: forced eos)


# ------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("dtype", [L.F32, L.F16])
def test_assemble_gathers_prompt_rows(emu, dtype):
    import prompt_checks as P
    P.check_assemble_gather(dtype)
    P.check_assemble_gather(dtype, B=2, n_img=3, n_txt=8, C=64, V=50, scale=1.0)


def test_assemble_refuses_half_given_prompt_slots(emu):
    t = torch.zeros(64)
    i32 = torch.zeros(8, dtype=torch.int32)
    for p in ([t.data_ptr(), t.data_ptr(), i32.data_ptr(), t.data_ptr(), t.data_ptr()],      # constant block AND ids
              [t.data_ptr(), None, i32.data_ptr(), None, t.data_ptr()],                      # ids without the table
              [t.data_ptr(), None, None, None, t.data_ptr()]):                               # neither
        with pytest.raises(L.OmniError):
            L.launch(L.make_op(L.OP_ASSEMBLE, L.F32, p=p, i={0: 1, 1: 1, 2: 1, 3: 8, 4: 4}))


# (plan dtype, head_dim) -> the kernel that serves mode 0: attn_rows_kernel (head_dim 32), mha_mfma_f32_kernel, mha_mfma_kernel;
# tile = keys per LDS tile of that kernel (a count on its boundary is one of the cases)
MODE0 = [(L.F32, 32, 48), (L.F16, 32, 48), (L.F32, 64, 64), (L.F16, 64, 32)]


@pytest.mark.parametrize("dtype,D,tile", MODE0)
@pytest.mark.parametrize("n_img,n_txt,heads,groups", [(5, 8, 12, 4), (5, 32, 12, 5), (5, 64, 12, 5), (577, 64, 2, 3)])
def test_masked_encoder_attention(emu, dtype, D, tile, n_img, n_txt, heads, groups):
    import prompt_checks as P
    P.check_attn_rows_masked(dtype, D, heads, n_img, n_txt, groups, tile)


@pytest.mark.parametrize("dtype,aligned", [(L.F32, True), (L.F32, False), (L.F16, True)])
@pytest.mark.parametrize("n_img,n_txt,heads,crops", [(5, 8, 12, 4), (5, 64, 12, 5), (577, 64, 2, 3)])
@pytest.mark.parametrize("kv_div", [1, 3])
def test_masked_decode_cross_attention(emu, dtype, aligned, n_img, n_txt, heads, crops, kv_div):
    import prompt_checks as P
    P.check_attn_decode_cross_masked(dtype, heads, n_img, n_txt, crops, kv_div, aligned)


def test_attn_rows_table_is_for_mode0(emu):
    t = torch.zeros(144 * 96)
    nk = torch.full((1,), 144, dtype=torch.int32)
    with pytest.raises(L.OmniError):
        L.launch(L.make_op(L.OP_ATTN_ROWS, L.F32, p=[t.data_ptr()] * 3 + [None, t.data_ptr(), None, None, nk.data_ptr()],
                           i={0: 96, 1: 96, 2: 96, 3: 96, 5: 32, 6: 64, 8: 1, 9: 144, 10: 144, 11: 1, 12: 1, 13: 12, 14: 12, 15: 32}, f={0: 1.0}))


# ------------------------------------------------------------------------------------------ captioner vs transformers
@pytest.fixture(scope="module")
def oracle():
    from tools.make_weights import shared_random_captioner
    return shared_random_captioner(0)


def _captioner():
    from omniparser_amd.florence import Florence2Captioner
    from tools.make_weights import ensure_caption_checkpoint
    return Florence2Captioner(ensure_caption_checkpoint(0), "cuda", precision="f32", resolution=64)


def test_uniform_prompt_token_exact_r64(emu, oracle):
    """a non-default prompt for every row: ids equal transformers' and differ from the default prompt's"""
    import prompt_checks as P
    pix, _, _ = P.real_pixels(64, 2)
    rows = [P.PROMPTS[11]] * 2
    ref, margins = P.oracle_generate(oracle, pix, rows, MAX_NEW)
    P.assert_margins(margins, "uniform 11 @64")
    dflt, _ = P.oracle_generate(oracle, pix, [P.PROMPT_IDS] * 2, MAX_NEW)
    assert not torch.equal(ref, dflt), "the oracle itself does not react to this prompt: the test would show nothing"
    cap = _captioner()
    ids, _ = P.hf_inputs(oracle, 64, rows)
    got = cap.generate(input_ids=ids, pixel_values=pix, max_new_tokens=MAX_NEW)          # no mask: every column counts
    P.tally_rows(oracle, 64, got, ref, margins, "uniform11")
    cp = cap.plans(cap.bucket(2), 64, MAX_NEW, n_txt=16)
    assert cp.n_txt == 16 and cp.S == 5 + 16 and len(cap._plans) == 1                     # smallest capacity that holds 11 tokens


def test_ragged_prompts_token_exact_and_equal_solo_r64(emu, oracle):
    """a ragged batch with an attention mask equals transformers, greedy and with num_beams=3; every row equals the same prompt
    run alone (on the plan of its own capacity)"""
    import prompt_checks as P
    pix, _, _ = P.real_pixels(64, 3)
    rows = [P.PROMPTS[5], P.PROMPTS[29], P.PROMPTS[11]]
    ref, margins = P.oracle_generate(oracle, pix, rows, MAX_NEW)
    P.assert_margins(margins, "ragged 5/29/11 @64")
    cap = _captioner()
    ids, mask = P.hf_inputs(oracle, 64, rows)
    got = cap.generate(input_ids=ids, attention_mask=mask, pixel_values=pix, max_new_tokens=MAX_NEW)
    P.tally_rows(oracle, 64, got, ref, margins, "ragged")
    for b, r in enumerate(rows):
        i1, _ = P.hf_inputs(oracle, 64, [r])
        solo = cap.generate(input_ids=i1, pixel_values=pix[b:b + 1], max_new_tokens=MAX_NEW)
        T = min(solo.shape[1], got.shape[1])
        assert torch.equal(solo[0, :T], got[b, :T]) and bool((got[b, T:] == P.PAD).all()), (b, solo, got[b])
    refb, _ = P.oracle_generate(oracle, pix[:2], rows[:2], MAX_NEW, num_beams=3)
    gotb = cap.generate(input_ids=ids[:2], attention_mask=mask[:2], pixel_values=pix[:2], max_new_tokens=MAX_NEW, num_beams=3)
    assert gotb.shape == refb.shape and torch.equal(gotb, refb), (gotb, refb)


def test_screen_parser_caption_with_prompt_merged_and_twin(emu, monkeypatch):
    """ScreenParser.caption(prompt=) over more crops than a micro-batch holds: prompt ids and key counts written into every
    micro-batch's plan (the remainder runs as an exact-row twin in the full plan's buffers), the key counts merged into the decode
    plan — the ids caption_crops(prompt_ids=) gives per micro-batch, different from the default prompt's, and the default
    prompt's plans stay what they were.  Small token table and three decode steps (one free arg-max), as
    test_models_emu_cpu.py::test_merged_decode_equals_per_micro_batch_decode."""
    import omniparser_amd.florence as FL
    from conftest import small_vocab_caption_checkpoint
    from omniparser_amd.pipeline import ScreenParser
    from omniparser_amd.synth import synthetic_screenshot
    cap = FL.Florence2Captioner(small_vocab_caption_checkpoint(0), "cuda", precision="f32", resolution=64)
    monkeypatch.setattr(FL.Florence2Captioner, "decode_bucket", staticmethod(lambda n: 8))
    monkeypatch.setattr(FL, "_BUCKETS", (2, 128))
    frame = torch.from_numpy(synthetic_screenshot(3, 640, 480))
    rects = [[[10, 20, 60, 70], [300, 200, 340, 260], [500, 100, 620, 140]], [[40, 40, 90, 80], [200, 300, 280, 360]]]
    prompt = [0] + [4 + (37 * k) % 8000 for k in range(9)] + [2]                # 11 tokens: capacity 16
    strip = lambda rows: [[t for t in r if t != cap.w.pad] for r in rows]
    sp = ScreenParser(None, cap, batch_size=2)
    sp.max_new_tokens = 3
    runs = [[[row.tolist() for _, row in f] for f in sp.caption([frame, frame], rects, prompt=prompt)] for _ in range(2)]
    assert runs[0] == runs[1]
    dec = next(v for k, v in cap._plans.items() if k[0] == "dec")
    assert dec.n_txt == 16 and dec.nkeys[:5].tolist() == [5 + 11] * 5 and dec.nkeys[5:].tolist() == [5 + 16] * 3
    cp = cap._plans[(2, 64, 3, 0, None, ("txt", 16))]
    assert cap.row_graph_builds == 1 and sorted(cp._row_plans) == [1]             # the second run's remainder: an exact-row twin
    assert cp._row_plans[1].prompt_ids.data_ptr() == cp.prompt_ids.data_ptr() and cp._row_plans[1].n_txt == 16
    flat = [r for f in rects for r in f]
    solo = cap.caption_crops(frame, flat, max_new_tokens=3, batch_size=2, prompt_ids=prompt)
    assert strip([r for f in runs[0] for r in f]) == strip(solo.tolist())
    dflt = [[row.tolist() for _, row in f] for f in sp.caption([frame, frame], rects)]
    assert strip([r for f in dflt for r in f]) == strip(cap.caption_crops(frame, flat, max_new_tokens=3, batch_size=2).tolist())
    assert cap._plans[(2, 64, 3)].nkeys is None
    assert strip([r for f in dflt for r in f]) != strip([r for f in runs[0] for r in f]), "the prompt changed no caption"
    print("prompt", runs[0], "default", dflt)


# ------------------------------------------------------------------------------------------ host side
def test_task_table_matches_transformers():
    import inspect
    from transformers.models.florence2 import processing_florence2 as PF
    from omniparser_amd.util import utils as U
    src = inspect.getsource(PF.Florence2Processor.__init__)
    for tk, sentence in U.TASK_PROMPTS.items():
        assert f'"{tk}": "{sentence}"' in src, tk
    assert src.count('": "', src.index("task_prompts_without_inputs"), src.index("task_prompts_with_input")) == len(U.TASK_PROMPTS)
    for tk in U.TASKS_WITH_INPUT:
        assert f'"{tk}": "' in src[src.index("task_prompts_with_input"):], tk


def _synth_dir(tmp_path):
    import shutil
    src = Path(__file__).resolve().parent / "golden" / "tokenizer_synth" / "tokenizer.json"
    shutil.copy(src, tmp_path / "tokenizer.json")
    return tmp_path


def test_processor_prompts(tmp_path):
    from PIL import Image
    from omniparser_amd.florence import PROMPT_IDS
    from omniparser_amd.util import utils as U
    bare = U.FlorenceProcessor(None)
    assert bare.prompt_ids(None) == PROMPT_IDS and bare.prompt_ids("<CAPTION>") == PROMPT_IDS
    with pytest.raises(ValueError, match="tokenizer.json"):
        bare.prompt_ids("<DETAILED_CAPTION>")
    with pytest.raises(ValueError, match="tokenizer.json"):
        U.FlorenceProcessor(tmp_path / "nowhere").prompt_ids("what is this?")
    proc = U.FlorenceProcessor(_synth_dir(tmp_path))
    assert proc.prompt_ids(None) == PROMPT_IDS and proc.prompt_ids("<CAPTION>") == PROMPT_IDS      # unchanged with a tokenizer too
    for tk, sentence in U.TASK_PROMPTS.items():
        if tk == "<CAPTION>":
            continue
        ids = proc.prompt_ids(tk)
        assert ids == proc.prompt_ids(sentence) and ids[0] == 0 and ids[-1] == 2
        assert len(ids) <= 64 and max(ids) < 400, (tk, len(ids))                # fits the largest text capacity; the fixture's vocabulary
        if "CAPTION" in tk and "REGION" not in tk:
            assert 25 <= len(ids) <= 36, (tk, len(ids))                        # the caption sentences with this tokenizer (20 .. 43 over all eight)
        assert proc.tok.decode(ids[1:-1]) == sentence                                              # round trip
    for tk in U.TASKS_WITH_INPUT:
        with pytest.raises(ValueError, match="needs an input"):
            proc.prompt_ids(tk + " a button")
    with pytest.raises(ValueError, match="only content"):
        proc.prompt_ids("<OCR> please")
    im = Image.new("RGB", (64, 64))
    one = proc(images=[im, im], text="<OCR>", do_resize=False)
    assert one["input_ids"].shape == (2, 5 + len(proc.prompt_ids("<OCR>"))) and bool(one["attention_mask"].all())
    assert one["input_ids"][0, :5].tolist() == [proc.image_token_id] * 5
    dflt = proc(images=im, do_resize=False)
    assert dflt["input_ids"][0].tolist() == [proc.image_token_id] * 5 + PROMPT_IDS
    a, b = proc.prompt_ids("<OCR>"), proc.prompt_ids("close window")
    two = proc(images=[im, im], text=["<OCR>", "close window"], do_resize=False)
    assert len(a) > len(b)
    assert two["input_ids"][1, 5:].tolist() == b + [1] * (len(a) - len(b))
    assert two["attention_mask"][1].tolist() == [1] * (5 + len(b)) + [0] * (len(a) - len(b)) and bool(two["attention_mask"][0].all())
    with pytest.raises(ValueError, match="prompts for"):
        proc(images=[im, im], text=["<OCR>"], do_resize=False)


def test_generate_refuses_bad_prompts(emu):
    from omniparser_amd.florence import PROMPT_IDS, text_capacity
    cap = _captioner()
    pix = torch.zeros(2, 3, 64, 64)
    img = [int(cap.w.cfg.get("image_token_id", 51289))] * 5
    vocab = cap.w.sd["model.language_model.shared.weight"].shape[0]
    gen = lambda ids, **k: cap.generate(input_ids=torch.tensor(ids), pixel_values=pix, max_new_tokens=2, **k)
    with pytest.raises(ValueError, match="image placeholder"):
        gen([[0] * 5 + PROMPT_IDS] * 2)
    with pytest.raises(ValueError, match="image placeholder"):
        gen([img] * 2)                                                   # no prompt at all
    with pytest.raises(ValueError, match="one row per image"):
        gen([img + PROMPT_IDS])
    with pytest.raises(ValueError, match="right-padded"):
        gen([img + [0, 7, 2], img + [1, 0, 2]], attention_mask=torch.tensor([[1] * 8, [1] * 5 + [0, 1, 1]]))
    with pytest.raises(ValueError, match="hides image"):
        gen([img + [0, 7, 2]] * 2, attention_mask=torch.tensor([[0] + [1] * 7] * 2))
    with pytest.raises(ValueError, match="does not match"):
        gen([img + [0, 7, 2]] * 2, attention_mask=torch.ones(2, 7))
    with pytest.raises(ValueError, match="outside the token table"):
        gen([img + [0, vocab, 2]] * 2)
    with pytest.raises(ValueError, match="outside the token table"):
        gen([img + [0, -1, 2]] * 2)
    with pytest.raises(ValueError, match="limit of 64"):
        gen([img + [0] + [7] * 63 + [2]] * 2)
    with pytest.raises(ValueError, match="attention_mask without"):
        cap.generate(pixel_values=pix, attention_mask=torch.ones(2, 13))
    with pytest.raises(ValueError, match="empty prompt"):
        cap.prompt_batch([[]], 64)
    with pytest.raises(ValueError, match="limit of 64"):
        cap.caption_crops(torch.zeros(100, 100, 3, dtype=torch.uint8), [[0, 0, 10, 10]], prompt_ids=[0] + [9] * 70 + [2])
    assert [text_capacity(n) for n in (1, 8, 9, 16, 17, 33, 64)] == [8, 8, 16, 16, 32, 64, 64]
    assert not cap._plans                                                # nothing was built on the way to an error
    # the default prompt given explicitly is the default plan: no capacity, no table
    assert cap.prompt_batch([PROMPT_IDS] * 3, 64) is None
    ids, nkeys, n_txt = cap.prompt_batch([[0, 9, 2], PROMPT_IDS], 64)
    assert n_txt == 8 and nkeys.tolist() == [8, 13] and ids[0].tolist() == [0, 9, 2, 1, 1, 1, 1, 1]


def test_get_parsed_content_icon_passes_the_prompt(tmp_path):
    import numpy as np
    from omniparser_amd.util import utils as U
    seen = []

    class Cap:
        device = torch.device("cpu")

        def caption_crops(self, image, boxes, max_new_tokens=20, batch_size=128, **kw):
            seen.append(kw)
            return torch.zeros(len(boxes), 1, dtype=torch.long)
    proc = U.FlorenceProcessor(_synth_dir(tmp_path))
    cmp_ = {"model": Cap(), "processor": proc}
    img = np.zeros((100, 200, 3), dtype=np.uint8)
    boxes = torch.tensor([[0.1, 0.1, 0.3, 0.4]])
    for prompt in (None, "<CAPTION>"):
        U.get_parsed_content_icon(boxes, None, img, cmp_, prompt=prompt)
        assert seen[-1] == {}                                            # exactly today's call: captioners without the keyword keep working
    U.get_parsed_content_icon(boxes, None, img, cmp_, prompt="<DETAILED_CAPTION>")
    assert seen[-1] == {"prompt_ids": proc.prompt_ids("<DETAILED_CAPTION>")}
    U.get_parsed_content_icon(boxes, None, img, cmp_, prompt="close window")
    assert seen[-1] == {"prompt_ids": proc.prompt_ids("close window")}

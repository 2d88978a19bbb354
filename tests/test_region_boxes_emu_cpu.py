"""Grounding on the host emulation of the HIP kernels (tests/emu) and on the host alone: OMNI_OP_REGION_OCR mode 3 case by case —
bit-equal to a literal host restatement and equal to transformers' three box parses — the ownership rule, the argument checks, modes
0 / 1 / 2 as before, and the host surface (task_prompt_ids, quantize_box, parse_box_answer, locate, ground_elements, describe_regions,
the /locate/ route) over a stand-in for the encode and the decode.  Helpers: tests/box_checks.py; the MI355X twin with the real
captioner: tests/test_gpu_y_region_boxes.py."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from omniparser_amd import _lib as L

CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def tok_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("region_boxes")


# ---------------------------------------------------------------------------------------------- kernel, one launch per case
@pytest.mark.parametrize("grammar", [0, 1])
@pytest.mark.parametrize("n", [1, 3, 17])
@pytest.mark.parametrize("T", [6, 10, 19, 65, 1025])
def test_boxes_are_the_twin_and_transformers(emu, tok_dir, T, n, grammar):
    import box_checks as BX
    BX.check_boxes(L, CPU, tok_dir, T, n, grammar)


@pytest.mark.parametrize("grammar", [0, 1])
def test_boxes_without_log_probabilities(emu, tok_dir, grammar):
    import box_checks as BX
    BX.check_boxes(L, CPU, tok_dir, 65, 23, grammar, with_logp=False)


@pytest.mark.parametrize("grammar", [0, 1])
def test_boxes_at_the_other_resolution(emu, tok_dir, grammar):
    import box_checks as BX
    names = BX.check_boxes(L, CPU, tok_dir, 65, 23, grammar, R=768)
    assert set(names) == set(BX.gen_cases(65))              # 23 rows: every listed case once


@pytest.mark.parametrize("text_share", [0.05, 0.2, 0.5])
@pytest.mark.parametrize("grammar", [0, 1])
def test_random_rows_are_the_twin_and_transformers(emu, tok_dir, grammar, text_share):
    import box_checks as BX
    assert BX.check_random(L, CPU, tok_dir, grammar, text_share) > 100


def test_the_listed_rows_give_what_the_list_says(emu, tok_dir):
    import box_checks as BX
    BX.check_expected(L, CPU, tok_dir)


def test_ownership_on_a_3x2_grid_and_exactly_on_the_boundaries(emu, tok_dir):
    import box_checks as BX
    BX.check_ownership(L, CPU, tok_dir)


def test_box_argument_errors(emu, tok_dir):
    import box_checks as BX
    seen = BX.check_errors(L, CPU, tok_dir)
    assert all("region_ocr" in msg for _, msg in seen), seen
    msgs = dict(seen)
    assert "(T - 1) / 4" in msgs["mode 1's M"] and "grammar" in msgs["grammar 2"] and "mode 2" in msgs["mode 2"]


def test_modes_0_1_and_2_behave_as_before(emu, tok_dir):
    import region_checks as RC
    RC.check_parse(L, CPU, tok_dir, 19, 3)
    RC.check_cut(L, CPU, "six_tiles", False)
    seen = dict(RC.check_parse_errors(L, CPU, tok_dir))     # mode 2 with mode-1 arguments among them
    assert "region_ocr" in seen["mode 2"]


def test_header_python_and_profiler_agree_on_mode_3():
    from omniparser_amd import florence as FL
    from omniparser_amd import opwork
    hdr = (Path(__file__).resolve().parents[1] / "include" / "omni_amd.h").read_text()
    doc = re.search(r"/\* REGION OCR.*?\*/\s*OMNI_OP_REGION_OCR = ", hdr, re.S).group(0)
    for word in ("i0 = 3", "region_boxes_kernel", "(T - 1) / 4", "i9 = grammar", "n_content", "cloc", "lead", "phrases found"):
        assert word in doc, word
    assert (L.OCR_MODE_CUT, L.OCR_MODE_PARSE, L.OCR_MODE_BOXES) == (0, 1, 3)
    assert [FL.box_slots(t) for t in (2, 4, 5, 6, 19, 65, 1025, 2049)] == [0, 0, 1, 1, 4, 16, 256, 512]
    op = FL.box_parse_op(1, 2, 3, 4, 5, 6, 7, 6, 1025, 51289, 768, 2, 1)
    assert op.kind == L.OP_REGION_OCR and op.i[0] == 3 and op.i[3] == 256 and op.i[9] == 1
    assert opwork.op_kernel(op) == "region_ocr (boxes)" and opwork.op_shape(op) == (6, 1025, 0)
    assert opwork.op_work(op) == (0, 6 * (4 * 1025 + 4 * 1024 + 72 * 256 + 40))
    op.p[2] = None
    assert opwork.op_work(op) == (0, 6 * (4 * 1025 + 72 * 256 + 40))


# ---------------------------------------------------------------------------------------------- host side, no device
@pytest.fixture(scope="module")
def hf_processor(tok_dir):
    """transformers' Florence2Processor over the synthetic tokenizer with the location tokens (for `_construct_prompts`)"""
    import warnings
    import region_checks as RC
    from transformers import CLIPImageProcessor, PreTrainedTokenizerFast
    from transformers.models.florence2.processing_florence2 import Florence2Processor
    d = RC.write_tokenizer(Path(tok_dir) / "tok_hf")
    tok = PreTrainedTokenizerFast(tokenizer_file=str(d / "tokenizer.json"), bos_token="<s>", eos_token="</s>", pad_token="<pad>", unk_token="<unk>")
    tok.image_token, tok.image_token_id = "<image>", 1400
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ip = CLIPImageProcessor()
    ip.image_seq_length = 5
    return Florence2Processor(ip, tok), tok


def test_task_prompt_ids_are_the_tokenizer_on_transformers_sentences(tok_dir, hf_processor):
    import region_checks as RC
    from omniparser_amd.util import utils as U
    proc, _post = RC.oracle(tok_dir)
    hf, tok = hf_processor
    post = hf.post_processor
    for task, text in (("<OPEN_VOCABULARY_DETECTION>", "the AB button"), ("<CAPTION_TO_PHRASE_GROUNDING>", "  A B and CD  ")):
        sentence = hf._construct_prompts([task + text])[0]
        assert task not in sentence and text.strip() in sentence
        want = tok(tok.bos_token + sentence + tok.eos_token, add_special_tokens=False)["input_ids"]
        assert proc.task_prompt_ids(task, text=text) == want and want[0] == RC.BOS and want[-1] == RC.EOS, task
    for task in U.TASKS_WITH_REGION:
        for region, size in (([8, 16, 24.5, 63], (64, 64)), ([0, 0, 768, 768], (768, 768)), ([100, 7, 300, 500], (768, 512))):
            bins = post.quantize(torch.tensor([region], dtype=torch.float32), size)[0].tolist()
            sentence = hf._construct_prompts([task + "".join(f"<loc_{b}>" for b in bins)])[0]
            want = tok(tok.bos_token + sentence + tok.eos_token, add_special_tokens=False)["input_ids"]
            got = proc.task_prompt_ids(task, region=region, size=size)
            assert got == want and sum(1 for t in got if RC.LOC0 <= t < RC.LOC0 + 1000) == 4, (task, region)
    good = dict(region=[1, 2, 3, 4], size=(64, 64))
    for task, kw in (("<REFERRING_EXPRESSION_SEGMENTATION>", dict(text="a")), ("<REGION_TO_SEGMENTATION>", good), ("<OD>", {}), ("<OCR>", {}),
                     ("<OPEN_VOCABULARY_DETECTION>", {}), ("<OPEN_VOCABULARY_DETECTION>", good), ("<REGION_TO_OCR>", dict(text="a")),
                     ("<REGION_TO_OCR>", dict(region=[1, 2, 3, 4])), ("<REGION_TO_OCR>", dict(region=[1, 2, 3], size=(64, 64)))):
        with pytest.raises(ValueError):
            proc.task_prompt_ids(task, **kw)
    with pytest.raises(ValueError, match="tokenizer.json"):
        U.FlorenceProcessor(None).task_prompt_ids("<OPEN_VOCABULARY_DETECTION>", text="a")
    for tk in U.TASKS_WITH_INPUT:                           # `prompt_ids` itself keeps refusing them
        with pytest.raises(ValueError, match="needs an input"):
            proc.prompt_ids(tk + " a button")


@pytest.mark.parametrize("size", [64, 768])
def test_quantize_box_is_transformers_for_every_coordinate(size, hf_processor):
    from omniparser_amd.util import utils as U
    post = hf_processor[0].post_processor
    xs = torch.arange(size + 1, dtype=torch.float32)
    ref = post.quantize(torch.stack([xs, xs, xs, xs], dim=1), (size, size))
    mine = [U.FlorenceProcessor.quantize_box([x, x, x, x], (size, size)) for x in range(size + 1)]
    assert mine == ref.tolist()
    plain = [x * 1000 // size for x in range(size + 1)]
    differs = [x for x in range(size + 1) if min(plain[x], 999) != mine[x][0]]
    assert differs == ([8, 16, 24, 32, 48, 56] if size == 64 else [])       # the plain integer form is NOT the post-processor's
    assert U.FlorenceProcessor.quantize_box([-5, 0.5, 1e9, 63.99], (64, 64)) == post.quantize(torch.tensor([[-5, 0.5, 1e9, 63.99]]), (64, 64))[0].tolist()


def test_parse_box_answer_is_transformers_on_hard_rows(tok_dir):
    import box_checks as BX
    import region_checks as RC
    from omniparser_amd.util import utils as U
    proc, post = RC.oracle(tok_dir)
    enc = lambda s: proc.tok.encode(s, add_special_tokens=False).ids       # noqa: E731
    A, B, C, NL, LT = RC.A, RC.B, RC.C, RC.TOK_NL, RC.TOK_LT
    rows = [[A, NL, B] + BX.BOX_A, [A, LT] + BX.BOX_A, [A] + BX.BOX_A[:3] + [NL] + BX.BOX_B, [NL] + BX.BOX_A + BX.BOX_B + [B, C] + BX.BOX_C,
            enc("A<ground>B") + BX.BOX_A + enc("<obj>C") + BX.BOX_B, enc("AB<od>C") + BX.BOX_A, enc("<box>") + BX.BOX_A + [A] + BX.BOX_B[:3] + [B] + BX.BOX_C,
            [A, B] + BX.BOX_A + BX.BOX_B + [RC.PAD, C] + BX.BOX_C + BX.BOX_A[:2], BX.BOX_A + BX.BOX_B[:1], [RC.SP, A, RC.SP] + BX.BOX_A]
    for g in rows:
        row = [RC.START, RC.BOS] + g + [RC.EOS] + BX.BOX_A + [A]
        for grammar in (0, 1):
            got = [(b["label"], b["bbox"]) for b in U.parse_box_answer(row, proc, (64, 48), grammar)]
            end = row.index(RC.EOS, 1)
            text, _ = post.decode_with_spans(row[1:end])
            want = [(b["cat_name"], [int(v) for v in b["bbox"]])
                    for b in post.parse_description_with_bboxes_from_text_and_spans(text, (64, 48), allow_empty_phrase=grammar == 1)]
            assert got == want, (g, grammar, got, want)
            if grammar == 0:
                ground = [(b["cat_name"], [int(v) for v in box]) for b in post.parse_phrase_grounding_from_text_and_spans(text, (64, 48)) for box in b["bbox"]]
                assert got == ground
    one = U.parse_box_answer([RC.START, A, B] + BX.BOX_A + BX.BOX_B + [RC.EOS], proc, (64, 64), 0)
    assert [b["phrase"] for b in one] == [0, 0] and one[0]["phrase_columns"] == [1, 2] and [b["box_columns"] for b in one] == [[3, 4, 5, 6], [7, 8, 9, 10]]
    for bad in (2, -1, True, None):
        with pytest.raises(ValueError, match="grammar"):
            U.parse_box_answer([RC.START, A], proc, (64, 64), bad)


# ---------------------------------------------------------------------------------------------- host surface over a stand-in locator
def _stand_in(tok_dir):
    import box_checks as BX
    import region_checks as RC
    proc, _ = RC.oracle(tok_dir)
    return {"model": BX.StandInLocator(L), "processor": proc}


def test_locate_with_a_stand_in_locator(emu, tok_dir):
    """tile cut and box parse are the real op on the emulation, the decode between them is canned (BX.StandInLocator)"""
    import box_checks as BX
    import region_checks as RC
    from omniparser_amd.util import utils as U
    cmp_ = _stand_in(tok_dir)
    img = RC.frame(150, 100)
    kw = dict(max_new_tokens=64, overlap=16)
    boxes, stats = BX.check_locate(cmp_, img, kw)
    tiles = [(0, 0), (43, 0), (86, 0), (0, 36), (43, 36), (86, 36)]
    assert torch.equal(cmp_["model"].tiles[..., :3], RC.host_tiles(img, tiles * 2, 64).permute(0, 2, 3, 1))
    assert len(stats) == 12 and [s["found"] for s in stats[:6]] == [2, 1, 0, 1, 0, 1] and [s["fallback"] for s in stats[:6]] == [False, False, True, False, False, True]
    assert [s["query"] for s in stats] == ["AB"] * 6 + ["C D"] * 6 and [s["tile"] for s in stats] == list(range(6)) * 2
    assert boxes and {b["query"] for b in boxes} <= {"AB", "C D"} and any(b["label"] == "loc_500>B" for b in boxes)
    two = [b for b in boxes if b["tile"] == 0 and b["query"] == "AB"]       # row 0: one phrase, two boxes; which of them tile 0 owns: by centre
    assert all(b["label"] == "AB" and b["phrase"] == 0 for b in two)
    # the other tasks: phrase grounding with a banned phrase, the tasks without text, boxes only
    all_cpg = BX.check_locate(cmp_, img, kw, task=BX.CPG, text=["A B"])[0]
    banned = U.locate(img, cmp_, task=BX.CPG, text="A B", banned_phrases=("AB",), **kw)
    assert banned == [b for b in all_cpg if b["label"] != "AB"] and len(banned) < len(all_cpg)
    assert U.locate(img, cmp_, task=BX.OVD, text="A B", banned_phrases=("AB",), **kw) == BX.check_locate(cmp_, img, kw, text=["A B"])[0]
    for task in ("<OD>", "<DENSE_REGION_CAPTION>", "<REGION_PROPOSAL>"):
        got, st = BX.check_locate(cmp_, img, kw, task=task, text=None)
        assert len(st) == 6 and all(b["query"] is None for b in got)
        if task == "<REGION_PROPOSAL>":
            assert got and all(b["label"] == "" for b in got if not st[b["tile"]]["fallback"])
    # polygons: an <OPEN_VOCABULARY_DETECTION> row whose text holds <poly> yields no boxes and is counted
    cmp_["model"].poly = cmp_["processor"].tok.encode("poly>", add_special_tokens=False).ids
    got, st = U.locate(img, cmp_, text="AB", return_stats=True, **kw)
    assert [s["polygons"] for s in st] == [False] * 5 + [True] and st[5]["found"] == 0 and all(b["tile"] != 5 for b in got)
    got, st = U.locate(img, cmp_, task=BX.CPG, text="AB", return_stats=True, **kw)
    assert not any(s["polygons"] for s in st)


def test_ground_elements_with_a_stand_in_locator(emu, tok_dir):
    import region_checks as RC
    from omniparser_amd.util import utils as U
    cmp_ = _stand_in(tok_dir)
    img = RC.frame(150, 100)
    kw = dict(max_new_tokens=64, overlap=16)
    boxes = U.locate(img, cmp_, text=["AB", "C D"], **kw)
    first = boxes[0]["bbox"]
    x0, y0, x1, y1 = min(first[0], first[2]), min(first[1], first[3]), max(first[0], first[2]), max(first[1], first[3])
    elements = [{"type": "icon", "bbox": [0.9, 0.9, 0.95, 0.95], "content": "far"},
                {"type": "icon", "bbox": [x0 / 150, y0 / 100, x1 / 150, y1 / 100], "content": "the box itself"}]
    per = U.ground_elements(img, elements, cmp_, ["AB", "C D"], **kw)
    assert [[{k: v for k, v in b.items() if k not in ("element", "iou")} for b in p] for p in per] == [[b for b in boxes if b["query"] == q] for q in ("AB", "C D")]
    assert all(0.0 <= b["iou"] <= 1.0 and (b["element"] == -1) == (b["iou"] < 0.5) for p in per for b in p)
    hit = per[0][0]
    if x1 > x0 and y1 > y0:
        assert hit["element"] == 1 and hit["iou"] > 0.99
    assert all(b["element"] == -1 for p in U.ground_elements(img, elements[:1], cmp_, ["AB"], **kw) for b in p)
    assert all(b["element"] in (-1, 1) for p in U.ground_elements(img, elements, cmp_, "AB", min_iou=0.0, **kw) for b in p)
    for bad in (dict(min_iou=1.5), dict(min_iou="x"), dict(return_stats=True)):
        with pytest.raises(ValueError):
            U.ground_elements(img, elements, cmp_, ["AB"], **{**kw, **bad})


def test_describe_regions_with_a_stand_in_locator(emu, tok_dir):
    import box_checks as BX
    import region_checks as RC
    from omniparser_amd.util import utils as U
    cmp_ = _stand_in(tok_dir)
    model, proc = cmp_["model"], cmp_["processor"]
    img = RC.frame(150, 100)
    tiles = [(0, 0), (43, 0), (86, 0), (0, 36), (43, 36), (86, 36)]
    for task in U.TASKS_WITH_REGION:
        texts = U.describe_regions(img, [list(b) for b in BX.DESCRIBE_BOXES], cmp_, task=task, max_new_tokens=8, overlap=16)
        origins, prompts = BX.describe_rows(proc, tiles, 64, task=task)
        call = model.calls[-1]
        assert call["origins"] == origins == [tiles[t] for t in BX.DESCRIBE_TILES] and call["prompts"] == prompts and call["max_new_tokens"] == 8
        assert texts == ["AB", "C A", "B"]
        assert torch.equal(model.tiles[..., :3], RC.host_tiles(img, origins, 64).permute(0, 2, 3, 1))
    # a box that reaches beyond its tile is clipped to it; one exactly on a cell boundary goes to the cell that starts there
    U.describe_regions(img, [[50, 40, 57, 60]], cmp_, max_new_tokens=8, overlap=16)     # doubled centre (107, 100): tile 4, origin (43, 36)
    assert model.calls[-1]["origins"] == [(43, 36)] and model.calls[-1]["prompts"] == [proc.task_prompt_ids("<REGION_TO_DESCRIPTION>", region=[7, 4, 14, 24], size=(64, 64))]
    U.describe_regions(img, [[-20, -5, 149, 99]], cmp_, max_new_tokens=8, overlap=16)    # centre (129, 94) doubled: tile 1, origin (43, 0)
    assert model.calls[-1]["origins"] == [(43, 0)] and model.calls[-1]["prompts"] == [proc.task_prompt_ids("<REGION_TO_DESCRIPTION>", region=[0, 0, 64, 64], size=(64, 64))]
    n = len(model.calls)
    assert U.describe_regions(img, [], cmp_, overlap=16) == []
    for kw in (dict(task="<OD>"), dict(task="<REGION_TO_SEGMENTATION>"), dict(overlap=64), dict(overlap=True), dict(max_new_tokens=0)):
        with pytest.raises(ValueError):
            U.describe_regions(img, [[1, 2, 3, 4]], cmp_, **{"overlap": 16, **kw})
    for bad in ([[1, 2, 3]], [[5, 2, 3, 4]], [[1, 5, 3, 4]]):
        with pytest.raises(ValueError):
            U.describe_regions(img, bad, cmp_, overlap=16)
    assert len(model.calls) == n


def test_surface_validation_errors(emu, tok_dir, tmp_path):
    import region_checks as RC
    from omniparser_amd.util import utils as U
    cmp_ = _stand_in(tok_dir)
    img = RC.frame(70, 70)
    for kw in (dict(text=None), dict(text=[]), dict(text=""), dict(text=["a", 3]), dict(task="<OCR>", text="a"), dict(task="<OD>", text="a"),
               dict(task="<REGION_TO_OCR>", text="a"), dict(task="<REFERRING_EXPRESSION_SEGMENTATION>", text="a"), dict(text="a", overlap=64),
               dict(text="a", overlap=True), dict(text="a", max_new_tokens=0), dict(text="a", min_confidence=1.5), dict(text="a", min_confidence="x"),
               dict(text="A" * 200)):
        with pytest.raises(ValueError):
            U.locate(img, cmp_, **kw)
    with pytest.raises(ValueError, match="tokenizer.json"):
        U.locate(img, {"model": cmp_["model"], "processor": U.FlorenceProcessor(tmp_path / "nowhere")}, text="a")
    assert cmp_["model"].calls == []                        # nothing reached the locator


@pytest.fixture(scope="module")
def host_cap():
    """a captioner object without a device: the argument checks run before anything touches one"""
    from omniparser_amd.florence import Florence2Captioner, FlorenceWeights
    from tools.make_weights import ensure_caption_checkpoint
    cap = Florence2Captioner.__new__(Florence2Captioner)
    cap.w = FlorenceWeights(ensure_caption_checkpoint(0))
    cap.num_beams, cap.token_scores, cap.resolution, cap._plans = 1, False, 64, {}
    return cap


def test_bad_captioner_arguments_are_value_errors_before_any_device_work(host_cap, tok_dir):
    import region_checks as RC
    proc, _ = RC.oracle(tok_dir)
    table, _ = proc.loc_class_table()
    img = torch.zeros(70, 70, 3, dtype=torch.uint8)
    row = proc.task_prompt_ids("<OPEN_VOCABULARY_DETECTION>", text="AB")
    good = dict(prompts=[row], class_table=table, grammar=0, max_new_tokens=64, overlap=16)
    for kw in (dict(prompts=[]), dict(prompts=None), dict(prompts=[row, [0] * 65]), dict(prompts=[[0, 10 ** 6, 2]]), dict(prompts=[[]]),
               dict(grammar=2), dict(grammar=-1), dict(grammar=True), dict(grammar=None), dict(class_table=None),
               dict(class_table=np.zeros((0,), np.uint16)), dict(overlap=64), dict(overlap=-1), dict(overlap=True), dict(overlap=16.0),
               dict(max_new_tokens=0), dict(max_new_tokens=host_cap.max_new_limit() + 1), dict(max_new_tokens=True),
               dict(controls={"repetition_penalty": -1.0}), dict(controls={"no_such_control": 1})):
        with pytest.raises(ValueError):
            host_cap.locate_regions(img, **{**good, **kw})
    for bad in (torch.zeros(70, 70, 3), torch.zeros(70, 70, 4, dtype=torch.uint8), "frame"):
        with pytest.raises(ValueError, match="uint8"):
            host_cap.locate_regions(bad, **good)
    tiles = dict(origins=[(0, 0), (6, 6)], prompts=[row, row], max_new_tokens=8)
    for kw in (dict(prompts=[row]), dict(origins=[(0, 0)]), dict(prompts=[]), dict(origins=[], prompts=[]), dict(prompts=[row, [0] * 65]),
               dict(max_new_tokens=0), dict(controls={"no_such_control": 1}), dict(origins=[(0, 0), (2 ** 31, 0)])):
        with pytest.raises(ValueError):
            host_cap.decode_tiles(img, **{**tiles, **kw})
    with pytest.raises(ValueError, match="uint8"):
        host_cap.decode_tiles(torch.zeros(70, 70, 3), **tiles)
    assert host_cap._plans == {}


# ---------------------------------------------------------------------------------------------- thin wrappers
def test_locate_route_with_a_stub_service():
    import warnings
    from fastapi.testclient import TestClient
    from omniparser_amd import server as S
    from omniparser_amd.client import OmniParserClient

    class Parser:
        calls = []

        def locate(self, image_base64, phrases, **kw):
            self.calls.append((image_base64, phrases, kw))
            if not phrases and "task" not in kw:
                raise ValueError("task <OPEN_VOCABULARY_DETECTION> needs a phrase or a list of phrases")
            return [{"label": "save", "query": (phrases or [None])[0], "bbox": [1, 2, 30, 40], "confidence": 0.5, "tile": 0, "phrase": 0}]

    svc = S.ParseService(Parser(), screen_parser=object(), workers=1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        tc = TestClient(S.build_app({}, service=svc))
    r = tc.post("/locate/", json={"base64_image": "aGk=", "phrases": ["the Save button"]})
    assert r.status_code == 200 and set(r.json()) == {"boxes", "latency"} and r.json()["boxes"][0]["bbox"] == [1, 2, 30, 40]
    assert Parser.calls[-1] == ("aGk=", ["the Save button"], {})
    r = tc.post("/locate/", json={"base64_image": "aGk=", "task": "<OD>"})
    assert r.status_code == 200 and Parser.calls[-1] == ("aGk=", None, {"task": "<OD>"})
    assert tc.post("/locate/", json={"base64_image": "aGk=", "phrases": []}).status_code == 422       # the ValueError
    assert tc.post("/locate/", json={"phrases": ["x"]}).status_code == 422
    assert tc.get("/probe/").json() == {"message": "Omniparser API ready"}
    # the client talks to it
    client = OmniParserClient("http://host/parse/", post=lambda url, json: tc.post(url.replace("http://host", ""), json=json))
    assert client.locate(b"hi", ["the Save button"])[0]["label"] == "save" and Parser.calls[-1][1] == ["the Save button"]
    assert client.locate(b"hi", None, task="<OD>")[0]["query"] is None
    with pytest.raises(RuntimeError, match="422"):
        client.locate(b"hi", [])


def test_facade_and_screen_parser_pass_through(monkeypatch, emu, tok_dir):
    import base64
    import io
    import box_checks as BX
    import region_checks as RC
    from PIL import Image
    from omniparser_amd.pipeline import ScreenParser
    from omniparser_amd.util import omniparser as F
    from omniparser_amd.util import utils as U
    cmp_ = _stand_in(tok_dir)
    monkeypatch.setattr(U, "get_yolo_model", lambda model_path, device: object())
    monkeypatch.setattr(U, "get_caption_model_processor", lambda model_name, model_name_or_path, device: cmp_)
    op = F.Omniparser({"som_model_path": "x", "caption_model_name": "florence2", "caption_model_path": "y", "BOX_TRESHOLD": 0.05})
    img = RC.frame(150, 100)
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format="PNG")
    kw = dict(max_new_tokens=64, overlap=16)
    want = U.locate(img, cmp_, text=["AB"], **kw)
    assert op.locate(base64.b64encode(buf.getvalue()).decode("ascii"), ["AB"], **kw) == want and want
    sp = ScreenParser.__new__(ScreenParser)
    sp.cap, sp.proc = cmp_["model"], cmp_["processor"]
    assert sp.locate(torch.from_numpy(img), ["AB"], **kw) == want
    assert sp.locate(torch.from_numpy(img), None, task="<REGION_PROPOSAL>", **kw) == U.locate(img, cmp_, task="<REGION_PROPOSAL>", **kw)
    assert BX.OVD == "<OPEN_VOCABULARY_DETECTION>"

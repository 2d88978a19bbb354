"""Segmentation on the host emulation of the HIP kernels (tests/emu) and on the host alone: OMNI_OP_REGION_OCR mode 5 case by case —
bit-equal to a literal host restatement and equal to transformers' "polygons" parse — mode 6 bit-equal to its twin, with written-down
rectangles and Pillow beside it, the ownership rule, the argument checks, the old refusals, and the host surface
(poly_class_table, segment_prompt_ids, parse_polygon_answer, raster_polygons, segment, segment_elements, the /segment/ route) over a
stand-in for the encode and the decode.  Helpers: tests/poly_checks.py; the MI355X twin: tests/test_gpu_y_region_polys.py."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from omniparser_amd import _lib as L

CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def tok_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("region_polys")


# ---------------------------------------------------------------------------------------------- mode 5, one launch per case
@pytest.mark.parametrize("n", [1, 3, 17])
@pytest.mark.parametrize("T", [3, 5, 6, 9, 65, 1025])
def test_polygons_are_the_twin_and_transformers(emu, tok_dir, T, n):
    import poly_checks as PC
    PC.check_polys(L, CPU, tok_dir, T, n)


def test_polygons_without_log_probabilities(emu, tok_dir):
    import poly_checks as PC
    PC.check_polys(L, CPU, tok_dir, 65, 19, with_logp=False)


def test_polygons_at_the_other_resolution(emu, tok_dir):
    import poly_checks as PC
    names = PC.check_polys(L, CPU, tok_dir, 65, 19, R=768)
    assert set(names) == set(PC.gen_cases(65))              # 19 rows: every listed case once


@pytest.mark.parametrize("text_share", [0.02, 0.05, 0.1])
def test_random_rows_are_the_twin_and_transformers(emu, tok_dir, text_share):
    import poly_checks as PC
    assert PC.check_random(L, CPU, tok_dir, text_share) > 100


def test_the_listed_rows_give_what_the_list_says(emu, tok_dir):
    import poly_checks as PC
    PC.check_expected(L, CPU, tok_dir)


def test_instance_ownership_on_a_3x2_grid_and_exactly_on_the_boundaries(emu, tok_dir):
    import poly_checks as PC
    PC.check_ownership(L, CPU, tok_dir)


def test_polygon_and_mask_argument_errors(emu, tok_dir):
    import poly_checks as PC
    seen = PC.check_errors(L, CPU, tok_dir)
    assert all("region_ocr" in msg for _, msg in seen), seen
    msgs = dict(seen)
    assert "T / 2" in msgs["mode 3's M"] and "(T - 1) / 2" in msgs["V too small"] and "mode 2" in msgs["mode 2"] and "mode 4" in msgs["mode 4"]
    assert "1..64" in msgs["I = 0"] and "1..64" in msgs["I = 65"] and "p3" in msgs["null vertices"]


# ---------------------------------------------------------------------------------------------- mode 6
@pytest.mark.parametrize("frame", [(30, 20), (64, 64), (150, 100)])
@pytest.mark.parametrize("I", [1, 4])
@pytest.mark.parametrize("R", [32, 40, 64])
def test_masks_are_the_twin(emu, R, I, frame):
    import poly_checks as PC
    assert PC.check_masks(L, CPU, R, I, frame) > 0


def test_masks_of_rectangles_frame_edges_and_a_1024_vertex_polygon(emu):
    import poly_checks as PC
    PC.check_masks_known(L, CPU)


def test_masks_of_one_row_at_768(emu):
    import poly_checks as PC
    PC.check_masks_768(L, CPU)


def test_masks_agree_with_pillow_away_from_the_edges(emu):
    import poly_checks as PC
    assert PC.check_masks_pillow(L, CPU) < 0.25


# ---------------------------------------------------------------------------------------------- the old refusals and the three files
def test_modes_1_and_3_and_their_refusals_behave_as_before(emu, tok_dir):
    import box_checks as BX
    import region_checks as RC
    RC.check_parse(L, CPU, tok_dir, 19, 3)
    assert "region_ocr" in dict(RC.check_parse_errors(L, CPU, tok_dir))["mode 2"]
    seen = dict(BX.check_errors(L, CPU, tok_dir))
    assert "mode 2" in seen["mode 2"] and "mode 4" in seen["mode 4"]
    # the three polygon classes are HARD to modes 1 and 3: a table that holds them parses as one that says HARD
    import poly_checks as PC
    _proc, _post, table, _texts = PC.class_table(tok_dir)
    ids = np.full((1, 19), RC.PAD, np.int32)
    row = [RC.START, RC.A, PC.SEP] + BX.BOX_A + [RC.EOS]
    ids[0, :len(row)] = row
    cells = [[0, 0, -2 ** 31, RC.INF, -2 ** 31, RC.INF]]
    hard = table.copy()
    hard[[PC.SEP, PC.POLY, PC.PEND]] = RC.HARD
    for grammar in (0, 1):
        a = BX.launch_boxes(L, CPU, lambda: None, ids, table, None, cells, 19, 64, grammar)
        b = BX.launch_boxes(L, CPU, lambda: None, ids, hard, None, cells, 19, 64, grammar)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)) and a[2][0, 2] & 1


def test_header_python_and_profiler_agree_on_modes_5_and_6():
    from omniparser_amd import florence as FL
    from omniparser_amd import opwork
    hdr = (Path(__file__).resolve().parents[1] / "include" / "omni_amd.h").read_text()
    doc = re.search(r"/\* REGION OCR.*?\*/\s*OMNI_OP_REGION_OCR = ", hdr, re.S).group(0)
    for word in ("i0 = 5", "region_polys_kernel", "exactly T / 2", "exactly (T - 1) / 2", "i0 = 6", "poly_mask_kernel", "instances kept",
                 "i0 = 2 and i0 = 4 stay refused", "OMNI_OCR_CLASS_POLY_END", "even-odd"):
        assert word in doc, word
    for name, val in (("SEP", L.OCR_CLASS_SEP), ("POLY", L.OCR_CLASS_POLY), ("POLY_END", L.OCR_CLASS_POLY_END)):
        assert f"#define OMNI_OCR_CLASS_{name} {val}\n" in hdr
    assert (L.OCR_CLASS_SEP, L.OCR_CLASS_POLY, L.OCR_CLASS_POLY_END) == (1003, 1004, 1005) and (L.OCR_MODE_POLYS, L.OCR_MODE_MASKS) == (5, 6)
    assert [FL.poly_slots(t) for t in (3, 5, 6, 65, 1025, 2049)] == [(1, 1), (2, 2), (3, 2), (32, 32), (512, 512), (1024, 1024)]
    op = FL.poly_parse_op(1, 2, 3, 4, 5, 6, 7, 8, 6, 1025, 51289, 768, 2)
    assert op.kind == L.OP_REGION_OCR and op.i[0] == 5 and op.i[3] == 512 and op.i[9] == 512
    assert opwork.op_kernel(op) == "region_ocr (polygons)" and opwork.op_shape(op) == (6, 1025, 0)
    assert opwork.op_work(op) == (0, 6 * (4 * 1025 + 4 * 1024 + 68 * 512 + 8 * 512 + 40))
    op.p[2] = None
    assert opwork.op_work(op) == (0, 6 * (4 * 1025 + 68 * 512 + 8 * 512 + 40))
    mk = FL.poly_mask_op(1, 2, 3, 4, 5, 6, 6, 1025, 4, 1080, 1920, 768)
    assert mk.i[0] == 6 and (mk.i[3], mk.i[4], mk.i[5], mk.i[7]) == (4, 1080, 1920, 768)
    assert opwork.op_kernel(mk) == "region_ocr (masks)" and opwork.op_shape(mk) == (6, 768, 4)
    assert opwork.op_work(mk) == (0, 6 * (64 * 512 + 8 * 512 + 40 + 4 * 768 * (4 * 24 + 4)))


# ---------------------------------------------------------------------------------------------- host side, no device
def test_poly_class_table_needs_the_three_tokens(tok_dir):
    import poly_checks as PC
    import region_checks as RC
    from omniparser_amd.util import utils as U
    PC.class_table(tok_dir)
    d = RC.write_tokenizer(Path(tok_dir) / "tok_without_poly")
    proc = U.FlorenceProcessor(d, image_token_id=1400, special_ids=(RC.BOS, RC.PAD, RC.EOS, 3))
    before = proc.loc_class_table()[0].copy()
    with pytest.raises(ValueError, match=r"tokenizer\.json.*<sep>"):
        proc.poly_class_table()
    assert np.array_equal(proc.loc_class_table()[0], before) and len(before) == 1400


def test_segment_prompt_ids_are_the_tokenizer_on_transformers_sentences(tok_dir):
    import warnings
    import poly_checks as PC
    import region_checks as RC
    from transformers import CLIPImageProcessor, PreTrainedTokenizerFast
    from transformers.models.florence2.processing_florence2 import Florence2Processor
    proc, _post = PC.oracle(tok_dir)
    tok = PreTrainedTokenizerFast(tokenizer_file=str(Path(tok_dir) / "tok_poly" / "tokenizer.json"), bos_token="<s>", eos_token="</s>", pad_token="<pad>",
                                  unk_token="<unk>")
    tok.image_token, tok.image_token_id = "<image>", PC.IMAGE_TOKEN
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ip = CLIPImageProcessor()
    ip.image_seq_length = 5
    hf = Florence2Processor(ip, tok)
    RES, R2S = "<REFERRING_EXPRESSION_SEGMENTATION>", "<REGION_TO_SEGMENTATION>"
    for text in ("the AB button", "  A B and CD  "):
        sentence = hf._construct_prompts([RES + text])[0]
        assert RES not in sentence and text.strip() in sentence and sentence.endswith("with mask")
        want = tok(tok.bos_token + sentence + tok.eos_token, add_special_tokens=False)["input_ids"]
        assert proc.segment_prompt_ids(RES, text=text) == want and want[0] == RC.BOS and want[-1] == RC.EOS
    for region, size in (([8, 16, 24.5, 63], (64, 64)), ([0, 0, 768, 768], (768, 768)), ([100, 7, 300, 500], (768, 512))):
        bins = hf.post_processor.quantize(torch.tensor([region], dtype=torch.float32), size)[0].tolist()
        sentence = hf._construct_prompts([R2S + "".join(f"<loc_{b}>" for b in bins)])[0]
        want = tok(tok.bos_token + sentence + tok.eos_token, add_special_tokens=False)["input_ids"]
        got = proc.segment_prompt_ids(R2S, region=region, size=size)
        assert got == want and sum(1 for t in got if RC.LOC0 <= t < RC.LOC0 + 1000) == 4, region
    good = dict(region=[1, 2, 3, 4], size=(64, 64))
    for task, kw in ((RES, {}), (RES, good), (RES, dict(text=3)), (R2S, dict(text="a")), (R2S, dict(region=[1, 2, 3, 4])), (R2S, dict(region=[1, 2, 3], size=(64, 64))),
                     ("<OPEN_VOCABULARY_DETECTION>", dict(text="a")), ("<OD>", {})):
        with pytest.raises(ValueError):
            proc.segment_prompt_ids(task, **kw)
    from omniparser_amd.util import utils as U
    with pytest.raises(ValueError, match="tokenizer.json"):
        U.FlorenceProcessor(None).segment_prompt_ids(RES, text="a")
    # the old entry points keep refusing the two tasks
    for task, kw in ((RES, dict(text="a")), (R2S, good)):
        with pytest.raises(ValueError):
            proc.task_prompt_ids(task, **kw)
        with pytest.raises(ValueError, match="needs an input"):
            proc.prompt_ids(task + " a")


def test_parse_polygon_answer_is_transformers_on_hard_rows(tok_dir):
    import poly_checks as PC
    import region_checks as RC
    from omniparser_amd.util import utils as U
    proc, post = PC.oracle(tok_dir)
    enc = lambda s: proc.tok.encode(s, add_special_tokens=False).ids       # noqa: E731
    A, B, NL, LT, S, P, E = RC.A, RC.B, RC.TOK_NL, RC.TOK_LT, PC.SEP, PC.POLY, PC.PEND
    rows = [[A, NL] + PC.L6, PC.L6 + [NL] + PC.L4 + [S] + PC.L2, [A, LT] + PC.L6 + [S] + PC.L7, [P] + PC.L6 + [NL] + PC.L4 + [E],
            enc("A<od>B") + [P] + PC.L6 + [E, P] + PC.L7 + [E], [LT] + PC.L3 + [S, S, S], [P] + PC.L6 + [P] + PC.L4 + [E, NL, E] + PC.L4 + [P],
            enc("<sep") + PC.L6 + [S] + PC.L3 + [RC.PAD] + PC.L3, PC.L3 + [LT] + PC.L3, [RC.SP, A] + PC.L2 + [P] + PC.L6 + [E, S, S]]
    some = 0
    for g in rows:
        row = [RC.START, RC.BOS] + g + [RC.EOS] + PC.L6 + [A]
        got = U.parse_polygon_answer(row, proc, (64, 48))
        end = row.index(RC.EOS, 1)
        text, _ = post.decode_with_spans(row[1:end])
        want = post.parse_description_with_polygons_from_text_and_spans(text, (64, 48), allow_empty_phrase=True)
        assert [x["polygons"] for x in got] == [[torch.tensor(p, dtype=torch.float32).int().tolist() for p in w["polygons"]] for w in want], (g, got, want)
        for x in got:                                       # the columns are the location tokens that made the vertices, in order
            flat = [v for p in x["polygons"] for v in p]
            assert len(x["columns"]) == len(flat) and all(RC.LOC0 <= row[j] < RC.LOC0 + 1000 for j in x["columns"]) and x["columns"] == sorted(x["columns"])
            assert flat == [U.dequantize_bin(row[j] - RC.LOC0, 48 if q & 1 else 64) for q, j in enumerate(x["columns"])]
        some += len(got)
    assert some >= 8


def test_raster_polygons_is_the_mask_rule():
    import poly_checks as PC
    from omniparser_amd.util import utils as U
    flat = lambda p: [v for xy in p for v in xy]                                                                     # noqa: E731
    for name, poly in list(PC.SIMPLE.items()) + [("bowtie", PC.BOWTIE)]:
        assert np.array_equal(U.raster_polygons([flat(poly)], (0, 0), (72, 72)), PC.inside_polygon(poly, 72)), name
    both = U.raster_polygons([flat(PC.RECT), flat(PC.TRI), [1, 1, 9, 9], []], (0, 0), (72, 72))
    assert np.array_equal(both, PC.inside_polygon(PC.RECT, 72) | PC.inside_polygon(PC.TRI, 72))
    moved = U.raster_polygons([flat([(x + 100, y + 50) for x, y in PC.RECT])], (103, 52), (30, 20), frame=(120, 60))
    want = PC.inside_polygon(PC.RECT, 72)[2:22, 3:33].copy()
    want[8:, :] = False                                     # frame rows 60.. lie outside
    want[:, 17:] = False                                    # frame columns 120.. lie outside
    assert np.array_equal(moved, want) and want.any()
    rect = U.raster_polygons([[5, 4, 40, 4, 40, 30, 5, 30]], (0, 0), (50, 40))
    assert rect.sum() == 35 * 26 and rect[4:30, 5:40].all()


# ---------------------------------------------------------------------------------------------- host surface over a stand-in segmenter
def _stand_in(tok_dir):
    import poly_checks as PC
    proc, _ = PC.oracle(tok_dir)
    return {"model": PC.StandInSegmenter(L), "processor": proc}


def test_segment_phrases_with_a_stand_in_segmenter(emu, tok_dir):
    """tile cut, polygon parse and mask raster are the real op on the emulation, the decode between them is canned"""
    import poly_checks as PC
    import region_checks as RC
    cmp_ = _stand_in(tok_dir)
    proc = cmp_["processor"]
    img = RC.frame(150, 100)
    kw = dict(max_new_tokens=64, overlap=16)
    got, stats = PC.check_segment(cmp_, img, kw, text=["AB", "C D"])
    tiles = [(0, 0), (43, 0), (86, 0), (0, 36), (43, 36), (86, 36)]
    call = cmp_["model"].calls[-1]
    assert call["origins"] == tiles * 2 and call["prompts"] == [proc.segment_prompt_ids(PC.RES, text="AB")] * 6 + [proc.segment_prompt_ids(PC.RES, text="C D")] * 6
    assert torch.equal(cmp_["model"].tiles[..., :3], RC.host_tiles(img, tiles * 2, 64).permute(0, 2, 3, 1))
    assert [s["index"] for s in stats] == [0] * 6 + [1] * 6 and [s["tile"] for s in stats] == list(range(6)) * 2
    assert [s["found"] for s in stats[:5]] == [2, 1, 1, 0, 5] and [s["fallback"] for s in stats[:5]] == [False, False, True, False, False]
    assert got and {g["query"] for g in got} <= {"AB", "C D"} and all("region" not in g for g in got)
    assert any(g["area"] > 100 and g["point"] is not None for g in got)
    # degenerate instances (tile 5: one vertex; the second phrase's tile 0: vertices on one line) come back with empty masks
    lone = [g for g in got if g["index"] == 0 and g["tile"] == 5]
    assert len(lone) == 1 and lone[0]["polygons"][0] == [] and len(lone[0]["polygons"][1]) == 2 and lone[0]["mask"].shape == (0, 0)
    assert (lone[0]["area"], lone[0]["point"]) == (0, None) and lone[0]["bbox"][0] == lone[0]["bbox"][2]
    flat = [g for g in got if g["index"] == 1 and g["tile"] == 0]
    assert len(flat) == 1 and [len(p) for p in flat[0]["polygons"]] == [6, 6] and flat[0]["area"] == 0 and flat[0]["point"] is None and flat[0]["mask"].size > 0
    from omniparser_amd.util import utils as U
    one_line = PC.StandInSegmenter(L)
    one_line.canned_polys = lambda k, T: ([PC.START] + PC.loc(100, 500, 300, 500, 600, 500) + [PC.EOS] + [PC.PAD] * T)[:T]
    only = U.segment(img, {"model": one_line, "processor": proc}, text="AB", **kw)
    assert only and all(g["mask"].shape[0] == 0 and g["mask"].shape[1] > 0 and g["area"] == 0 and g["point"] is None for g in only)
    one = PC.check_segment(cmp_, img, dict(kw, instances=1), text="AB")[0]      # everything behind the first instance of a row: host raster
    assert [(g["index"], g["polygons"], g["area"], g["point"]) for g in one] == [(g["index"], g["polygons"], g["area"], g["point"]) for g in got if g["index"] == 0]


def test_segment_regions_and_elements_with_a_stand_in_segmenter(emu, tok_dir):
    import box_checks as BX
    import poly_checks as PC
    import region_checks as RC
    from omniparser_amd.util import utils as U
    cmp_ = _stand_in(tok_dir)
    model, proc = cmp_["model"], cmp_["processor"]
    img = RC.frame(150, 100)
    kw = dict(max_new_tokens=64, overlap=16)
    tiles = [(0, 0), (43, 0), (86, 0), (0, 36), (43, 36), (86, 36)]
    boxes = [list(b) for b in BX.DESCRIBE_BOXES]
    got, stats = PC.check_segment(cmp_, img, kw, regions=boxes)
    call = model.calls[-1]
    origins = [tiles[t] for t in BX.DESCRIBE_TILES]
    assert call["origins"] == origins and [s["tile"] for s in stats] == list(BX.DESCRIBE_TILES) and [s["index"] for s in stats] == [0, 1, 2]
    for b, (ox, oy), row in zip(boxes, origins, call["prompts"]):           # clipped and quantised as describe_regions does
        clip = lambda v: min(max(v, 0), 64)                                  # noqa: E731
        assert row == proc.segment_prompt_ids(PC.R2S, region=[clip(b[0] - ox), clip(b[1] - oy), clip(b[2] - ox), clip(b[3] - oy)], size=(64, 64))
    assert all(g["region"] == [float(v) for v in boxes[g["index"]]] and "query" not in g for g in got)
    U.segment(img, cmp_, regions=[[50, 40, 57, 60]], **kw)                  # doubled centre (107, 100): tile 4, origin (43, 36)
    assert model.calls[-1]["origins"] == [(43, 36)] and model.calls[-1]["prompts"] == [proc.segment_prompt_ids(PC.R2S, region=[7, 4, 14, 24], size=(64, 64))]
    elements = [{"type": "icon", "bbox": [b[0] / 150, b[1] / 100, b[2] / 150, b[3] / 100], "content": str(k)} for k, b in enumerate(boxes)]
    per = U.segment_elements(img, elements, cmp_, **kw)
    assert len(per) == 3
    for k, g in enumerate(per):
        mine = [x for x in got if x["index"] == k]
        assert (g is None) == (not mine)
        if g is not None:
            assert g["confidence"] == max(x["confidence"] for x in mine) and g["index"] == k
    assert any(g is not None for g in per)
    assert U.segment(img, cmp_, regions=[], **kw) == []
    # what a box gives does not depend on the other boxes of the call: [5, 5, 40, 30] lands on tile 0 and is answered with a shape
    # at tile pixels x 54..62, right of x = 53.5 — the boundary tiles 0 and 1 ALONE would draw once [60, 5, 80, 30] joins the call
    right = PC.StandInSegmenter(L)
    right.canned_polys = lambda k, T: ([PC.START] + PC.loc(850, 200, 980, 200, 980, 700, 850, 700) + [PC.EOS] + [PC.PAD] * T)[:T]
    cmp_r = {"model": right, "processor": proc}
    strip = lambda gs, i: [{k: (v.tolist() if k == "mask" else v) for k, v in g.items() if k not in ("index", "confidence")}   # noqa: E731
                            for g in gs if g["index"] == i]         # (the stand-in's log-probabilities depend on the number of rows)
    alone = U.segment(img, cmp_r, regions=[[5, 5, 40, 30]], **kw)
    assert right.calls[-1]["origins"] == [(0, 0)] and len(alone) == 1 and alone[0]["bbox"] == [54, 12, 62, 44] and alone[0]["area"] == 8 * 32
    both = U.segment(img, cmp_r, regions=[[5, 5, 40, 30], [60, 5, 80, 30]], **kw)
    assert right.calls[-1]["origins"] == [(0, 0), (43, 0)] and strip(both, 0) == strip(alone, 0) and len(strip(both, 1)) == 1
    swapped = U.segment(img, cmp_r, regions=[[60, 5, 80, 30], [60, 70, 90, 95], [5, 5, 40, 30]], **kw)
    assert strip(swapped, 2) == strip(alone, 0) and [g["index"] for g in swapped] == [0, 1, 2]
    per_r = U.segment_elements(img, [elements[0], {"type": "icon", "bbox": [0.4, 0.05, 0.53, 0.3], "content": "b"}], cmp_r, **kw)
    assert per_r[0] is not None and strip([per_r[0]], 0) == strip(alone, 0)


def test_segment_validation_errors_reach_nothing(emu, tok_dir, tmp_path):
    import region_checks as RC
    from omniparser_amd.util import utils as U
    cmp_ = _stand_in(tok_dir)
    img = RC.frame(70, 70)
    for kw in (dict(), dict(text="a", regions=[[1, 2, 3, 4]]), dict(text=[]), dict(text=""), dict(text=["a", 3]), dict(regions=[[1, 2, 3]]),
               dict(regions=[[5, 2, 3, 4]]), dict(regions=[[1, 5, 3, 4]]), dict(text="a", overlap=64), dict(text="a", overlap=True),
               dict(text="a", max_new_tokens=0), dict(text="a", min_confidence=1.5), dict(text="a", min_confidence="x"), dict(text="a", instances=0),
               dict(text="a", instances=65), dict(text="a", instances=True), dict(text="A" * 200)):
        with pytest.raises(ValueError):
            U.segment(img, cmp_, **{"overlap": 16, **kw})
    with pytest.raises(ValueError, match="tokenizer.json"):
        U.segment(img, {"model": cmp_["model"], "processor": U.FlorenceProcessor(tmp_path / "nowhere")}, text="a", overlap=16)
    no_poly = U.FlorenceProcessor(RC.write_tokenizer(tmp_path / "tok_plain"), image_token_id=1400, special_ids=(RC.BOS, RC.PAD, RC.EOS, 3))
    with pytest.raises(ValueError, match="<sep>"):
        U.segment(img, {"model": cmp_["model"], "processor": no_poly}, text="a", overlap=16)
    assert cmp_["model"].calls == []                        # nothing reached the segmenter
    # the old entry points keep refusing the two tasks
    for task in ("<REFERRING_EXPRESSION_SEGMENTATION>", "<REGION_TO_SEGMENTATION>"):
        with pytest.raises(ValueError):
            U.locate(img, cmp_, task=task, text="a", overlap=16)
        with pytest.raises(ValueError):
            U.describe_regions(img, [[1, 2, 3, 4]], cmp_, task=task, overlap=16)


def test_bad_segment_regions_arguments_are_value_errors_before_any_device_work(tok_dir):
    import poly_checks as PC
    from omniparser_amd.florence import Florence2Captioner, FlorenceWeights
    from tools.make_weights import ensure_caption_checkpoint
    cap = Florence2Captioner.__new__(Florence2Captioner)
    cap.w = FlorenceWeights(ensure_caption_checkpoint(0))
    cap.num_beams, cap.token_scores, cap.resolution, cap._plans = 1, False, 64, {}
    proc, _ = PC.oracle(tok_dir)
    table, _ = proc.poly_class_table()
    img = torch.zeros(70, 70, 3, dtype=torch.uint8)
    row = proc.segment_prompt_ids(PC.RES, text="AB")
    good = dict(origins=[(0, 0), (6, 6)], prompts=[row, row], class_table=table, max_new_tokens=8)
    for kw in (dict(prompts=[row]), dict(origins=[(0, 0)]), dict(prompts=[]), dict(origins=[], prompts=[]), dict(prompts=[row, [0] * 65]),
               dict(max_new_tokens=0), dict(max_new_tokens=1), dict(controls={"no_such_control": 1}), dict(origins=[(0, 0), (2 ** 31, 0)]),
               dict(class_table=None), dict(class_table=np.zeros((0,), np.uint16)), dict(instances=0), dict(instances=65), dict(instances=True),
               dict(instances=4.0), dict(cells=[[0, 0, 0, 9, 0, 9]]), dict(cells=[[1, 0, 0, 9, 0, 9], [6, 6, 0, 9, 0, 9]]),
               dict(cells=[[0, 0, 0, 9, 0], [6, 6, 0, 9, 0, 9]]), dict(cells=[[0, 0, 0, 2 ** 31, 0, 9], [6, 6, 0, 9, 0, 9]])):
        with pytest.raises(ValueError):
            cap.segment_regions(img, **{**good, **kw})
    with pytest.raises(ValueError, match="uint8"):
        cap.segment_regions(torch.zeros(70, 70, 3), **good)
    assert cap._plans == {}


# ---------------------------------------------------------------------------------------------- thin wrappers
def test_segment_route_with_a_stub_service():
    import warnings
    from fastapi.testclient import TestClient
    from omniparser_amd import server as S
    from omniparser_amd.client import OmniParserClient

    class Parser:
        calls = []

        def segment(self, image_base64, phrases=None, regions=None, **kw):
            self.calls.append((image_base64, phrases, regions, kw))
            if (phrases is None) == (regions is None):
                raise ValueError("segment takes exactly one of text and regions")
            return [{"query": phrases[0], "index": 0, "polygons": [[1, 2, 30, 2, 30, 40]], "bbox": [1, 2, 30, 40], "area": 500, "confidence": 0.5, "tile": 0,
                     "point": [20, 15], "mask": None, "mask_origin": (1, 2)}] if phrases else \
                   [{"region": regions[0], "index": 0, "polygons": [], "bbox": [0, 0, 0, 0], "area": 0, "confidence": 0.25, "tile": 1, "point": None,
                     "mask": None, "mask_origin": (0, 0)}]

    svc = S.ParseService(Parser(), screen_parser=object(), workers=1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        tc = TestClient(S.build_app({}, service=svc))
    r = tc.post("/segment/", json={"base64_image": "aGk=", "phrases": ["the Save button"]})
    assert r.status_code == 200 and set(r.json()) == {"segments", "latency"}
    seg = r.json()["segments"][0]
    assert seg["polygons"] == [[1, 2, 30, 2, 30, 40]] and seg["point"] == [20, 15] and seg["area"] == 500 and "mask" not in seg and "mask_origin" not in seg
    assert Parser.calls[-1] == ("aGk=", ["the Save button"], None, {"return_masks": False})
    r = tc.post("/segment/", json={"base64_image": "aGk=", "regions": [[1, 2, 3, 4]]})
    assert r.status_code == 200 and r.json()["segments"][0]["region"] == [1, 2, 3, 4] and Parser.calls[-1][1:3] == (None, [[1.0, 2.0, 3.0, 4.0]])
    assert tc.post("/segment/", json={"base64_image": "aGk="}).status_code == 422                          # the ValueError
    assert tc.post("/segment/", json={"base64_image": "aGk=", "phrases": ["a"], "regions": [[1, 2, 3, 4]]}).status_code == 422
    assert tc.post("/segment/", json={"phrases": ["x"]}).status_code == 422
    client = OmniParserClient("http://host/parse/", post=lambda url, json: tc.post(url.replace("http://host", ""), json=json))
    assert client.segment(b"hi", ["the Save button"])[0]["bbox"] == [1, 2, 30, 40]
    assert client.segment(b"hi", regions=[[1, 2, 3, 4]])[0]["tile"] == 1
    with pytest.raises(RuntimeError, match="422"):
        client.segment(b"hi")


def test_facade_and_screen_parser_pass_segment_through(monkeypatch, emu, tok_dir):
    import base64
    import io
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
    kw = dict(max_new_tokens=64, overlap=16, return_masks=False)
    want = U.segment(img, cmp_, text=["AB"], **kw)
    assert op.segment(base64.b64encode(buf.getvalue()).decode("ascii"), ["AB"], **kw) == want and want
    sp = ScreenParser.__new__(ScreenParser)
    sp.cap, sp.proc = cmp_["model"], cmp_["processor"]
    assert sp.segment(torch.from_numpy(img), ["AB"], **kw) == want
    assert sp.segment(torch.from_numpy(img), regions=[[5, 5, 40, 30]], **kw) == U.segment(img, cmp_, regions=[[5, 5, 40, 30]], **kw)

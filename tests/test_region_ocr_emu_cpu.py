"""Region OCR on the host emulation of the HIP kernels (tests/emu) and on the host alone: OMNI_OP_REGION_OCR case by case — mode 1
bit-equal to a literal host restatement and equal to transformers' Florence2PostProcessor, mode 0 bit-equal to the image processor on
Pillow crops — the ownership rule, the argument checks, the host surface (loc_class_table, parse_ocr_regions, read_text_regions,
FlorenceOCR, Omniparser's "florence" provider) over a stand-in for the encode.  Helpers: tests/region_checks.py; the MI355X twin with
the real captioner: tests/test_gpu_x_region_ocr.py."""
import re
from pathlib import Path

import pytest
import torch

from omniparser_amd import _lib as L

CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def tok_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("region_ocr")


# ---------------------------------------------------------------------------------------------- kernel, one launch per case
@pytest.mark.parametrize("n", [1, 3, 17])
@pytest.mark.parametrize("T", [10, 19, 65, 1025])
def test_parse_is_the_twin_and_transformers(emu, tok_dir, T, n):
    import region_checks as RC
    RC.check_parse(L, CPU, tok_dir, T, n)


def test_parse_without_log_probabilities(emu, tok_dir):
    import region_checks as RC
    RC.check_parse(L, CPU, tok_dir, 65, 17, with_logp=False)


def test_parse_at_the_other_resolution(emu, tok_dir):
    import region_checks as RC
    RC.check_parse(L, CPU, tok_dir, 65, 17, R=768)


def test_the_listed_rows_give_what_the_list_says(emu, tok_dir):
    import region_checks as RC
    RC.check_expected_counts(L, CPU, tok_dir)


def test_ownership_on_a_3x2_grid_and_exactly_on_the_boundaries(emu, tok_dir):
    import region_checks as RC
    RC.check_ownership(L, CPU, tok_dir)


def test_parse_argument_errors(emu, tok_dir):
    import region_checks as RC
    seen = RC.check_parse_errors(L, CPU, tok_dir)
    assert all("region_ocr" in msg for _, msg in seen), seen


@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("name", ["six_tiles", "one_tile", "narrower_than_a_tile"])
def test_tile_cut_is_the_processor_on_pillow_crops(emu, name, f16):
    import region_checks as RC
    RC.check_cut(L, CPU, name, f16)


def test_tile_cut_argument_errors(emu):
    import region_checks as RC
    seen = RC.check_cut_errors(L, CPU)
    assert all("region_ocr" in msg for _, msg in seen), seen


# ---------------------------------------------------------------------------------------------- host side, no device
@pytest.mark.parametrize("R", [64, 100, 768])
def test_integer_dequantisation_is_transformers(R):
    import region_checks as RC
    RC.check_dequantize(R)


def test_class_table_needs_florence_location_tokens(tmp_path):
    import region_checks as RC
    from omniparser_amd.util import utils as U
    with pytest.raises(ValueError, match="tokenizer.json"):
        U.FlorenceProcessor(None).loc_class_table()
    with pytest.raises(ValueError, match=re.escape(str(tmp_path / "none" / "tokenizer.json"))):
        U.FlorenceProcessor(tmp_path / "none").loc_class_table()
    plain = tmp_path / "plain"
    plain.mkdir()
    (plain / "tokenizer.json").write_text(RC.GOLDEN_TOK.read_text())
    for d in (plain, RC.write_tokenizer(tmp_path / "short", n_loc=999), RC.write_tokenizer(tmp_path / "swapped", shuffle=True)):
        with pytest.raises(ValueError, match="contiguous"):
            U.FlorenceProcessor(d, image_token_id=1400).loc_class_table()
    table, texts = U.FlorenceProcessor(RC.write_tokenizer(tmp_path / "good"), image_token_id=1400).loc_class_table()
    assert len(table) == len(texts) == 1400 and table.dtype.name == "uint16" and texts[RC.LOC0 + 5] == "<loc_5>"


def test_cells_are_midpoints_of_the_overlaps():
    from omniparser_amd.florence import OCR_INF, ocr_cells, ocr_slots
    assert ocr_cells([(0, 0)], 64) == [[0, 0, -2 ** 31, OCR_INF, -2 ** 31, OCR_INF]]
    assert ocr_cells([(0, 0), (64, 0)], 64)[0][3] == 128 == ocr_cells([(0, 0), (64, 0)], 64)[1][2]       # no overlap: the seam itself
    assert [ocr_slots(t) for t in (2, 9, 10, 19, 65, 1025)] == [0, 0, 1, 2, 7, 113]


def test_header_python_and_profiler_agree_on_the_op():
    from omniparser_amd import florence as FL
    from omniparser_amd import opwork
    hdr = (Path(__file__).resolve().parents[1] / "include" / "omni_amd.h").read_text()
    assert re.search(r"OMNI_OP_REGION_OCR = OMNI_OP_VISUAL_MATCH \+ 1,\s*/\* 29\b.*?\*/\s*OMNI_OP__END\s*\}", hdr)
    assert L.OP_REGION_OCR == 29 == L.OP_VISUAL_MATCH + 1
    assert len(re.findall(r"\b(OMNI_OP_[A-Z0-9_]+) = (\d+),", hdr)) == 24 and "#define OMNI_ABI_VERSION 3" in hdr
    for name, val in (("STRIP", L.OCR_CLASS_STRIP), ("TEXT", L.OCR_CLASS_TEXT), ("HARD", L.OCR_CLASS_HARD)):
        assert f"#define OMNI_OCR_CLASS_{name} {val}\n" in hdr
    doc = re.search(r"/\* REGION OCR.*?\*/\s*OMNI_OP_REGION_OCR = ", hdr, re.S).group(0)
    for word in ("tile_cut_kernel", "region_parse_kernel", "2049", "(T - 1) / 9", "i13", "OMNI_E_ARG"):
        assert word in doc, word
    assert FL.OCR_MAX_T == 2049
    cut = FL.tile_cut_op(L.F16, 1, 2, 3, 4, 6, 1080, 1920, 768, 8)
    par = FL.region_parse_op(1, 2, 3, 4, 5, 6, 7, 6, 1025, 51289, 768, 2)
    assert par.i[3] == 113 and opwork.op_kernel(cut) == "region_ocr (tile cut)" and opwork.op_kernel(par) == "region_ocr (parse)"
    assert opwork.op_work(cut, 2) == (6 * 6 * 768 * 768, 6 * 768 * 768 * (3 + 16)) and opwork.op_shape(cut) == (6, 768, 0)
    assert opwork.op_work(par) == (0, 6 * (4 * 1025 + 4 * 1024 + 68 * 113 + 40)) and opwork.op_shape(par) == (6, 1025, 0)


# ---------------------------------------------------------------------------------------------- host surface over a stand-in reader
def _stand_in(tok_dir):
    import region_checks as RC
    proc, _ = RC.oracle(tok_dir)
    return {"model": RC.StandInReader(L), "processor": proc}


def test_read_text_regions_and_florence_ocr_with_a_stand_in_reader(emu, tok_dir):
    """tile cut and region parse are the real op on the emulation, the decode between them is canned (RC.StandInReader)"""
    import region_checks as RC
    cmp_ = _stand_in(tok_dir)
    img = RC.frame(150, 100)
    regions, stats = RC.check_read_text_regions(cmp_, img, dict(max_new_tokens=64, overlap=16))
    # the stand-in really cut the tiles: its last call's input is the processor's
    assert torch.equal(cmp_["model"].tiles[..., :3], RC.host_tiles(img, [(0, 0), (43, 0), (86, 0), (0, 36), (43, 36), (86, 36)], 64).permute(0, 2, 3, 1))
    assert [s["fallback"] for s in stats] == [False, False, True, False, False, False] and not any(s["truncated"] for s in stats)
    assert [s["found"] for s in stats] == [2, 1, 1, 1, 0, 2]
    # tile 1 reads whitespace only: found and (by its centre) possibly kept, never returned; tile 2 is parsed from its text
    assert all(g["tile"] != 1 for g in regions)
    from omniparser_amd.util import utils as U
    proc, post = RC.oracle(tok_dir)
    row2 = cmp_["model"].canned(2, 65)
    assert [(g["text"], g["quad"]) for g in U.parse_ocr_regions(row2, proc, (64, 64))] == RC.oracle_regions(post, row2, 64) == [("B", [0, 1, 32, 1, 32, 19, 0, 19])]


def test_surface_validation_errors(emu, tok_dir, tmp_path):
    import region_checks as RC
    from omniparser_amd.util import utils as U
    cmp_ = _stand_in(tok_dir)
    img = RC.frame(70, 70)
    for kw in (dict(overlap=64), dict(overlap=-1), dict(overlap=True), dict(overlap=1.5), dict(max_new_tokens=0), dict(max_new_tokens=1025),
               dict(min_confidence=1.5), dict(min_confidence=-0.1), dict(min_confidence="x")):
        with pytest.raises(ValueError):
            U.read_text_regions(img, cmp_, **kw)
    with pytest.raises(ValueError, match="tokenizer.json"):
        U.read_text_regions(img, {"model": cmp_["model"], "processor": U.FlorenceProcessor(tmp_path / "nowhere")})
    assert cmp_["model"].calls == []                        # nothing reached the reader
    with pytest.raises(ValueError, match="unknown"):
        U.FlorenceOCR(cmp_, text_threshold=0.5)


@pytest.fixture(scope="module")
def host_cap():
    """a captioner object without a device: the argument checks run before anything touches one"""
    from omniparser_amd.florence import Florence2Captioner, FlorenceWeights
    from tools.make_weights import ensure_caption_checkpoint
    cap = Florence2Captioner.__new__(Florence2Captioner)
    cap.w = FlorenceWeights(ensure_caption_checkpoint(0))
    cap.num_beams, cap.token_scores, cap.resolution, cap._plans = 1, False, 64, {}
    return cap


def test_bad_read_regions_arguments_are_value_errors_before_any_device_work(host_cap, tok_dir):
    import numpy as np
    import region_checks as RC
    proc, _ = RC.oracle(tok_dir)
    table, _ = proc.loc_class_table()
    img = torch.zeros(70, 70, 3, dtype=torch.uint8)
    good = dict(max_new_tokens=64, overlap=16, prompt_ids=proc.prompt_ids("<OCR_WITH_REGION>"), class_table=table)
    for kw in (dict(prompt_ids=None), dict(class_table=None), dict(class_table=np.zeros((0,), np.uint16)), dict(class_table=[1, 2]),
               dict(class_table=np.zeros((4, 4), np.uint16)), dict(overlap=64), dict(overlap=-1), dict(overlap=True), dict(overlap=16.0),
               dict(max_new_tokens=0), dict(max_new_tokens=host_cap.max_new_limit() + 1), dict(max_new_tokens=True),
               dict(controls={"repetition_penalty": -1.0}), dict(controls={"no_such_control": 1})):
        with pytest.raises(ValueError):
            host_cap.read_regions(img, **{**good, **kw})
    for bad in (torch.zeros(70, 70, 3), torch.zeros(70, 70, 4, dtype=torch.uint8), torch.zeros(70, 70, dtype=torch.uint8), "frame"):
        with pytest.raises(ValueError, match="uint8"):
            host_cap.read_regions(bad, **good)
    assert host_cap._plans == {}


def test_omniparser_florence_provider(monkeypatch, emu, tok_dir):
    """fake detector, stand-in reader: "florence" installs a FlorenceOCR over the object's OWN caption model with the ocr_* settings;
    what `_ocr` hands to the detector glue are exactly read_text_regions' texts and boxes; a callable and None stay what they were"""
    import types
    import region_checks as RC
    from PIL import Image
    from omniparser_amd.util import omniparser as F
    from omniparser_amd.util import utils as U
    cmp_ = _stand_in(tok_dir)
    monkeypatch.setattr(U, "get_yolo_model", lambda model_path, device: object())
    monkeypatch.setattr(U, "get_caption_model_processor", lambda model_name, model_name_or_path, device: cmp_)
    base = {"som_model_path": "x", "caption_model_name": "florence2", "caption_model_path": "y", "BOX_TRESHOLD": 0.05}
    op = F.Omniparser({**base, "ocr_provider": "florence", "ocr_max_new_tokens": 64, "ocr_overlap": 16, "ocr_min_confidence": 0.0})
    assert isinstance(op.ocr_provider, U.FlorenceOCR) and op.ocr_provider.caption_model_processor is cmp_
    assert op.ocr_provider.defaults == {"max_new_tokens": 64, "overlap": 16, "min_confidence": 0.0}
    img = RC.frame(150, 100)
    regions = U.read_text_regions(img, cmp_, max_new_tokens=64, overlap=16)
    texts, boxes = op._ocr(Image.fromarray(img))
    assert texts == [g["text"] for g in regions] and [list(b) for b in boxes] == [g["bbox"] for g in regions] and regions
    assert (texts, boxes) == op._ocr(Image.fromarray(img), ocr=([g["text"] for g in regions], [g["bbox"] for g in regions]))
    assert cmp_["model"].calls[-1] == dict(max_new_tokens=64, overlap=16, controls=None)
    fn = lambda image: (["a"], [[1, 2, 3, 4]])
    assert F.Omniparser({**base, "ocr_provider": fn}).ocr_provider is fn and F.Omniparser(base).ocr_provider is None
    assert F.Omniparser({**base, "ocr_provider": fn})._ocr(Image.fromarray(img)) == (["a"], [(1, 2, 3, 4)])
    for bad in ({"ocr_provider": "easyocr"}, {"ocr_provider": 3}, {"ocr_provider": "florence", "ocr_max_new_tokens": 0},
                {"ocr_provider": "florence", "ocr_overlap": -1}, {"ocr_provider": "florence", "ocr_overlap": True},
                {"ocr_provider": "florence", "ocr_min_confidence": 2}, {"ocr_provider": "florence", "ocr_generation": [1]},
                {"ocr_provider": "florence", "ocr_generation": {"nope": 1}}, {"ocr_overlap": 16}, {"ocr_provider": fn, "ocr_max_new_tokens": 64}):
        with pytest.raises(ValueError):
            F.Omniparser({**base, **bad})


def test_server_passes_the_provider_through():
    import inspect
    from omniparser_amd import server
    assert '"--ocr_provider"' in inspect.getsource(server.main) and "build_app(vars(a))" in inspect.getsource(server.main)

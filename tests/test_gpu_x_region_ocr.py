"""`-m gpu`: region OCR on the MI355X — OMNI_OP_REGION_OCR case by case (mode 1 bit-equal to a literal host restatement and equal to
transformers' Florence2PostProcessor; mode 0 bit-equal to the image processor on Pillow crops, f32 and f16 plans), the ownership rule,
the argument checks, Florence2Captioner.read_regions against generate() and against transformers on the CPU, and the public surface
(read_text_regions, FlorenceOCR behind check_ocr_box, Omniparser's "florence" provider).  Helpers: tests/region_checks.py; the
host-emulation twin: tests/test_region_ocr_emu_cpu.py."""
import pytest

from omniparser_amd import _lib as L

pytestmark = pytest.mark.gpu


def _dev():
    import gpu_checks as G
    return G.DEV, G._sync


@pytest.fixture(scope="module")
def tok_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("region_ocr")


# ---------------------------------------------------------------------------------------------- kernel, one launch per case
@pytest.mark.parametrize("n", [1, 3, 17])
@pytest.mark.parametrize("T", [10, 19, 65, 1025])
def test_parse_is_the_twin_and_transformers(tok_dir, T, n):
    import region_checks as RC
    dev, sync = _dev()
    RC.check_parse(L, dev, tok_dir, T, n, sync=sync)


def test_parse_without_log_probabilities(tok_dir):
    import region_checks as RC
    dev, sync = _dev()
    RC.check_parse(L, dev, tok_dir, 65, 17, with_logp=False, sync=sync)


def test_parse_at_the_other_resolution(tok_dir):
    import region_checks as RC
    dev, sync = _dev()
    RC.check_parse(L, dev, tok_dir, 65, 17, R=768, sync=sync)


def test_the_listed_rows_give_what_the_list_says(tok_dir):
    import region_checks as RC
    dev, sync = _dev()
    RC.check_expected_counts(L, dev, tok_dir, sync=sync)


def test_ownership_on_a_3x2_grid_and_exactly_on_the_boundaries(tok_dir):
    import region_checks as RC
    dev, sync = _dev()
    RC.check_ownership(L, dev, tok_dir, sync=sync)


def test_parse_argument_errors(tok_dir):
    import region_checks as RC
    dev, sync = _dev()
    seen = RC.check_parse_errors(L, dev, tok_dir, sync=sync)
    assert all("region_ocr" in msg for _, msg in seen), seen


@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("name", ["six_tiles", "one_tile", "narrower_than_a_tile"])
def test_tile_cut_is_the_processor_on_pillow_crops(name, f16):
    import region_checks as RC
    dev, sync = _dev()
    RC.check_cut(L, dev, name, f16, sync=sync)


def test_tile_cut_argument_errors():
    import region_checks as RC
    dev, sync = _dev()
    seen = RC.check_cut_errors(L, dev, sync=sync)
    assert all("region_ocr" in msg for _, msg in seen), seen


# ---------------------------------------------------------------------------------------------- captioner
@pytest.mark.parametrize("eos_prone", [False, True])
def test_read_regions_is_generate_transformers_and_the_post_processor(tok_dir, eos_prone):
    """R = 64, 150 x 100 frame (6 tiles), 64 new tokens, generation restricted to the location tokens and 40 text tokens; the stock
    checkpoint gives 6 regions per tile, the EOS-prone one ends every tile at once (the early exit)"""
    import region_checks as RC
    cap, _proc, _ref, out = RC.check_read_regions(tok_dir, eos_prone)
    if eos_prone:
        assert cap.last_steps < RC.OCR_MAX_NEW and not out.rows[:, 0].any()
    else:
        assert cap.last_steps == RC.OCR_MAX_NEW and int(out.rows[:, 0].sum()) >= 4


def test_read_regions_at_768_cuts_the_processors_tiles_and_decodes_like_generate():
    import region_checks as RC
    out = RC.check_read_regions_768()
    assert len(out.origins) == 4 and tuple(out.ids.shape) == (4, 17)


# ---------------------------------------------------------------------------------------------- public surface, real captioner
def _cmp64(tok_dir):
    import os
    import region_checks as RC
    from omniparser_amd.util import utils as U
    os.environ["OMNI_CAPTION_RES"] = "64"
    try:
        return U.get_caption_model_processor("florence2", str(RC.caption_dir_with_tokenizer(tok_dir)), "cuda")
    finally:
        os.environ.pop("OMNI_CAPTION_RES", None)


def test_read_text_regions_and_florence_ocr(tok_dir):
    import region_checks as RC
    cmp_ = _cmp64(tok_dir)
    kw = dict(max_new_tokens=RC.OCR_MAX_NEW, overlap=16, generation={"suppress_tokens": RC.ocr_suppress(cmp_["model"].w.vocab, keep=(RC.BOS, RC.EOS))})
    regions, stats = RC.check_read_text_regions(cmp_, RC.frame(150, 100), kw)
    print(f"read_text_regions: {len(regions)} regions returned, per tile found/kept {[(s['found'], s['kept']) for s in stats]}")
    # without the restriction the stand-in writes ids the synthetic tokenizer does not know: every tile falls back to its text
    _r, plain = RC.check_read_text_regions(cmp_, RC.frame(150, 100), dict(max_new_tokens=16, overlap=16), expect_some=False)
    assert all(s["fallback"] for s in plain)


def test_omniparser_reads_its_own_text(tok_dir):
    """Omniparser({"ocr_provider": "florence"}).parse on a bare screenshot = parse(ocr=(texts, boxes)) fed read_text_regions' lists;
    its text elements are those regions"""
    import base64
    import io
    import os
    import region_checks as RC
    from PIL import Image
    from omniparser_amd.synth import synthetic_screenshot
    from omniparser_amd.util import utils as U
    from omniparser_amd.util.omniparser import Omniparser
    from tools.make_weights import ensure_blob
    arr = synthetic_screenshot(2, 480, 320)
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, format="PNG")
    b64 = base64.b64encode(buf.getvalue()).decode("ascii")
    base = {"som_model_path": str(ensure_blob(seed=0, nc=1, width=0.5)), "caption_model_name": "florence2",
            "caption_model_path": str(RC.caption_dir_with_tokenizer(tok_dir)), "BOX_TRESHOLD": 0.05}
    gen = {"suppress_tokens": RC.ocr_suppress(51289, keep=(RC.BOS, RC.EOS))}
    os.environ["OMNI_CAPTION_RES"] = "64"
    try:
        op = Omniparser({**base, "ocr_provider": "florence", "ocr_max_new_tokens": 32, "ocr_overlap": 16, "ocr_generation": gen})
    finally:
        os.environ.pop("OMNI_CAPTION_RES", None)
    regions = U.read_text_regions(arr, op.caption_model_processor, max_new_tokens=32, overlap=16, generation=gen)
    assert regions
    png, elements = op.parse(b64)
    png2, elements2 = op.parse(b64, ocr=([g["text"] for g in regions], [g["bbox"] for g in regions]))
    assert png == png2 and elements == elements2
    texts = [e["content"] for e in elements if e["type"] == "text"]
    assert texts and set(texts) <= {g["text"] for g in regions}

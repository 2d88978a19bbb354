"""`-m gpu`: grounding on the MI355X — OMNI_OP_REGION_OCR mode 3 case by case (bit-equal to a literal host restatement and equal to
transformers' three box parses), the ownership rule, the argument checks, modes 0 / 1 / 2 as before,
Florence2Captioner.locate_regions / decode_tiles against generate() and against transformers on the CPU, and
util.utils.describe_regions with the real captioner.  Helpers: tests/box_checks.py; the host-emulation twin:
tests/test_region_boxes_emu_cpu.py."""
import pytest

from omniparser_amd import _lib as L

pytestmark = pytest.mark.gpu


def _dev():
    import gpu_checks as G
    return G.DEV, G._sync


@pytest.fixture(scope="module")
def tok_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("region_boxes")


# ---------------------------------------------------------------------------------------------- kernel, one launch per case
@pytest.mark.parametrize("grammar", [0, 1])
@pytest.mark.parametrize("n", [1, 3, 17])
@pytest.mark.parametrize("T", [6, 10, 19, 65, 1025])
def test_boxes_are_the_twin_and_transformers(tok_dir, T, n, grammar):
    import box_checks as BX
    dev, sync = _dev()
    BX.check_boxes(L, dev, tok_dir, T, n, grammar, sync=sync)


@pytest.mark.parametrize("grammar", [0, 1])
def test_boxes_without_log_probabilities(tok_dir, grammar):
    import box_checks as BX
    dev, sync = _dev()
    BX.check_boxes(L, dev, tok_dir, 65, 23, grammar, with_logp=False, sync=sync)


@pytest.mark.parametrize("grammar", [0, 1])
def test_boxes_at_the_other_resolution(tok_dir, grammar):
    import box_checks as BX
    dev, sync = _dev()
    BX.check_boxes(L, dev, tok_dir, 65, 23, grammar, R=768, sync=sync)


@pytest.mark.parametrize("text_share", [0.05, 0.2, 0.5])
@pytest.mark.parametrize("grammar", [0, 1])
def test_random_rows_are_the_twin_and_transformers(tok_dir, grammar, text_share):
    import box_checks as BX
    dev, sync = _dev()
    assert BX.check_random(L, dev, tok_dir, grammar, text_share, sync=sync) > 100


def test_the_listed_rows_give_what_the_list_says(tok_dir):
    import box_checks as BX
    dev, sync = _dev()
    BX.check_expected(L, dev, tok_dir, sync=sync)


def test_ownership_on_a_3x2_grid_and_exactly_on_the_boundaries(tok_dir):
    import box_checks as BX
    dev, sync = _dev()
    BX.check_ownership(L, dev, tok_dir, sync=sync)


def test_box_argument_errors(tok_dir):
    import box_checks as BX
    dev, sync = _dev()
    seen = BX.check_errors(L, dev, tok_dir, sync=sync)
    assert all("region_ocr" in msg for _, msg in seen), seen


def test_modes_0_1_and_2_behave_as_before(tok_dir):
    import region_checks as RC
    dev, sync = _dev()
    RC.check_parse(L, dev, tok_dir, 19, 3, sync=sync)
    RC.check_cut(L, dev, "six_tiles", False, sync=sync)
    seen = dict(RC.check_parse_errors(L, dev, tok_dir, sync=sync))
    assert "region_ocr" in seen["mode 2"]


# ---------------------------------------------------------------------------------------------- captioner
@pytest.mark.parametrize("eos_prone", [False, True])
def test_locate_regions_is_generate_transformers_and_the_post_processor(tok_dir, eos_prone):
    """R = 64, 150 x 100 frame (6 tiles), two <OPEN_VOCABULARY_DETECTION> phrases (12 rows), 64 new tokens, generation restricted to
    the location tokens and 40 text tokens; the EOS-prone checkpoint ends every row at once (the early exit)"""
    import box_checks as BX
    import region_checks as RC
    cap, _proc, _ref, out = BX.check_locate_regions(tok_dir, eos_prone)
    if eos_prone:
        assert cap.last_steps < RC.OCR_MAX_NEW and not out.rows[:, 0].any()
    else:
        assert int(out.rows[:, 0].min()) >= 1


def test_describe_regions_decodes_transformers_rows(tok_dir):
    import box_checks as BX
    BX.check_describe_regions(tok_dir)


def test_locate_regions_at_768_decodes_like_generate():
    import box_checks as BX
    out = BX.check_locate_regions_768()
    assert len(out.origins) == 4 and tuple(out.ids.shape) == (4, 17) and tuple(out.records.shape) == (4, 4, 16)

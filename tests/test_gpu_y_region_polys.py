"""`-m gpu`: segmentation on the MI355X — OMNI_OP_REGION_OCR mode 5 case by case (bit-equal to a literal host restatement and equal to
transformers' "polygons" parse), mode 6 bit-equal to its twin with written-down rectangles and Pillow beside it, the ownership rule,
the argument checks and the old refusals.  Helpers: tests/poly_checks.py; the host-emulation twin: tests/test_region_polys_emu_cpu.py."""
import pytest

from omniparser_amd import _lib as L

pytestmark = pytest.mark.gpu


def _dev():
    import gpu_checks as G
    return G.DEV, G._sync


@pytest.fixture(scope="module")
def tok_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("region_polys")


# ---------------------------------------------------------------------------------------------- mode 5, one launch per case
@pytest.mark.parametrize("n", [1, 3, 17])
@pytest.mark.parametrize("T", [3, 5, 6, 9, 65, 1025])
def test_polygons_are_the_twin_and_transformers(tok_dir, T, n):
    import poly_checks as PC
    dev, sync = _dev()
    PC.check_polys(L, dev, tok_dir, T, n, sync=sync)


def test_polygons_without_log_probabilities(tok_dir):
    import poly_checks as PC
    dev, sync = _dev()
    PC.check_polys(L, dev, tok_dir, 65, 19, with_logp=False, sync=sync)


def test_polygons_at_the_other_resolution(tok_dir):
    import poly_checks as PC
    dev, sync = _dev()
    PC.check_polys(L, dev, tok_dir, 65, 19, R=768, sync=sync)


@pytest.mark.parametrize("text_share", [0.02, 0.05, 0.1])
def test_random_rows_are_the_twin_and_transformers(tok_dir, text_share):
    import poly_checks as PC
    dev, sync = _dev()
    assert PC.check_random(L, dev, tok_dir, text_share, sync=sync) > 100


def test_the_listed_rows_give_what_the_list_says(tok_dir):
    import poly_checks as PC
    dev, sync = _dev()
    PC.check_expected(L, dev, tok_dir, sync=sync)


def test_instance_ownership_on_a_3x2_grid_and_exactly_on_the_boundaries(tok_dir):
    import poly_checks as PC
    dev, sync = _dev()
    PC.check_ownership(L, dev, tok_dir, sync=sync)


def test_polygon_and_mask_argument_errors(tok_dir):
    import poly_checks as PC
    dev, sync = _dev()
    seen = PC.check_errors(L, dev, tok_dir, sync=sync)
    assert all("region_ocr" in msg for _, msg in seen), seen


def test_modes_1_and_3_refuse_modes_2_and_4_as_before(tok_dir):
    import box_checks as BX
    import region_checks as RC
    dev, sync = _dev()
    assert "region_ocr" in dict(RC.check_parse_errors(L, dev, tok_dir, sync=sync))["mode 2"]
    seen = dict(BX.check_errors(L, dev, tok_dir, sync=sync))
    assert "mode 2" in seen["mode 2"] and "mode 4" in seen["mode 4"]


# ---------------------------------------------------------------------------------------------- mode 6
@pytest.mark.parametrize("frame", [(30, 20), (64, 64), (150, 100)])
@pytest.mark.parametrize("I", [1, 4])
@pytest.mark.parametrize("R", [32, 40, 64])
def test_masks_are_the_twin(R, I, frame):
    import poly_checks as PC
    dev, sync = _dev()
    assert PC.check_masks(L, dev, R, I, frame, sync=sync) > 0


def test_masks_of_rectangles_frame_edges_and_a_1024_vertex_polygon():
    import poly_checks as PC
    dev, sync = _dev()
    PC.check_masks_known(L, dev, sync=sync)


def test_masks_of_one_row_at_768():
    import poly_checks as PC
    dev, sync = _dev()
    PC.check_masks_768(L, dev, sync=sync)


def test_masks_agree_with_pillow_away_from_the_edges():
    import poly_checks as PC
    dev, sync = _dev()
    assert PC.check_masks_pillow(L, dev, sync=sync) < 0.25


# ---------------------------------------------------------------------------------------------- captioner
@pytest.mark.parametrize("eos_prone", [False, True])
def test_segment_is_transformers_the_post_processor_and_the_mask_twin(tok_dir, eos_prone):
    """R = 64, 150 x 100 frame (6 tiles): one phrase over all tiles, then three boxes, 48 new tokens, generation restricted to the
    location tokens, the three polygon tokens and EOS; the EOS-prone checkpoint ends every row at once (the early exit)"""
    import poly_checks as PC
    by_text, by_box = PC.check_segment_captioner(tok_dir, eos_prone)
    if not eos_prone:
        assert by_text and all(g["area"] > 0 and g["point"] is not None and g["mask"][g["point"][1] - g["bbox"][1], g["point"][0] - g["bbox"][0]]
                               for g in by_text + by_box if g["area"])

"""Visual embeddings and exemplar matching on the host emulation of the HIP kernels (tests/emu) and on the host alone:
OMNI_OP_VISUAL_MATCH case by case against f64, Florence2Captioner.embed against transformers, the embed plan, the equality of the
entry points, the argument checks and the public surface.  Helpers and bounds: tests/match_checks.py; the MI355X twin:
tests/test_gpu_w_visual_match.py."""
import re
import types
from pathlib import Path

import pytest
import torch

from omniparser_amd import _lib as L

CPU = torch.device("cpu")
SRC = pytest.mark.parametrize("f16", [False, True])


# ---------------------------------------------------------------------------------------------- kernel, one launch per case
@SRC
def test_embed_rows_vs_f64(emu, f16):
    import match_checks as MC
    MC.check_embed(L, CPU, f16)


@SRC
def test_embed_rows_at_layernorm_scale(emu, f16):
    import match_checks as MC
    MC.check_embed(L, CPU, f16, sigma=1.0)


@pytest.mark.parametrize("k", [8, 1])
def test_match_vs_f64_under_both_splits(emu, k):
    import match_checks as MC
    MC.check_match(L, CPU, k)


@pytest.mark.parametrize("k", [8, 1])
def test_ties_go_to_the_lower_index(emu, k):
    import match_checks as MC
    MC.check_match(L, CPU, k, ties=True)


def test_short_gallery_pads_with_minus_one(emu):
    import match_checks as MC
    MC.check_short_gallery(L, CPU)


def test_two_query_groups(emu):
    import match_checks as MC
    MC.check_two_groups(L, CPU)


def test_odd_width_wide_rows_and_default_slices(emu):
    import match_checks as MC
    MC.check_odd_width(L, CPU)


def test_argument_errors(emu):
    import match_checks as MC
    seen = MC.check_argument_errors(L, CPU)
    assert all("visual_match" in msg for _, msg in seen), seen


def test_match_seed_is_the_first_the_reference_can_rank():
    import match_checks as MC
    assert MC.find_seed() == MC.MATCH_SEED


# ---------------------------------------------------------------------------------------------- captioner (emulated encodes are slow:
# one seed, two decode steps where a decode is only there to fill a caption plan)
def test_embed_matches_transformers_f64(emu):
    import match_checks as MC
    e = MC.embed_vs_f64(MC.captioner(), MC.EMBED_SEEDS[0])
    assert e < MC.TOL_EMBED_F32, e


def test_embed_plan_and_entry_points(emu):
    """(the unchanged-defaults check and the full set of entry points run on the MI355X only: tests/test_gpu_w_visual_match.py)"""
    import match_checks as MC
    cap = MC.captioner()
    MC.check_embed_plan(cap, L, max_new=2)
    MC.check_entry_points(cap, n_boxes=2, max_new=2, beams=False, lean=True)


def test_public_surface_with_a_stand_in_embedder(emu):
    """match_elements / track_elements / ScreenParser.embed, match, track over embeddings that are a cheap pure function of the crop's
    pixels; the matching itself is the real op on the emulation.  With the real captioner: the MI355X twin."""
    import match_checks as MC
    from omniparser_amd.util import utils as U
    MC.check_public_surface(MC.PooledPixels(), U.FlorenceProcessor(None))


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


def test_bad_match_arguments_are_value_errors_before_any_device_work(host_cap):
    q, g = torch.zeros(3, 768), torch.zeros(5, 768)
    bad = [dict(top_k=0), dict(top_k=9), dict(top_k=True), dict(top_k=2.0), dict(top_k=None), dict(gallery=torch.zeros(5, 764)),
           dict(queries=torch.zeros(0, 768)), dict(gallery=torch.zeros(0, 768)), dict(queries=torch.zeros(3, 768, dtype=torch.float64)),
           dict(queries=torch.zeros(2, 6), gallery=torch.zeros(2, 6)), dict(queries=torch.zeros(1, 4100), gallery=torch.zeros(1, 4100)),
           dict(queries=torch.zeros(4097, 4), gallery=torch.zeros(1, 4)), dict(gallery=torch.zeros(65537, 4), queries=torch.zeros(1, 4)),
           dict(queries=[[0.0] * 768])]
    from omniparser_amd.florence import match_topk
    for kw in bad:
        a = dict(queries=q, gallery=g, top_k=1)
        a.update(kw)
        with pytest.raises(ValueError):
            host_cap.match(a["queries"], a["gallery"], top_k=a["top_k"])
        with pytest.raises(ValueError):
            match_topk(a["queries"], a["gallery"], a["top_k"])
    with pytest.raises(ValueError, match="return_embeddings"):
        host_cap.caption_crops(torch.zeros(64, 64, 3, dtype=torch.uint8), [[0, 0, 8, 8]], return_embeddings=1)
    assert host_cap._plans == {}


def test_track_elements_is_one_to_one_and_ties_go_to_the_lower_index(emu):
    """four prev elements and five cur elements given as embeddings: twins 0 = 1 on both sides (equal scores everywhere), a pair below
    min_score, an element without a partner"""
    from omniparser_amd.util import utils as U
    g = torch.Generator().manual_seed(3)
    base = torch.nn.functional.normalize(torch.randn(4, 768, generator=g, dtype=torch.float64), dim=1)
    far = torch.nn.functional.normalize(base[3] + 0.8 * torch.nn.functional.normalize(torch.randn(768, generator=g, dtype=torch.float64), dim=0), dim=0)
    prev = ([10, 11, 12, 13], torch.stack([base[0], base[0], base[1], base[3]]).float())
    cur = ([20, 21, 22, 23, 24], torch.stack([base[2], base[0], base[0], base[1], far]).float())
    pairs = U.track_elements(prev, cur, min_score=0.9)
    assert [(a, b) for a, b, _ in pairs] == [(10, 21), (11, 22), (12, 23)] and all(s > 0.99999 for _, _, s in pairs)
    loose = U.track_elements(prev, cur, min_score=0.5)
    assert [(a, b) for a, b, _ in loose] == [(10, 21), (11, 22), (12, 23), (13, 24)] and 0.7 < loose[3][2] < 0.85
    assert [(a, b) for a, b, _ in U.track_elements(prev, cur, min_score=0.9, top_k=1)] == [(10, 21), (12, 23)]
    for bad in (0, 9, True):
        with pytest.raises(ValueError):
            U.track_elements(prev, cur, top_k=bad)
    with pytest.raises(ValueError):
        U.track_elements(([1], prev[1]), cur)


def test_find_similar_is_parse_plus_match_elements(monkeypatch):
    """fake models: the exemplars are decoded like the screenshot and handed to match_elements with the parsed elements"""
    import base64
    import io
    import numpy as np
    from PIL import Image
    from omniparser_amd.util import omniparser as F
    from omniparser_amd.util import utils as U
    monkeypatch.setattr(U, "get_yolo_model", lambda model_path, device: object())
    monkeypatch.setattr(U, "get_caption_model_processor", lambda model_name, model_name_or_path, device: {"model": types.SimpleNamespace(token_scores=False), "processor": None})
    op = F.Omniparser({"som_model_path": "x", "caption_model_name": "florence2", "caption_model_path": "y", "BOX_TRESHOLD": 0.05})
    elements = [{"type": "icon", "bbox": [0.1, 0.1, 0.2, 0.2], "content": "a"}]
    monkeypatch.setattr(op, "parse_image", lambda image, ocr=None: ("png", elements))
    seen = {}

    def fake(image_source, els, cmp_, exemplars, top_k=5, min_score=None):
        seen.update(image=image_source, elements=els, cmp=cmp_, exemplars=exemplars, top_k=top_k)
        return [[{"index": 0, "score": 1.0}] for _ in exemplars]
    monkeypatch.setattr(U, "match_elements", fake)

    def b64(arr):
        buf = io.BytesIO()
        Image.fromarray(arr).save(buf, format="PNG")
        return base64.b64encode(buf.getvalue()).decode("ascii")
    rng = np.random.default_rng(0)
    shot, ex = rng.integers(0, 256, (40, 60, 3), dtype=np.uint8), [rng.integers(0, 256, (9, 7, 3), dtype=np.uint8) for _ in range(2)]
    got_elements, matches = op.find_similar(b64(shot), [b64(e) for e in ex], top_k=3)
    assert got_elements is elements and matches == [[{"index": 0, "score": 1.0}]] * 2 and seen["top_k"] == 3
    assert np.array_equal(seen["image"], shot) and all(np.array_equal(a, b) for a, b in zip(seen["exemplars"], ex))
    assert seen["elements"] is elements and seen["cmp"] is op.caption_model_processor
    with pytest.raises(ValueError):
        op.find_similar(b64(shot), b64(ex[0]))


def test_header_python_and_profiler_agree_on_the_op():
    from omniparser_amd import florence as FL
    from omniparser_amd import opwork
    hdr = (Path(__file__).resolve().parents[1] / "include" / "omni_amd.h").read_text()
    assert re.search(r"OMNI_OP_GREEDY_VOCAB_STEP = OMNI_OP_GREEDY_CTRL_STEP \+ 1,\s*/\*.*?\*/\s*/\*.*?\*/\s*OMNI_OP_VISUAL_MATCH = OMNI_OP_GREEDY_VOCAB_STEP \+ 1,\s*/\* 28\b.*?\*/\s*OMNI_OP__END\s*\}", hdr, re.S)
    assert L.OP_VISUAL_MATCH == 28 == L.OP_GREEDY_VOCAB_STEP + 1
    assert len(re.findall(r"\b(OMNI_OP_[A-Z0-9_]+) = (\d+),", hdr)) == 24 and "#define OMNI_ABI_VERSION 3" in hdr
    doc = re.search(r"/\* VISUAL EMBEDDINGS.*?\*/\s*OMNI_OP_VISUAL_MATCH = ", hdr, re.S).group(0)
    for word in ("embed_rows_kernel", "match_partial_kernel", "match_merge_kernel", "i5", "i6", "65536", "4096"):
        assert word in doc, word
    assert (FL.MATCH_MAX_K, FL.MATCH_MAX_D, FL.MATCH_MAX_QUERIES, FL.MATCH_MAX_GALLERY) == (8, 4096, 4096, 65536)
    assert "omni_visual_match_cfg" in L.EXPORTS and "int omni_visual_match_cfg(" in hdr
    one, two = FL.match_ops(1, 2, 3, 4, 5, 300, 65536, 768, 5, 2048, 0)
    assert opwork.op_kernel(one) == "visual_match (partial top-k)" and opwork.op_kernel(two) == "visual_match (merge)"
    assert opwork.op_work(one) == (2 * 300 * 65536 * 768, 4 * (300 + 65536) * 768 + 8 * 300 * 32 * 5)
    assert opwork.op_work(two) == (0, 8 * 300 * 32 * 5 + 8 * 300 * 5) and opwork.op_shape(one) == (300, 768, 65536)
    emb = FL.embed_op(L.F16, 1, 577 * 768, torch.zeros(1), torch.zeros(1), 128, 768)
    assert opwork.op_kernel(emb) == "visual_match (embed)" and opwork.op_work(emb, 2) == (3 * 128 * 768, 128 * 768 * 6 + 4 * 128)
    assert opwork.op_shape(emb) == (128, 768, 0)


def test_launcher_fills_the_chip_for_a_large_gallery(emu):
    """the launcher's own split (omni_visual_match_cfg): one block per query group for a small gallery, about 1024 blocks for a large one"""
    from omniparser_amd.florence import match_geometry
    assert match_geometry(300, 300, 768, 5) == (38, 300, 1, 300 * 5 * 8)
    groups, length, splits, nbytes = match_geometry(300, 65536, 768, 5)
    assert groups == 38 and splits == 26 and length % 4 == 0 and (splits - 1) * length < 65536 <= splits * length and nbytes == 300 * 26 * 5 * 8
    groups, length, splits, _ = match_geometry(4096, 65536, 768, 8)
    assert (groups, length, splits) == (512, 32768, 2)
    assert match_geometry(3, 70, 768, 8, 32)[1:3] == (32, 3) and match_geometry(1, 65536, 4096, 8)[2] == 256
    for bad in ((0, 1, 4, 1), (1, 0, 4, 1), (1, 1, 6, 1), (1, 1, 4, 9), (4097, 1, 4, 1), (1, 65537, 4, 1), (1, 1, 4100, 1)):
        with pytest.raises(L.OmniError):
            match_geometry(*bad)

"""Long-form greedy decoding on the host emulation of the HIP kernels (tests/emu) and on the host alone: the long-history form of
OMNI_OP_GREEDY_STEP (exact n-gram ban), the split-key self-attention of OMNI_OP_ATTN_DECODE, generate(max_new_tokens=128) against
transformers, the bounds on max_new_tokens, the row limit of long plans and the public surface's argument checks.  Helpers, bounds
and tolerance: tests/long_checks.py; the MI355X twin: tests/test_gpu_q_long_decode.py."""
import types

import pytest
import torch

from omniparser_amd import _lib as L

CPU = torch.device("cpu")
V_EMU = 1037                    # no multiple of 32 or 256


# ---------------------------------------------------------------------------------------------- greedy kernel
@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("scores", [False, True])
def test_greedy_step_bans_every_repeated_ngram_of_a_long_history(emu, f16, scores):
    """B = 4, T = 130, max_new = 129, step = 121: row 0's history holds 40 distinct followers of its last two tokens and its 40
    largest logits are exactly those — transformers bans all 40, a 32-slot list lets the last eight through.  Also a row without
    any ban, a finished row, a row with a repeated follower, ngram 2, the forced EOS at the last position and ngram 0."""
    import long_checks as LC
    worst = LC.check_greedy_long(L, CPU, V_EMU, f16, scores)
    print(f"f16={f16} scores={scores}: worst logp error {worst:.3f} of the bound")


def test_greedy_step_long_form_degenerate_rows(emu):
    import long_checks as LC
    LC.check_degenerate_rows_long(L, CPU, V_EMU)


@pytest.mark.parametrize("f16", [False, True])
def test_greedy_step_forms_agree_at_the_routing_boundary(emu, f16):
    import long_checks as LC
    LC.check_routing_boundary(L, CPU, V_EMU, f16)


# ---------------------------------------------------------------------------------------------- self-attention kernel
@pytest.mark.parametrize("scale", ["unit", "sharp"])
@pytest.mark.parametrize("cap", [65, 130, 1025])
def test_split_key_self_attention_matches_f64(emu, cap, scale):
    """B = 3, 2 heads, f32, cache pitch padded by 64, steps on both sides of the 4-key load, the per-wave quota and the 32-key batch:
    NaN beyond the step never reaches the output, the append is bit-exact, nothing else of the cache changes"""
    import long_checks as LC
    worst = LC.check_self_attn(L, CPU, L.F32, cap, scale)
    print(f"cap={cap} {scale}: worst {worst:.3f} of the bound")


@pytest.mark.parametrize("dtype,ldpad", [("f32", 2), ("f16", 64)])
def test_self_attention_routed_to_the_generic_kernel_keeps_the_bound(emu, dtype, ldpad):
    """cap = 130 with an unaligned cache pitch (f32) and with f16 tensors: the generic kernel, same bound"""
    import long_checks as LC
    for scale in ("unit", "sharp"):
        LC.check_self_attn(L, CPU, L.F32 if dtype == "f32" else L.F16, 130, scale, ldpad=ldpad)


# ---------------------------------------------------------------------------------------------- whole captioner
def test_long_captions_match_transformers_r64_eos_prone(emu):
    """case 2: 4 crops, EOS-prone checkpoint, max_new_tokens = 128: rows end early at several lengths (the early-exit poll and
    finished rows on a long plan); ids equal transformers', log-probabilities within TOL_LOGP_LONG"""
    import long_checks as LC
    cap, out, worst, ref = LC.captioner_long_vs_hf(2)
    assert cap.last_steps < 128                       # the poll ended the decode
    assert out.sequences.shape[1] == ref.shape[1]


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


def test_max_new_tokens_is_bounded_by_the_position_table(host_cap):
    cap = host_cap
    rows = cap.w.sd["model.language_model.decoder.embed_positions.weight"].shape[0]
    assert cap.max_new_limit() == rows - 2 == 1024
    pix = torch.zeros(1, 3, 64, 64)
    frame = torch.zeros(64, 64, 3, dtype=torch.uint8)
    for bad in (0, True, 20.0, rows - 1, -3, "20", None):
        with pytest.raises(ValueError, match=str(rows - 2)):
            cap.generate(pixel_values=pix, max_new_tokens=bad)
        with pytest.raises(ValueError, match=str(rows - 2)):
            cap.caption_crops(frame, [[0, 0, 8, 8]], max_new_tokens=bad)
        with pytest.raises(ValueError, match=str(rows - 2)):
            cap.plans(8, 64, bad)
    assert cap._plans == {}
    assert cap.check_max_new(rows - 2) == rows - 2 and cap.check_max_new(1) == 1


def test_beam_search_refuses_what_its_staging_cannot_hold(host_cap):
    from omniparser_amd.florence import beam_max_new
    cap = host_cap
    pix = torch.zeros(1, 3, 64, 64)
    for k in (2, 3, 8):
        lim = beam_max_new(k)
        assert 3 * k * (lim + 1) * 4 <= 48 * 1024 < 3 * k * (lim + 2) * 4
    assert beam_max_new(3) == 1364 and beam_max_new(8) == 511
    lim = min(beam_max_new(8), cap.max_new_limit())
    with pytest.raises(ValueError, match=str(lim)):
        cap.generate(pixel_values=pix, max_new_tokens=lim + 1, num_beams=8)
    with pytest.raises(ValueError, match=str(lim)):
        cap.plans(8, 64, lim + 1, beam=(8, 1.0, False))
    # num_beams = 3 holds 1364 positions: more than the position table's 1024, which therefore is the limit named
    with pytest.raises(ValueError, match="1024"):
        cap.generate(pixel_values=pix, max_new_tokens=1025, num_beams=3)
    assert cap.check_max_new(lim, (8, 1.0, False)) == lim
    assert cap._plans == {}


def test_beam_limit_below_the_position_table_is_named(host_cap, monkeypatch):
    """num_beams = 3 with a max_new_tokens beyond the LDS staging (a position table long enough to allow it)"""
    import omniparser_amd.florence as FL
    cap = host_cap
    monkeypatch.setattr(FL.Florence2Captioner, "max_new_limit", lambda self: 4096)
    with pytest.raises(ValueError, match="1364"):
        cap.check_max_new(1365, (3, 1.0, False))
    assert cap.check_max_new(1364, (3, 1.0, False)) == 1364


def test_long_plans_take_fewer_rows_under_the_kv_budget(host_cap):
    cap = host_cap
    assert cap.long_kv_budget_bytes == 2 ** 30
    per_row = lambda T: T * cap.w.d_model * 4 * 2 * cap.w.dec_layers
    assert per_row(1025) * 128 > 4.8e9
    assert cap.long_plan_rows(20) == 128 and cap.long_plan_rows(34) == 128
    # T = 1025: 37.8 MB per row -> 28 rows fit into 1 GiB -> the 16-row bucket
    assert 2 ** 30 // per_row(1025) == 28 and cap.long_plan_rows(1024) == 16
    assert cap.long_plan_rows(128) == 128 and cap.long_plan_rows(256) == 96 and cap.long_plan_rows(512) == 32
    assert cap.long_plan_rows(1024, k=3) == 8           # beam / candidate rows count
    cap.long_kv_budget_bytes = 1
    try:
        assert cap.long_plan_rows(1024) == 8            # never below the smallest capacity of the ladder
    finally:
        del cap.long_kv_budget_bytes
    for rows in (cap.long_plan_rows(t) for t in (20, 256, 512, 1024)):
        assert cap.bucket(rows) == rows                 # a capacity the bucket ladder already has


def _fake_models(monkeypatch):
    from omniparser_amd.util import utils as U
    model = types.SimpleNamespace(token_scores=False)
    monkeypatch.setattr(U, "get_yolo_model", lambda model_path, device: object())
    monkeypatch.setattr(U, "get_caption_model_processor", lambda model_name, model_name_or_path, device: {"model": model, "processor": None})
    return {"som_model_path": "x", "caption_model_name": "florence2", "caption_model_path": "y", "BOX_TRESHOLD": 0.05}


def test_omniparser_rejects_a_non_int_caption_max_new_tokens(monkeypatch):
    from omniparser_amd.util import omniparser as F
    cfg = _fake_models(monkeypatch)
    for bad in (True, "20", 20.0, 0, -1, None):
        with pytest.raises(ValueError):
            F.Omniparser({**cfg, "caption_max_new_tokens": bad})
    assert F.Omniparser(cfg).caption_max_new_tokens == 20
    assert F.Omniparser({**cfg, "caption_max_new_tokens": 40}).caption_max_new_tokens == 40


def test_describe_image_refuses_bad_arguments_before_the_model_runs():
    from omniparser_amd.util import utils as U
    from PIL import Image
    calls = []
    model = types.SimpleNamespace(resolution=64, generate=lambda **k: calls.append(k))
    cmp_ = {"model": model, "processor": None}
    img = Image.new("RGB", (32, 24))
    for bad in (0, True, 2.5):
        with pytest.raises(ValueError):
            U.describe_image(img, cmp_, max_new_tokens=bad)
    with pytest.raises(ValueError):
        U.describe_image(img, cmp_, task=7)
    assert calls == []


def test_header_documents_when_each_form_launches():
    from pathlib import Path
    hdr = (Path(__file__).resolve().parents[1] / "include" / "omni_amd.h").read_text()
    assert "attn_decode_self_kernel" in hdr and "greedy_step_long_kernel" in hdr
    assert "#define OMNI_ABI_VERSION 3" in hdr

"""`-m gpu`: Florence-2 captioner kernels and the whole caption / end-to-end path vs CPU references."""
import pytest

from omniparser_amd import _lib as L

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", [L.F32, L.F16])
def test_caption_kernels_vs_interpreter(dtype):
    import gpu_checks as G
    G.check_caption_ops(dtype)


def test_caption_kernels_vs_f64_benched_shapes():
    """Every caption-op signature of the captioner's plans at the benched 768x768 crops (2 crops; tests/caption_f64.py::GPU_TIER, kept
    in step with the plans by test_caption_bounds_cpu.py), O(1) and adversarial inputs (sharp softmax, LayerNorm rows at mean 1e3),
    against float64 references per token / head segment, inside NaN guard bands."""
    import caption_f64 as CF
    worst = CF.check_caption_f64(L.F32, tier="gpu")
    print({k: (f"{v[0]:.2e}", v[2], v[3]) for k, v in worst.items()})


@pytest.mark.parametrize("dtype", [L.F32, L.F16])
def test_caption_kernels_vs_f64_every_branch(dtype):
    """the emulated tier's cases (every launcher branch, window heads 1-32, channel groups 4-32) on the MI355X itself."""
    import caption_f64 as CF
    worst = CF.check_caption_f64(dtype, tier="emu")
    print({k: (f"{v[0]:.2e}", v[2], v[3]) for k, v in worst.items()})


def test_captioner_token_exact_r64():
    """reference cuda-branch shape (64x64 crops, 5 image tokens): greedy ids == transformers CPU."""
    import gpu_checks as G
    out, _ = G.check_captioner(R=64, n=5)
    assert out["ids_equal"], out
    assert out["feat_rel_err"] < 1e-4 and out["enc_rel_err"] < 1e-4
    assert out["max_logit_err"] < out["min_top1_top2_margin"], out
    print(out)


def test_captioner_token_exact_r768():
    """reference CPU-branch shape (768x768 crops, 577 image tokens) — the parity target."""
    import gpu_checks as G
    out, _ = G.check_captioner(R=768, n=2)
    assert out["ids_equal"], out
    assert out["feat_rel_err"] < 3e-4 and out["enc_rel_err"] < 3e-4
    assert out["max_logit_err"] < out["min_top1_top2_margin"], out      # token-exactness is not a coin flip: error below the smallest arg-max margin
    print(out)


def test_omniparser_facade_parse_roundtrip():
    """ref:util/omniparser.py contract: Omniparser(config).parse(base64) -> (base64 PNG, element list)."""
    import base64
    import io
    from PIL import Image
    from omniparser_amd.synth import synthetic_ocr, synthetic_screenshot
    from omniparser_amd.util.omniparser import Omniparser
    from tools.make_weights import ensure_blob, ensure_caption_checkpoint
    import os
    os.environ["OMNI_CAPTION_RES"] = "64"
    try:
        cfg = {"som_model_path": str(ensure_blob(seed=0, nc=1, width=0.5)), "caption_model_name": "florence2",
               "caption_model_path": str(ensure_caption_checkpoint(0)), "BOX_TRESHOLD": 0.05,
               "ocr_provider": lambda image: synthetic_ocr(2, image.size[0], image.size[1], 24)}
        op = Omniparser(cfg)
        buf = io.BytesIO()
        Image.fromarray(synthetic_screenshot(2, 1280, 800)).save(buf, format="PNG")
        png_b64, elems = op.parse(base64.b64encode(buf.getvalue()).decode("ascii"))
    finally:
        os.environ.pop("OMNI_CAPTION_RES", None)
    img = Image.open(io.BytesIO(base64.b64decode(png_b64)))
    assert img.size == (1280, 800)
    assert len(elems) > 10
    for e in elems:
        assert set(e) == {"type", "bbox", "interactivity", "content", "source"}
        assert e["type"] in ("text", "icon") and len(e["bbox"]) == 4 and isinstance(e["content"], str)
        assert all(0.0 <= v <= 1.0 for v in e["bbox"])
    assert any(e["source"] == "box_yolo_content_yolo" for e in elems) and any(e["type"] == "text" for e in elems)


def test_plan_capacity_invariance_r768():
    """The same 16 real crops through an 8-row plan and through the 128-row plan bench.py uses (60 GB of activations, tensors
    beyond 2^31 elements, 18 k-tile GEMM launches): every stage output, the encoder output, the first free logits and the ids of
    a crop must not depend on the plan capacity or on the crop's row."""
    import gpu_checks as G
    out, _ = G.check_plan_capacity(R=768, n=16, small=8, large=128)
    print(out)
    assert out["x_in"]["bitwise"], out
    assert out["ids_equal"], out
    # default composition (Florence2Captioner.reuse_activations): the buffers of stages 0-2 are re-used by later tensors, their taps do not
    # exist; `check_plan_capacity(..., all_taps=True)` builds the plans without reuse to bisect a failure stage by stage
    assert "stage3" in out and "stage0" not in out, list(out)
    for k in ("stage3", "img_feat", "enc_out"):
        assert out[k]["rel"] <= 1e-5, (k, out)
    assert out["logits1"]["max_abs"] <= 1e-4, out


def test_captioner_real_crops_token_exact_r768():
    """randn-free twin of test_captioner_token_exact_r768: up-sampled screenshot crops (what the reference feeds Florence-2) in the
    last rows of a 128-row plan vs transformers on the CPU."""
    import gpu_checks as G
    out, _ = G.check_captioner_real_crops(R=768, n=4, capacity=128)
    print(out)
    assert out["x_in_bitwise"], out
    assert out["ids_equal"], out
    assert out["feat_rel_err"] < 3e-4 and out["enc_rel_err"] < 3e-4, out
    assert out["logit1_max_err"] < 0.1 * out["logit1_min_margin"], out


def test_captioner_f16_token_match_rate_r64():
    """OMNI_PRECISION=f16 at 64x64 crops = the precision class of the reference's OWN cuda branch (ref:util/utils.py:120-121: fp16 weights,
    do_resize=False).  Not the parity mode: greedy decoding amplifies a first differing token, so the class is stated as a RATE — the
    fraction of token positions equal to the fp32 CPU oracle's — and the encoder output within f16 accuracy; printed, with a floor."""
    import gpu_checks as G
    out, _ = G.check_captioner(R=64, n=16, precision="f16")
    print({k: out[k] for k in ("tokens_match", "feat_rel_err", "enc_rel_err", "ids_equal")})
    assert out["enc_rel_err"] < 5e-2, out
    assert out["tokens_match"] >= 0.8, out          # measured 0.985 on the MI355X (profiles/r5_s3_f16_rate.txt); a broken f16 path scores < 0.2


def test_exact_row_encode_twin_r768():
    """Round 6: the remainder micro-batch of a merged caption batch encodes exactly its rows as a second hipGraph in the buffers of the
    full-capacity plan set (florence.py::_CaptionPlans.encode_rows).  24 rows of a 32-row plan set at 768x768: features, encoder output
    and every layer's cross-attention K / V equal the full plan's on those rows (capacity-invariance bar), the full plan is unharmed
    afterwards, the twin is cached.  (The benched 89-of-128 case is covered token for token by test_gpu_z_bench_path.py.)"""
    import gpu_checks as G
    out, _ = G.check_exact_rows(R=768, n=24, capacity=32)
    print(out)
    assert out["twin_cached"] and out["builds"] == 1 and out["twin_ops"] == out["full_ops"]
    for k, v in out.items():
        if isinstance(v, dict):
            assert v["rel"] <= 1e-5 and v["full_again_bitwise"], (k, out)

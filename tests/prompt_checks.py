"""Prompt-conditioned captioning: helpers shared by tests/test_prompt_emu_cpu.py (host emulation of the kernels) and
tests/test_gpu_m_prompt.py (the MI355X).  The oracle is transformers' Florence-2 on the CPU over `shared_random_captioner`, never
the product's own code; the kernel references are float64 restatements with the mask applied as -inf before the softmax.

PROMPTS: the non-default prompts the end-to-end tests use, `[bos] + random ids in 4..49999 + [eos]` drawn from
torch.Generator().manual_seed(1234) in the order of PROMPT_LENGTHS.  The token-exactness rule is the project's own
(gpu_checks.CaptionTally, CAPTION_MARGIN = 2e-4 and the f64 referee) with one condition on top: NO compared crop may need the
referee — every test asserts that the oracle's smallest arg-max margin over all its rows and free steps is >= CAPTION_MARGIN, so a
masking bug cannot hide behind a below-margin excuse.  ORACLE_MARGINS records what the oracle gave when the prompts were chosen."""
import numpy as np
import torch

from omniparser_amd import _lib as L
from omniparser_amd.florence import CLIP_MEAN, CLIP_STD, PROMPT_IDS

BOS, PAD, EOS = 0, 1, 2
PROMPT_LENGTHS = (8, 11, 29, 64, 5, 16, 33, 40)      # total tokens, bos and eos included; drawn in this order from one generator


def _draw_prompts():
    g = torch.Generator().manual_seed(1234)
    return {n: [BOS] + torch.randint(4, 50000, (n - 2,), generator=g).tolist() + [EOS] for n in PROMPT_LENGTHS}


PROMPTS = _draw_prompts()

# what the oracle's scan gave for the prompts above (16 real crops of seed 0 at R = 64, 4 at R = 768, 20 new tokens, greedy):
# smallest top-1 / top-2 margin of the processed scores over all rows and free steps.  The tests re-measure and assert >= 2e-4.
ORACLE_MARGINS = {
    ("uniform", 64): {8: 5.4e-4, 11: 3.7e-3, 29: 2.6e-3, 64: 6.0e-4, 5: 3.0e-3, 16: 2.3e-4, 33: 4.6e-4, 40: 1.3e-3},     # default prompt: 2.8e-4
    ("ragged16", 64): 4.6e-4,                                                  # RAGGED_LENGTHS; the oracle's ragged rows equal their solo runs, 16 of 16
    ("uniform", 768): {11: 6.9e-3, 29: 7.2e-4, 64: 9.3e-4, 40: 1.3e-4},        # default prompt: 3.0e-3.  Length 40 is below 2e-4: NOT used at 768
}


def real_pixels(R, n, seed=0):
    """(pixel_values [n,3,R,R] f32 of the oracle's crop pre-processing, the screenshot u8 [H,W,3], the crop boxes): the n rectangles
    of gpu_checks.real_crop_boxes on synthetic_screenshot(seed), as in gpu_checks.check_captioner_real_crops"""
    import gpu_checks as G
    from oracle import preprocess_ref as PR
    from omniparser_amd.synth import synthetic_screenshot
    img = synthetic_screenshot(seed, 1920, 1080)
    boxes = G.real_crop_boxes(seed, n)
    pv = np.stack([PR.caption_pixel_values(img, b, R, CLIP_MEAN, CLIP_STD) for b in boxes])
    return torch.from_numpy(pv).permute(0, 3, 1, 2).contiguous(), img, boxes


def hf_inputs(model, R, rows):
    """transformers' inputs for one prompt per image: image placeholders + the rows right-padded with <pad>, and the attention mask"""
    n_img = (R // 32) ** 2 + 1
    T = max(len(r) for r in rows)
    ids = torch.tensor([[model.config.image_token_id] * n_img + list(r) + [PAD] * (T - len(r)) for r in rows])
    mask = torch.tensor([[1] * (n_img + len(r)) + [0] * (T - len(r)) for r in rows])
    return ids, mask


def oracle_generate(model, pix, rows, max_new=20, num_beams=1, **kw):
    """transformers.generate on the CPU with one prompt per image.  Returns (sequences, per-row smallest arg-max margin).  Greedy:
    the margin is the top-1 / top-2 difference of the processed scores (n-gram ban applied: what the arg-max is taken over) over
    the free steps of a row (not the forced bos / eos step, not after the row's eos).  Beam search: no margin (None)."""
    ids, mask = hf_inputs(model, pix.shape[-1], rows)
    with torch.inference_mode():
        out = model.generate(input_ids=ids, attention_mask=mask, pixel_values=pix, max_new_tokens=max_new, num_beams=num_beams,
                             do_sample=False, output_scores=num_beams == 1, return_dict_in_generate=True, **kw)
    if num_beams > 1:
        return out.sequences, None
    seq = out.sequences
    n = seq.shape[0]
    margins = [float("inf")] * n
    for t, sc in enumerate(out.scores):
        if t == 0 or t == max_new - 1:                      # forced bos / forced eos
            continue
        top2 = sc.float().topk(2, dim=1).values
        for b in range(n):
            if (seq[b, 1:t + 1] == EOS).any():               # the row has finished: it emits pad from here on
                continue
            margins[b] = min(margins[b], float(top2[b, 0] - top2[b, 1]))
    return seq, margins


def tally_rows(model, R, got, ref, margins, tag, pad=PAD):
    """gpu_checks.CaptionTally over the rows (no image is handed over: a crop below the margin that differs stays unresolved,
    i.e. fails — the callers assert the margins first, so the referee is never needed)"""
    import gpu_checks as G
    tally = G.CaptionTally(model, R, pad=pad)
    for b in range(ref.shape[0]):
        tally.add(f"{tag}[{b}]", got[b], ref[b], margins[b])
    stats, problems = tally.finish()
    assert stats["below_margin"] == 0, stats
    assert not problems, problems
    return stats


def assert_margins(margins, tag):
    import gpu_checks as G
    print(f"[prompt] oracle margins {tag}: min {min(margins):.3e}", flush=True)
    assert min(margins) >= G.CAPTION_MARGIN, (tag, min(margins), "pick another prompt: the oracle itself is within its rounding here")


# ------------------------------------------------------------------------------------------ float64 kernel references
def attn_rows_masked_f64(q, k, v, heads, scale, nkeys):
    """OMNI_OP_ATTN_ROWS mode 0 with a per-group key count: q / k / v [G, n, heads * D] -> [G, n, heads * D] in float64; keys at or
    beyond nkeys[g] get -inf before the softmax (transformers adds finfo.min there: the same zero weight)"""
    G_, nq, C = q.shape
    nk, D = k.shape[1], C // heads
    qh, kh, vh = (t.double().reshape(G_, -1, heads, D).transpose(1, 2) for t in (q, k, v))
    s = qh @ kh.transpose(-2, -1) * scale
    dead = torch.arange(nk)[None, :] >= torch.as_tensor(nkeys)[:, None]
    s = s.masked_fill(dead[:, None, None, :], float("-inf"))
    return (torch.softmax(s, -1) @ vh).transpose(1, 2).reshape(G_, nq, C)


def attn_decode_cross_masked_f64(q, kv, heads, scale, nkeys, kv_div=1):
    """OMNI_OP_ATTN_DECODE cross mode: q [B, C], kv [B / kv_div, S, 2 C] (k | v) -> [B, C] in float64; row b reads cache row
    b // kv_div and its first nkeys[b // kv_div] keys"""
    B, C = q.shape
    D = C // heads
    idx = torch.arange(B) // kv_div
    k, v = kv[idx, :, :C].double(), kv[idx, :, C:].double()
    S = k.shape[1]
    qh = q.double().view(B, heads, 1, D)
    kh, vh = (t.view(B, S, heads, D).transpose(1, 2) for t in (k, v))
    s = qh @ kh.transpose(-2, -1) * scale
    dead = torch.arange(S)[None, :] >= torch.as_tensor(nkeys)[idx][:, None]
    s = s.masked_fill(dead[:, None, None, :], float("-inf"))
    return (torch.softmax(s, -1) @ vh).transpose(1, 2).reshape(B, C)


def ragged_counts(n_img, n_txt, groups, tile):
    """key counts for `groups` groups of a plan with n_img image rows and text capacity n_txt: the shortest possible prompt, a
    count on a key-tile boundary of the kernel (multiple of `tile`) when one lies in range, the full count, and counts between"""
    S = n_img + n_txt
    want = [n_img + 1, S]
    edge = [c for c in range(n_img + 1, S + 1) if c % tile == 0]
    if edge:
        want.append(edge[0])
    g = torch.Generator().manual_seed(S)
    while len(want) < groups:
        want.append(int(torch.randint(n_img + 1, S + 1, (1,), generator=g)))
    return want[:groups]


# ------------------------------------------------------------------------------------------ kernel checks (emulation and MI355X)
def _dev():
    import gpu_checks as G
    return G.DEV


def _sync():
    import gpu_checks as G
    G._sync()


def check_assemble_gather(dtype=L.F32, B=3, n_img=5, n_txt=16, C=96, V=301, scale=27.7128):
    """OMNI_OP_ASSEMBLE with ids: y[b, n_img + t] = table[ids[b][t]] * scale, the image rows copied: bitwise against
    torch.nn.functional.embedding * scale in the plan dtype's f32 arithmetic"""
    tdt = torch.float32 if dtype == L.F32 else torch.float16
    g = torch.Generator().manual_seed(5)
    table = torch.randn(V, C, generator=g).to(tdt)
    img = torch.randn(B, n_img, C, generator=g).to(tdt)
    ids = torch.randint(0, V, (B, n_txt), generator=g, dtype=torch.int32)
    ids[0, 0], ids[-1, -1] = 0, V - 1                                  # first and last row of the table
    dev = _dev()
    d = {k: v.to(dev) for k, v in {"table": table, "img": img, "ids": ids, "y": torch.zeros(B, n_img + n_txt, C, dtype=tdt)}.items()}
    L.launch(L.make_op(L.OP_ASSEMBLE, dtype, p=[d["img"].data_ptr(), None, d["ids"].data_ptr(), d["table"].data_ptr(), d["y"].data_ptr()],
                       i={0: B, 1: n_img, 2: n_txt, 3: C, 4: V}, f={0: scale}))
    _sync()
    y = d["y"].cpu()
    want = (torch.nn.functional.embedding(ids.long(), table.float()) * scale).to(tdt)
    assert torch.equal(y[:, :n_img], img), "image rows are copied"
    assert torch.equal(y[:, n_img:], want), "gathered rows differ from embedding * scale"


def _attn_rows_op(dtype, d, heads, D, S, groups, nkeys):
    C = heads * D
    return L.make_op(L.OP_ATTN_ROWS, dtype, p=[d["qkv"].data_ptr(), d["qkv"].data_ptr(), d["qkv"].data_ptr(), None, d["o"].data_ptr()]
                     + ([None, None, nkeys.data_ptr()] if nkeys is not None else []),
                     i={0: 3 * C, 1: 3 * C, 2: 3 * C, 3: C, 4: 0, 5: C, 6: 2 * C, 7: 0, 8: heads, 9: S, 10: S, 11: groups, 12: 0, 15: D},
                     f={0: D ** -0.5})


def check_attn_rows_masked(dtype, D, heads, n_img, n_txt, groups, tile):
    """OMNI_OP_ATTN_ROWS mode 0 with the per-group key table (D = 32: attn_rows_kernel; D = 64: mha_mfma_f32_kernel on f32 plans,
    mha_mfma_kernel on f16 plans) against the f64 reference inside caption_f64.bound("attention", dtype).  The rows behind a
    group's count hold LARGE keys and values (they would dominate the softmax if they had any weight); as queries they must come
    out finite.  Also: a table that says `full` for every group gives the bits of the launch without a table."""
    import caption_f64 as CF
    tdt = torch.float32 if dtype == L.F32 else torch.float16
    S, C = n_img + n_txt, heads * D
    counts = ragged_counts(n_img, n_txt, groups, tile)
    g = torch.Generator().manual_seed(100 + S + D)
    qkv = torch.randn(groups, S, 3 * C, generator=g)
    for gi, c in enumerate(counts):
        qkv[gi, c:, C:] *= 40.0
    qkv = qkv.to(tdt)
    dev = _dev()
    d = {"qkv": qkv.to(dev), "o": torch.full((groups, S, C), float("nan"), dtype=tdt).to(dev)}
    nk = torch.tensor(counts, dtype=torch.int32).to(dev)
    L.launch(_attn_rows_op(dtype, d, heads, D, S, groups, nk))
    _sync()
    o = d["o"].cpu()
    ref = attn_rows_masked_f64(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], heads, D ** -0.5, counts)
    worst = 0.0
    for gi, c in enumerate(counts):
        e, _ = CF.seg_err(o[gi, :c], ref[gi, :c], D)
        worst = max(worst, e)
        assert bool(torch.isfinite(o[gi, c:].float()).all()), f"padded query rows of group {gi} (count {c}) are not finite"
    print(f"[prompt] attn_rows masked dtype={dtype} D={D} S={S} counts={counts}: worst segment error {worst:.3e}", flush=True)
    assert worst <= CF.bound("attention", dtype), (worst, CF.bound("attention", dtype), counts)
    # bit-identity across padding: table = [full] * groups vs no table
    outs = []
    for table in (None, torch.full((groups,), S, dtype=torch.int32).to(dev)):
        d["o"].fill_(float("nan"))
        L.launch(_attn_rows_op(dtype, d, heads, D, S, groups, table))
        _sync()
        outs.append(d["o"].cpu())
    assert torch.equal(outs[0].view(torch.int32 if dtype == L.F32 else torch.int16),
                       outs[1].view(torch.int32 if dtype == L.F32 else torch.int16)), "a full table changes bits"
    return worst


def check_attn_decode_cross_masked(dtype, heads, n_img, n_txt, crops, kv_div=1, aligned=True):
    """OMNI_OP_ATTN_DECODE cross mode with the per-row key table: attn_decode_cross_kernel (f32 plans, 16-byte aligned pitches) or the
    generic path of attn_decode_body (f16 plans, or an unaligned cache pitch), with and without beam rows (i12 = kv_div), against
    the f64 reference inside caption_f64.bound("attn_decode", dtype); a full table gives the bits of the launch without one."""
    import caption_f64 as CF
    tdt = torch.float32 if dtype == L.F32 else torch.float16
    esz = 4 if dtype == L.F32 else 2
    S, C = n_img + n_txt, heads * 64
    ldc = 2 * C + (0 if aligned else 2)
    B = crops * kv_div
    counts = ragged_counts(n_img, n_txt, crops, 32)
    g = torch.Generator().manual_seed(200 + S)
    kv = torch.randn(crops, S, ldc, generator=g)
    for ci, c in enumerate(counts):
        kv[ci, c:] *= 40.0
    kv = kv.to(tdt)
    q = torch.randn(B, C, generator=g).to(tdt)
    dev = _dev()
    d = {"q": q.to(dev), "kv": kv.to(dev), "o": torch.full((B, C), float("nan"), dtype=tdt).to(dev)}

    def run(table):
        d["o"].fill_(float("nan"))
        L.launch(L.make_op(L.OP_ATTN_DECODE, dtype,
                           p=[d["q"].data_ptr(), None, None, d["kv"].data_ptr(), d["o"].data_ptr(), d["kv"].data_ptr() + C * esz, None]
                           + ([table.data_ptr()] if table is not None else []),
                           i={0: C, 1: 0, 5: C, 6: heads, 7: S, 8: S, 9: C, 10: B, 11: ldc, **({12: kv_div} if kv_div > 1 else {})},
                           f={0: 0.125}))
        _sync()
        return d["o"].cpu()
    o = run(torch.tensor(counts, dtype=torch.int32).to(dev))
    ref = attn_decode_cross_masked_f64(q, kv[..., :2 * C], heads, 0.125, counts, kv_div)
    e, _ = CF.seg_err(o, ref, 64)
    print(f"[prompt] attn_decode cross masked dtype={dtype} S={S} kv_div={kv_div} aligned={aligned} counts={counts}: {e:.3e}", flush=True)
    assert e <= CF.bound("attn_decode", dtype), (e, CF.bound("attn_decode", dtype), counts)
    a, b = run(None), run(torch.full((crops,), S, dtype=torch.int32).to(dev))
    it = torch.int32 if dtype == L.F32 else torch.int16
    assert torch.equal(a.view(it), b.view(it)), "a full table changes bits"
    return e


# ------------------------------------------------------------------------------------------ end-to-end cases of the MI355X tests
UNIFORM_CASES = {64: (16, (11, 29)), 768: (4, (11, 64))}       # R -> (real crops of seed 0, prompt lengths: two different capacities)
RAGGED_LENGTHS = (5, 8, 11, 16, 29, 33, 40, 64, 64, 40, 33, 29, 16, 11, 8, 5)     # a batch of 16 at R = 64: every capacity, both ends


def ragged_rows():
    return [PROMPTS[n] for n in RAGGED_LENGTHS]


def check_uniform_prompts(R, max_new=20):
    """generate(input_ids=...) with a non-default prompt for all rows, on real crops, token-exact against transformers (CaptionTally,
    no crop below the margin); two prompts of different text capacities; the prompt must change the oracle's captions"""
    from omniparser_amd.florence import Florence2Captioner, text_capacity
    from tools.make_weights import ensure_caption_checkpoint, shared_random_captioner
    n, lengths = UNIFORM_CASES[R]
    model = shared_random_captioner(0)
    pix, _, _ = real_pixels(R, n)
    cap = Florence2Captioner(ensure_caption_checkpoint(0), "cuda", precision="f32", resolution=R)
    dflt, _ = oracle_generate(model, pix, [PROMPT_IDS] * n, max_new)
    out = {}
    for ln in lengths:
        rows = [PROMPTS[ln]] * n
        ref, margins = oracle_generate(model, pix, rows, max_new)
        assert_margins(margins, f"uniform {ln} @{R}")
        T = min(ref.shape[1], dflt.shape[1])
        changed = sum(ref[b, :T].tolist() != dflt[b, :T].tolist() or ref.shape[1] != dflt.shape[1] for b in range(n))
        assert changed == n, f"the oracle's captions change on {changed} of {n} crops only"
        ids, _ = hf_inputs(model, R, rows)
        got = cap.generate(input_ids=ids, pixel_values=pix.to(_dev()), max_new_tokens=max_new)
        stats = tally_rows(model, R, got, ref, margins, f"uniform{ln}@{R}")
        assert any(k[-1] == ("txt", text_capacity(ln)) for k in cap._plans), list(cap._plans)
        out[ln] = (min(margins), stats["caption_crops_compared"])
    return out, cap


def check_ragged_batch(max_new=20):
    """a ragged batch of 16 prompts (5 .. 64 tokens, attention mask) at R = 64: token-exact against transformers, and every row
    equal to the same prompt run alone on the plan of its own capacity"""
    from omniparser_amd.florence import Florence2Captioner
    from tools.make_weights import ensure_caption_checkpoint, shared_random_captioner
    R, rows = 64, ragged_rows()
    n = len(rows)
    model = shared_random_captioner(0)
    pix, _, _ = real_pixels(R, n)
    ref, margins = oracle_generate(model, pix, rows, max_new)
    assert_margins(margins, "ragged 16 @64")
    cap = Florence2Captioner(ensure_caption_checkpoint(0), "cuda", precision="f32", resolution=R)
    ids, mask = hf_inputs(model, R, rows)
    pd = pix.to(_dev())
    got = cap.generate(input_ids=ids, attention_mask=mask, pixel_values=pd, max_new_tokens=max_new)
    tally_rows(model, R, got, ref, margins, "ragged16")
    for b, r in enumerate(rows):
        i1, _ = hf_inputs(model, R, [r])
        solo = cap.generate(input_ids=i1, pixel_values=pd[b:b + 1], max_new_tokens=max_new)
        assert _trim(solo[0]) == _trim(got[b]), (b, len(r), solo[0].tolist(), got[b].tolist())
    return {"min_margin": min(margins), "rows": n}, cap


def _trim(row, pad=PAD):
    row = [int(v) for v in row.tolist()]
    while row and row[-1] == pad:
        row.pop()
    return row

"""Target-score checks shared by the CPU (emulation) and GPU tests of the target-score form of OMNI_OP_GREEDY_STEP (p5) and of
Florence2Captioner.score / score_crops / rank_elements: the kernel against an f64 log-softmax of the raw logits (+ bias), the
captioner against transformers' teacher-forced forward pass on the CPU.

Bound of the kernel check (`kernel_bound`; absolute, per row; derived for the ONE-PASS algorithm, not tuned).  u = 2^-24 is the f32
unit round-off, D = ulp_f32(max |x|) over the row's finite entries, N the elements per 16-byte load (4 for f32, 8 for f16 logits) and
G = ceil(V / (256 N)) + 2 the most calls of the per-thread update (the vector loop plus the peeled head and tail).  The kernel returns
(x_t - m) - log(s), where s is the rescaled sum the row's terms reach through one thread, six shuffle levels and three LDS merges.
  * inputs: every x_v = f32(logit) + bias is one rounding (<= D / 2) of what the f64 reference adds exactly; that moves log(sum) by
    at most D / 2 and x_t by at most D / 2: D.
  * exponents of the rescaled sum: a term enters as exp(x - m) — one rounding of x - m, <= ulp_f32(2 max |x|) / 2 <= D — and is then
    multiplied by exp(m_old - m_new) whenever the running maximum moves, in the thread and in the merges.  Along one term's path the
    maximum only grows, so the differences sum to at most 2 max |x|, and their roundings (each half an ulp of its OWN size, i.e.
    <= u times it) to at most 2 u max |x| <= 2 D, however many rescales there are.  Exponent errors are relative errors of the term: 3 D.
  * relative errors of the sum's arithmetic: per update call at most one rescale (expf at <= 2 ulp = 4 u, one multiplication u) and N
    additions (u each): G (N + 5) u; the term's own expf 4 u; nine merges of two expf, a multiplication and an addition: 9 * 6 u.
    All terms are positive, so the relative error of s is at most the largest along a path, and log(s) moves by that much (a factor
    1.01 covers the second order): 1.01 (3 D + (G (N + 5) + 58) u).
  * the result: x_t - m is one rounding (<= D), logf at <= 2 ulp of a value <= ln V, and the final subtraction half an ulp of a
    value <= 2 max |x| + ln V.
V = 51289, |x| < 32: f32 logits G = 53, 4.8e-5; f16 logits G = 28, 4.1e-5.  Model tolerance: TOL_TARGET_LOGP below."""
import math

import torch

import score_checks as SC

START, PAD, EOS, BOS = SC.START, SC.PAD, SC.EOS, SC.BOS
ulp_f32 = SC.ulp_f32
LOGP_FILL, TOP1_FILL = 7.5, -7                   # what the untouched entries of p4 / p7 hold in the kernel check

# |token_logprobs - transformers| of Florence2Captioner.score (f32 plans, 64x64 crops, stand-in checkpoint, every label position):
# largest value measured on the host emulation and on the MI355X (profiles/target_scores_tolerance.json), times
# the project's factor 5.  The oracle side is transformers on the CPU.
MEASURED_MAX_DLOGP = {"emulation": 1.686e-05, "mi355x": 2.824e-05}
TOL_TARGET_LOGP = 5.0 * max(MEASURED_MAX_DLOGP.values())


def kernel_bound(V, f16, max_abs_x):
    """see the module docstring"""
    u, N = 2.0 ** -24, (8 if f16 else 4)
    G = math.ceil(V / (256 * N)) + 2
    D = ulp_f32(max_abs_x)
    lnV = math.log(V)
    return (D + 1.01 * (3 * D + (G * (N + 5) + 58) * u) + D + 2 * ulp_f32(lnV) + 0.5 * ulp_f32(2 * max_abs_x + lnV))


def target_lengths(B, T):
    """tlen per row: every of 0, 1, mid, T - 1 occurs among six rows"""
    mid = max(1, (T - 1) // 2)
    return torch.tensor([(T - 1, 1, mid, T - 1, 0, mid)[b % 6] for b in range(B)], dtype=torch.int32)


def scripted_case(B, V, steps, seed, tdt, with_bias):
    """scripted seeded logits per step (score_checks.scripted_logits), random targets, and the special rows: b % 6 == 0 the target is
    the row's maximum, 1 its minimum, 2 the target's logit is -inf, 3 the leading 2100 (or V / 2) entries are -inf — so that every
    thread's first loads, the peeled head included, see nothing but -inf"""
    g = torch.Generator().manual_seed(seed + 7)
    seq = SC.scripted_logits(B, V, steps, seed, tdt)
    bias = torch.randn(V, generator=torch.Generator().manual_seed(seed + 1)) * 0.5 if with_bias else None
    T = steps + 1
    ids = torch.randint(0, V, (B, T), generator=g, dtype=torch.int32)
    ids[:, 0] = START
    lead = min(V // 2, 2100)
    for t, x in enumerate(seq):
        for b in range(B):
            if b % 6 == 3:
                x[b, :lead] = float("-inf")
            full = x[b].double() + (bias.double() if bias is not None else 0.0)
            if b % 6 == 0:
                ids[b, t + 1] = int(full.argmax())
            elif b % 6 == 1:
                ids[b, t + 1] = int(full.argmin())
            elif b % 6 == 2:
                x[b, int(ids[b, t + 1])] = float("-inf")
    return seq, bias, ids


def score_op(L, dtype, logits, bias, ids, step, logp, tlen, top1, B, V, T, fin=None, ngram=3, fbos=BOS, feos=EOS):
    """the target-score form; the processors' slots hold what a generation plan would put there: they must be ignored"""
    ptr = lambda t: t.data_ptr() if t is not None else None
    return L.make_op(L.OP_GREEDY_STEP, dtype, p=[ptr(logits), ptr(bias), ptr(ids), ptr(fin), ptr(logp), ptr(tlen), ptr(step), ptr(top1)],
                     i={0: B, 1: V, 2: V, 3: T, 4: T - 1, 5: ngram, 6: BOS, 7: EOS, 8: PAD, 9: fbos, 10: feos, 11: 1})


def run_scores(L, dev, seq, bias, ids, tlen, dtype, with_top1=True, sync=lambda: None):
    """`len(seq)` launches of the op on the scripted logits -> host (ids, step, logp, top1 or None); logp / top1 start as the
    fill values"""
    B, V = seq[0].shape
    T = ids.shape[1]
    d_ids, d_tlen, d_step = ids.to(dev), tlen.to(dev), torch.zeros(1, dtype=torch.int32, device=dev)
    d_logp = torch.full((B, T), LOGP_FILL, dtype=torch.float32, device=dev)
    d_top1 = torch.full((B, T), TOP1_FILL, dtype=torch.int32, device=dev) if with_top1 else None
    d_bias = bias.to(dev) if bias is not None else None
    d_logits = torch.empty_like(seq[0], device=dev)
    op = score_op(L, dtype, d_logits, d_bias, d_ids, d_step, d_logp, d_tlen, d_top1, B, V, T)
    for x in seq:
        d_logits.copy_(x)
        L.launch(op)
        sync()
    return d_ids.cpu(), d_step.cpu(), d_logp.cpu(), (d_top1.cpu() if with_top1 else None)


def check_kernel_case(L, dev, B, V, steps, with_bias, f16, seed, sync=lambda: None):
    """One case of the kernel check: see the module docstring for the bound.  Returns {max_err, max_bound_ratio, scored, top1_checked,
    neg_inf_targets} and asserts everything else."""
    dtype, tdt = (L.F16, torch.float16) if f16 else (L.F32, torch.float32)
    seq, bias, ids = scripted_case(B, V, steps, seed, tdt, with_bias)
    T = steps + 1
    tlen = target_lengths(B, T)
    got_ids, step, logp, top1 = run_scores(L, dev, seq, bias, ids, tlen, dtype, True, sync)
    assert torch.equal(got_ids, ids), "the target-score form wrote ids"
    assert int(step[0]) == steps
    _, _, logp_only, _ = run_scores(L, dev, seq, bias, ids, tlen, dtype, False, sync)          # p7 = NULL: the same log-probabilities
    assert torch.equal(torch.nan_to_num(logp_only, nan=-1.0), torch.nan_to_num(logp, nan=-1.0))
    worst, ratio, scored, top1_checked, neg_inf = 0.0, 0.0, 0, 0, 0
    assert bool((logp[:, 0] == LOGP_FILL).all()) and bool((top1[:, 0] == TOP1_FILL).all()), "column 0 was written"
    for t in range(steps):
        full = seq[t].double() + (bias.double() if bias is not None else 0.0)
        lsm = torch.log_softmax(full, dim=-1)
        for b in range(B):
            got, g1 = float(logp[b, t + 1]), int(top1[b, t + 1])
            if t + 1 > int(tlen[b]):
                assert got == LOGP_FILL and g1 == TOP1_FILL, f"row {b} position {t + 1} behind tlen {int(tlen[b])} was written"
                continue
            tok = int(ids[b, t + 1])
            want = float(lsm[b, tok])
            finite = full[b][torch.isfinite(full[b])]
            bound = kernel_bound(V, f16, float(finite.abs().max()))
            scored += 1
            if want == float("-inf"):
                assert got == float("-inf"), f"row {b} step {t}: a -inf target scored {got}"
                neg_inf += 1
            else:
                err = abs(got - want)
                assert err <= bound, f"row {b} step {t}: logp {got} vs f64 {want}: {err:.3e} > {bound:.3e}"
                worst, ratio = max(worst, err), max(ratio, err / bound)
            top2 = full[b].topk(2).values
            assert 0 <= g1 < V
            if float(top2[0] - top2[1]) > bound:
                assert g1 == int(full[b].argmax()), (b, t, g1, int(full[b].argmax()))
                top1_checked += 1
            if b % 6 == 0:
                assert g1 == tok                          # the target IS the maximum (lifted entries: a gap far above the bound)
    print(f"target scores vs f64: B={B} V={V} steps={steps} bias={with_bias} f16={f16}: max err {worst:.3e} = {ratio:.3f} of the bound, "
          f"{scored} positions, {top1_checked} arg-max checked, {neg_inf} -inf targets")
    assert neg_inf >= 1 and top1_checked >= 1
    return {"max_err": worst, "max_bound_ratio": ratio, "scored": scored, "top1_checked": top1_checked, "neg_inf_targets": neg_inf}


def check_degenerate_rows(L, dev, sync=lambda: None):
    """an all-NaN row and an all -inf row: top1 = 0, the rows next to them get their values, a token outside the vocabulary scores
    -inf; nothing outside 0..V-1 is written"""
    Bq, Vv, T = 4, 1003, 5
    logits = torch.randn(Bq, Vv, generator=torch.Generator().manual_seed(0))
    logits[1] = float("nan")
    logits[2] = float("-inf")
    ids = torch.full((Bq, T), 11, dtype=torch.int32); ids[:, 0] = START
    ids[3, 1] = Vv + 5                                         # out of range
    tlen = torch.tensor([2, 2, 2, 2], dtype=torch.int32)
    got_ids, step, logp, top1 = run_scores(L, dev, [logits], None, ids, tlen, L.F32, True, sync)
    assert torch.equal(got_ids, ids) and int(step[0]) == 1
    new = top1[:, 1].tolist()
    assert new == [int(torch.argmax(logits[0])), 0, 0, int(torch.argmax(logits[3]))], new
    assert abs(float(logp[0, 1]) - float(torch.log_softmax(logits[0].double(), -1)[11])) < 1e-5
    assert math.isnan(float(logp[1, 1])) and float(logp[2, 1]) == float("-inf") and float(logp[3, 1]) == float("-inf")
    assert bool((logp[:, 2:] == LOGP_FILL).all()) and bool((top1[:, 2:] == TOP1_FILL).all())
    return new


def check_argument_errors(L, dev):
    """p5 with p4 = NULL, and p7 without p5: OMNI_E_ARG (an OmniError), nothing launched"""
    B, V, T = 2, 64, 3
    t = {"logits": torch.zeros(B, V, device=dev), "ids": torch.zeros(B, T, dtype=torch.int32, device=dev),
         "step": torch.zeros(1, dtype=torch.int32, device=dev), "logp": torch.zeros(B, T, device=dev),
         "tlen": torch.ones(B, dtype=torch.int32, device=dev), "top1": torch.zeros(B, T, dtype=torch.int32, device=dev)}
    seen = {}
    for name, kw in (("p5_without_p4", {"logp": None}), ("p7_without_p5", {"tlen": None})):
        a = {**t, **kw}
        op = score_op(L, L.F32, a["logits"], None, a["ids"], a["step"], a["logp"], a["tlen"], a["top1"], B, V, T)
        try:
            L.launch(op)
        except L.OmniError as e:
            seen[name] = str(e)
            assert "error -1" in str(e), str(e)                # OMNI_E_ARG
        else:
            raise AssertionError(f"{name} was accepted")
    assert int(t["step"].cpu()[0]) == 0
    return seen


# ---------------------------------------------------------------------------------------------- whole captioner vs transformers
def hf_input_ids(model, n, R):
    from omniparser_amd.florence import PROMPT_IDS
    n_img = (R // 32) ** 2 + 1
    return torch.tensor([[model.config.image_token_id] * n_img + PROMPT_IDS] * n)


def hf_greedy_labels(model, pix, max_new):
    """per crop its own greedy caption as a label: transformers' generate(num_beams=1) without the decoder start token, cut behind
    the first EOS"""
    with torch.inference_mode():
        seq = model.generate(input_ids=hf_input_ids(model, pix.shape[0], pix.shape[-1]), pixel_values=pix, max_new_tokens=max_new,
                             num_beams=1, do_sample=False)
    out = []
    for row in seq.tolist():
        lab = row[1:]
        end = next((p for p, t in enumerate(lab) if t == EOS and p > 0), len(lab) - 1)
        out.append(lab[:end + 1])
    return out


def random_labels(lengths, seed, vocab=50000):
    """[bos, random ids, eos] of the given lengths (length 1: [bos])"""
    g = torch.Generator().manual_seed(seed)
    return [([BOS] + torch.randint(4, vocab, (max(0, n - 2),), generator=g).tolist() + [EOS])[:n] for n in lengths]


def hf_label_logprobs(model, pix, per):
    """the oracle: per image b and label j the f64 gather of Florence2ForConditionalGeneration(input_ids, pixel_values,
    decoder_input_ids=shift_tokens_right(labels)).logits.log_softmax(-1) at the label's tokens, over the label's own length, and the
    arg-max of the same rows -> (logp [n][M] lists of f64 tensors, top1 likewise, top-1 / top-2 gaps likewise)"""
    from transformers.models.bart.modeling_bart import shift_tokens_right
    n, M = len(per), len(per[0])
    cfg = model.config
    start = model.generation_config.decoder_start_token_id
    start = 2 if start is None else start
    logp, top1, gaps = [[None] * M for _ in range(n)], [[None] * M for _ in range(n)], [[None] * M for _ in range(n)]
    inp = hf_input_ids(model, n, pix.shape[-1])
    for j in range(M):
        Lj = max(len(per[b][j]) for b in range(n))
        lab = torch.full((n, Lj), PAD, dtype=torch.long)
        for b in range(n):
            lab[b, :len(per[b][j])] = torch.tensor(per[b][j])
        with torch.inference_mode():
            logits = model(input_ids=inp, pixel_values=pix, decoder_input_ids=shift_tokens_right(lab, PAD, start)).logits
        lsm = torch.log_softmax(logits.double(), dim=-1)
        for b in range(n):
            k = len(per[b][j])
            logp[b][j] = lsm[b, :k].gather(1, lab[b, :k, None])[:, 0]
            top1[b][j] = lsm[b, :k].argmax(-1)
            t2 = lsm[b, :k].topk(2, dim=-1).values
            gaps[b][j] = t2[:, 0] - t2[:, 1]
    return logp, top1, gaps


def compare_scores(out, per, ref_logp, ref_top1, gaps, tol):
    """`score`'s output against the oracle: shapes, lengths, zeros behind each label, |delta logp| <= tol over each label's length;
    top1 equals the oracle's arg-max wherever its top-1 / top-2 gap exceeds 2 tol.  Returns the largest |delta logp|."""
    n, M = len(per), len(per[0])
    Lmax = max(len(r) for rows in per for r in rows)
    assert tuple(out.token_logprobs.shape) == (n, M, Lmax) == tuple(out.top1.shape) and out.token_logprobs.dtype == torch.float32
    assert out.lengths.tolist() == [[len(r) for r in rows] for rows in per]
    worst, failures = 0.0, []
    for b in range(n):
        for j in range(M):
            k = len(per[b][j])
            assert bool((out.token_logprobs[b, j, k:] == 0).all()) and bool((out.top1[b, j, k:] == 0).all())
            d = (out.token_logprobs[b, j, :k].double() - ref_logp[b][j]).abs()
            worst = max(worst, float(d.max()))
            if float(d.max()) > tol:
                failures.append({"image": b, "label": j, "max_dlogp": float(d.max())})
            sure = gaps[b][j] > 2 * tol
            if not torch.equal(out.top1[b, j, :k][sure], ref_top1[b][j][sure]):
                failures.append({"image": b, "label": j, "top1": out.top1[b, j, :k].tolist(), "ref": ref_top1[b][j].tolist()})
    assert not failures, failures[:3]
    return worst


_ORACLE = {}


def captioner_case(n, lengths, seed, greedy_new, R=64):
    """(pixels, per-image labels, oracle log-probs / top1 / gaps) of one case, computed once per process: n seeded RxR crops, label 0
    the crop's own greedy caption (transformers, max_new_tokens=greedy_new), the others random labels of `lengths` shared by all"""
    import beam_checks as BC
    key = (n, tuple(lengths), seed, greedy_new, R)
    if key not in _ORACLE:
        pix = torch.randn(n, 3, R, R, generator=torch.Generator().manual_seed(seed))
        model = BC.oracle_model(0, False)
        own = hf_greedy_labels(model, pix, greedy_new)
        shared = random_labels(lengths, seed + 1)
        per = [[own[b]] + shared for b in range(n)]
        _ORACLE[key] = (pix, per, shared) + hf_label_logprobs(model, pix, per)
    return _ORACLE[key]


def make_captioner(R=64):
    from omniparser_amd.florence import Florence2Captioner
    from tools.make_weights import ensure_caption_checkpoint
    return Florence2Captioner(ensure_caption_checkpoint(0), "cuda", precision="f32", resolution=R)


def captioner_vs_hf(cap, n, lengths, seed, greedy_new, device_pixels=False, tol=None):
    """Florence2Captioner.score against transformers; the largest |delta logp| is printed before it is compared (the measurement
    of TOL_TARGET_LOGP).  Returns (pixels as given to the captioner, per-image labels, shared labels, output, oracle log-probs)."""
    pix, per, shared, ref_logp, ref_top1, gaps = captioner_case(n, lengths, seed, greedy_new)
    px = pix.cuda() if device_pixels else pix
    out = cap.score(px, per)
    worst = compare_scores(out, per, ref_logp, ref_top1, gaps, float("inf"))
    print(f"target scores vs transformers: n={n} M={len(per[0])} label lengths {sorted(set(len(r) for rows in per for r in rows))}: "
          f"max |dlogp| = {worst:.3e}, stats {cap.score_stats}")
    compare_scores(out, per, ref_logp, ref_top1, gaps, TOL_TARGET_LOGP if tol is None else tol)
    return px, per, shared, out, ref_logp


# ---------------------------------------------------------------------------------------------- interface: crops, ranking
# seed 5: the smallest gap between two elements in the oracle's own scores is 3.3e-3 (checked on the CPU, crops from the emulated crop op),
# far above 2 TOL_TARGET_LOGP: the oracle alone has no near tie
FRAME_SEED, FRAME_W, FRAME_H = 5, 1280, 800
QUERY_LENGTHS = (3, 5, 8)


def frame_elements():
    """nine elements of mixed types with ratio bboxes on the synthetic 1280x800 frame; element 4 has an empty crop and is skipped"""
    boxes = [(40, 30, 120, 90), (200, 60, 330, 100), (400, 300, 460, 360), (700, 120, 900, 180), (500, 500, 500, 560),
             (1000, 600, 1100, 700), (60, 640, 260, 700), (880, 40, 940, 100), (620, 420, 700, 470)]
    return [{"type": "text" if k % 3 == 1 else "icon", "bbox": [x0 / FRAME_W, y0 / FRAME_H, x1 / FRAME_W, y1 / FRAME_H],
             "interactivity": k % 3 != 1, "content": f"element {k}", "source": "box_ocr_content_ocr" if k % 3 == 1 else "box_yolo_content_yolo"}
            for k, (x0, y0, x1, y1) in enumerate(boxes)]


def frame_and_queries():
    from omniparser_amd.synth import synthetic_screenshot
    frame = torch.from_numpy(synthetic_screenshot(FRAME_SEED, FRAME_W, FRAME_H))
    return frame, frame_elements(), random_labels(QUERY_LENGTHS, 77)


def crop_pixels(cap, frame, boxes_px):
    """the normalised pixels [n, 3, R, R] the captioner's crop op (OMNI_OP_CROP_RESIZE, tested on its own) makes of the rectangles"""
    n = len(boxes_px)
    cp = cap.plans(cap.bucket(n), cap.resolution, 4)
    rects = torch.tensor(boxes_px, dtype=torch.int32).to(cap.device)
    with torch.cuda.stream(cap.stream):
        cap.launch_crops(cp, 0, n, frame.to(cap.device), rects, *cap.crop_scratch(n, cp.R), cap.stream)
        pix = cp.x_in.t[:n, :, :, :3].permute(0, 3, 1, 2).float().clone()
    cap.stream.synchronize()
    return pix.cpu()


def oracle_ranking(cap, frame, elements, queries, normalize="mean"):
    """transformers' scores of every query on every non-empty crop -> (kept element indices, boxes, pixels, scores f64 [n, M])"""
    import beam_checks as BC
    from omniparser_amd.florence import sequence_score
    from omniparser_amd.util.utils import crop_boxes_px
    index, boxes = [], []
    for k, e in enumerate(elements):
        px = crop_boxes_px([e["bbox"]], frame.shape[1], frame.shape[0])
        if px:
            index.append(k); boxes.append(px[0])
    pix = crop_pixels(cap, frame, boxes)
    per = [list(queries) for _ in index]
    ref_logp, _, _ = hf_label_logprobs(BC.oracle_model(0, False), pix, per)
    Lmax = max(len(q) for q in queries)
    lp = torch.zeros(len(index), len(queries), Lmax, dtype=torch.float64)
    for b in range(len(index)):
        for j, q in enumerate(queries):
            lp[b, j, :len(q)] = ref_logp[b][j]
    lengths = torch.tensor([[len(q) for q in queries]] * len(index))
    scores = sequence_score(lp, lengths, labels=per, normalize=normalize, forced_bos=cap.w.forced_bos)
    return index, boxes, pix, scores, (lp, lengths)


def smallest_oracle_gap(scores):
    """smallest |score difference| between two elements under one query"""
    n = scores.shape[0]
    return min(float((scores[a, j] - scores[b, j]).abs()) for j in range(scores.shape[1]) for a in range(n) for b in range(a + 1, n))


def check_ranking(ranked, index, scores, tol):
    """`rank_elements`' lists against the oracle's scores: all kept elements, each once; a pair of neighbours may stand in the other
    order only where the oracle's gap is below 2 tol, at most one such pair per query; scores within tol"""
    where = {k: b for b, k in enumerate(index)}
    for j, lst in enumerate(ranked):
        assert sorted(r["index"] for r in lst) == sorted(index), (j, lst)
        want = sorted(range(len(index)), key=lambda b: (-float(scores[b, j]), index[b]))
        got = [where[r["index"]] for r in lst]
        swapped = 0
        for a in range(len(got)):
            for b in range(a + 1, len(got)):
                if want.index(got[a]) > want.index(got[b]):
                    assert abs(float(scores[got[a], j] - scores[got[b], j])) < 2 * tol, (j, got, want)
                    swapped += 1
        assert swapped <= 1, (j, got, want)
        for r in lst:
            assert abs(r["score"] - float(scores[where[r["index"]], j])) <= tol, (j, r, float(scores[where[r["index"]], j]))

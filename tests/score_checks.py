"""Token-score checks shared by the CPU (emulation) and GPU tests of OMNI_OP_GREEDY_STEP p4 / Florence2Captioner.generate(
output_scores=True): the kernel against an f64 log-softmax of transformers' processed scores, the captioner against transformers'
generate(output_scores=True) + compute_transition_scores(normalize_logits=True) on the CPU.

Bound of the kernel check (absolute, per row; derived, not tuned): the kernel returns -log(sum_v exp(x_v - max)) in f32.
  * every x_v = f32(logit) + bias and every x_v - max is one f32 rounding of values no larger than max |x|: <= ulp_f32(max |x|) each,
    which moves the term's exponent, hence log(sum), by at most that much — 4 ulp_f32(max |x|) covers both plus the exp / log
    arguments' own rounding;
  * the sum: V / 256 sequential additions per thread, 6 wave-reduction levels, 3 additions across the waves, and the final expf /
    logf at a couple of ulp each, every one a relative error of <= 2^-24 of a sum >= 1 (the maximum's own term is 1), i.e. an
    absolute error of log(sum) of at most 2^-23 (V / 256 + 16) with a factor 2 to spare.
Model tolerance: TOL_LOGP below."""
import math

import torch

import beam_checks as BC
import plan_interp as PI

START, PAD, EOS, BOS = 2, 1, 2, 0
REPEAT_TOKEN = 7

# |token_logprobs - transformers| of the whole captioner (f32 plans, 64x64 crops, stand-in checkpoint, positions up to each row's EOS):
# largest value measured on the host emulation and on the MI355X (profiles/token_scores_tolerance.json), times
# the project's factor 5.  The oracle side is transformers on the CPU.
MEASURED_MAX_DLOGP = {"emulation": 1.287e-05, "mi355x": 1.574e-05}
TOL_LOGP = 5.0 * max(MEASURED_MAX_DLOGP.values())


def ulp_f32(x: float) -> float:
    """spacing of f32 at |x| (normal range)"""
    return 2.0 ** (math.floor(math.log2(max(abs(x), 2.0 ** -126))) - 23)


def scripted_logits(B, V, steps, seed, dtype=torch.float32):
    """seeded logits per step.  Rows finish at several lengths: in row b the EOS logit is lifted above the row's maximum at step
    finish_step(b, steps) (rows with b % 6 in (4, 5) never finish).  Rows with b % 6 == 1 get REPEAT_TOKEN lifted far above everything
    else at every step, so that NoRepeatNGram(3) bans the row's LARGEST logit from the fourth repeat on (the ban path of the sum)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for t in range(steps):
        x = torch.randn(B, V, generator=g) * 3.0
        top = x.max(dim=1).values
        for b in range(B):
            if b % 6 == 1:
                x[b, REPEAT_TOKEN] = top[b] + 3.0
            elif finish_step(b, steps) == t:
                x[b, EOS] = top[b] + 1.0 + float(torch.rand((), generator=g))
        out.append(x.to(dtype).contiguous())
    return out


def finish_step(b, steps):
    return {0: min(2, steps - 1), 2: min(5, steps - 1), 3: steps - 2}.get(b % 6)


def processed_logprobs_f64(logits, bias, prefix_ids, ngram, fbos, feos, max_length):
    """f64 log-softmax of the PROCESSED scores in hf's greedy order — logits (+ final_logits_bias), then NoRepeatNGram, ForcedBOS,
    ForcedEOS (transformers' own processors), then normalise — which is what compute_transition_scores(normalize_logits=True) reports
    for greedy `scores`.  Returns (log-probs [B, V] f64, processed scores [B, V] f64)."""
    from transformers.generation.logits_process import (ForcedBOSTokenLogitsProcessor, ForcedEOSTokenLogitsProcessor,
                                                        NoRepeatNGramLogitsProcessor)
    x = logits.double() + (bias.double() if bias is not None else 0.0)
    if ngram > 0:
        x = NoRepeatNGramLogitsProcessor(ngram)(prefix_ids, x)
    if fbos >= 0:
        x = ForcedBOSTokenLogitsProcessor(fbos)(prefix_ids, x)
    if feos >= 0:
        x = ForcedEOSTokenLogitsProcessor(max_length, feos)(prefix_ids, x)
    return torch.log_softmax(x, dim=-1), x


def greedy_op(L, dtype, logits, bias, ids, fin, step, logp, B, V, T, max_new, ngram, fbos, feos):
    ptr = lambda t: t.data_ptr() if t is not None else None
    return L.make_op(L.OP_GREEDY_STEP, dtype, p=[ptr(logits), ptr(bias), ptr(ids), ptr(fin), ptr(logp), None, ptr(step)],
                     i={0: B, 1: V, 2: V, 3: T, 4: max_new, 5: ngram, 6: BOS, 7: EOS, 8: PAD, 9: fbos, 10: feos, 11: 1})


def run_greedy(L, dev, seq, bias, dtype, T, max_new, ngram, fbos, feos, scores, sync=lambda: None):
    """`len(seq)` launches of OMNI_OP_GREEDY_STEP on the scripted logits -> host (ids, finished, step, logp or None); logp starts as
    zeros, as `_StepPlans.reset` leaves it"""
    B, V = seq[0].shape
    ids = torch.zeros(B, T, dtype=torch.int32); ids[:, 0] = START
    d_ids, d_fin, d_step = ids.to(dev), torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    d_logp = torch.zeros(B, T, dtype=torch.float32, device=dev) if scores else None
    d_bias = bias.to(dev) if bias is not None else None
    d_logits = torch.empty_like(seq[0], device=dev)
    op = greedy_op(L, dtype, d_logits, d_bias, d_ids, d_fin, d_step, d_logp, B, V, T, max_new, ngram, fbos, feos)
    for x in seq:
        d_logits.copy_(x)
        L.launch(op)
        sync()
    return d_ids.cpu(), d_fin.cpu(), d_step.cpu(), (d_logp.cpu() if scores else None)


def check_kernel_case(L, dev, B, V, steps, ngram, forced, with_bias, f16, seed, sync=lambda: None, T=17, max_new=16):
    """One case of the kernel check (tests/test_token_scores_emu_cpu.py case 1): see the module docstring for the bound.  Returns
    {max_err, max_bound_ratio, finished_early, unfinished} and asserts everything else."""
    dtype, tdt = (L.F16, torch.float16) if f16 else (L.F32, torch.float32)
    fbos, feos = (BOS, EOS) if forced else (-1, -1)
    seq = scripted_logits(B, V, steps, seed, tdt)
    bias = torch.randn(V, generator=torch.Generator().manual_seed(seed + 1)) * 0.5 if with_bias else None
    ids, fin, step, logp = run_greedy(L, dev, seq, bias, dtype, T, max_new, ngram, fbos, feos, True, sync)
    ids0, fin0, step0, _ = run_greedy(L, dev, seq, bias, dtype, T, max_new, ngram, fbos, feos, False, sync)
    assert torch.equal(ids, ids0) and torch.equal(fin, fin0) and torch.equal(step, step0), "p4 changed ids / finished / step"
    assert int(step[0]) == steps
    # the ids are transformers' greedy ids (f64 arg-max over the same logits)
    ids_r = torch.zeros(B, T, dtype=torch.int32); ids_r[:, 0] = START
    fin_r = torch.zeros(B, dtype=torch.int32)
    worst, ratio, banned_max = 0.0, 0.0, 0
    assert torch.equal(logp[:, 0], torch.zeros(B)) and torch.equal(logp[:, steps + 1:], torch.zeros(B, T - steps - 1))
    for t in range(steps):
        was_fin = fin_r.clone()
        lsm, proc = processed_logprobs_f64(seq[t], bias, ids_r[:, :t + 1].long(), ngram, fbos, feos, max_new + 1)
        raw = seq[t].double() + (bias.double() if bias is not None else 0.0)
        PI.greedy_step_ref(seq[t], bias, ids_r, fin_r, t, max_new, ngram, EOS, PAD, fbos, feos, torch.float64)
        assert torch.equal(ids[:, t + 1], ids_r[:, t + 1]), (t, ids[:, t + 1].tolist(), ids_r[:, t + 1].tolist())
        is_forced = (fbos >= 0 and t == 0) or (feos >= 0 and t + 1 == max_new)
        for b in range(B):
            got = float(logp[b, t + 1])
            if is_forced or was_fin[b]:
                assert got == 0.0, (b, t, got)
                continue
            tok = int(ids_r[b, t + 1])
            finite = proc[b][torch.isfinite(proc[b])]
            bound = 2.0 ** -23 * (V / 256 + 16) + 4 * ulp_f32(float(finite.abs().max()))
            err = abs(got - float(lsm[b, tok]))
            assert err <= bound, f"row {b} step {t}: logp {got} vs f64 {float(lsm[b, tok])}: {err:.3e} > {bound:.3e}"
            worst, ratio = max(worst, err), max(ratio, err / bound)
            banned_max += int(float(raw[b].max()) > float(finite.max()))       # the ban removed the row's largest logit
    assert torch.equal(fin, fin_r)
    first_eos = [next((p for p in range(1, steps + 1) if int(ids[b, p]) == EOS), None) for b in range(B)]
    return {"max_err": worst, "max_bound_ratio": ratio, "banned_max": banned_max,
            "finished_early": sum(p is not None and p < max_new for p in first_eos),      # before max_new (where EOS may be forced)
            "unfinished": sum(p is None or p >= max_new for p in first_eos)}


def check_degenerate_rows(L, dev, sync=lambda: None):
    """the all-NaN and all -inf rows of gpu_checks.check_greedy_degenerate_rows with p4 set: same ids as with p4 = NULL, all in range"""
    Bq, Vv, T = 4, 1000, 21
    logits = torch.randn(Bq, Vv, generator=torch.Generator().manual_seed(0))
    logits[1] = float("nan")
    logits[2] = float("-inf")
    ids = torch.zeros(Bq, T, dtype=torch.int32); ids[:, 0] = START
    ids[:, 1:6] = torch.tensor([[0, 7, 8, 7, 9]] * Bq, dtype=torch.int32)
    got = {}
    for scores in (False, True):
        d = {"logits": logits.to(dev), "ids": ids.to(dev), "fin": torch.zeros(Bq, dtype=torch.int32, device=dev),
             "step": torch.tensor([5], dtype=torch.int32, device=dev), "logp": torch.zeros(Bq, T, device=dev) if scores else None}
        L.launch(greedy_op(L, L.F32, d["logits"], None, d["ids"], d["fin"], d["step"], d["logp"], Bq, Vv, T, 20, 0, -1, -1))
        sync()
        got[scores] = (d["ids"].cpu(), d["fin"].cpu(), d["step"].cpu())
        if scores:
            lp = d["logp"].cpu()
    for a, b in zip(got[True], got[False]):
        assert torch.equal(a, b)
    new = got[True][0][:, 6].tolist()
    assert new == [int(torch.argmax(logits[0])), 0, 0, int(torch.argmax(logits[3]))], new
    assert all(0 <= t < Vv for t in new)
    for b in (0, 3):                             # the ordinary rows next to them still get their log-probability
        assert abs(float(lp[b, 6]) - float(torch.log_softmax(logits[b].double(), -1).max())) < 1e-5
    return new


# ---------------------------------------------------------------------------------------------- whole captioner vs transformers
def hf_greedy_scores(model, pix, max_new):
    """transformers generate(num_beams=1, output_scores=True) on the fixed <CAPTION> prompt -> (sequences, transition scores
    [n, generated] with normalize_logits=True, per row and position the top-1 / top-2 gap of the processed scores)"""
    from omniparser_amd.florence import PROMPT_IDS
    cfg = model.config
    n = pix.shape[0]
    n_img = (pix.shape[-1] // 32) ** 2 + 1
    inp = torch.tensor([[cfg.image_token_id] * n_img + PROMPT_IDS] * n)
    with torch.inference_mode():
        out = model.generate(input_ids=inp, pixel_values=pix, max_new_tokens=max_new, num_beams=1, do_sample=False,
                             output_scores=True, return_dict_in_generate=True)
        ts = model.compute_transition_scores(out.sequences, out.scores, normalize_logits=True)
    gaps = []
    for s in out.scores:
        top = s.double().topk(2, dim=-1).values
        g = top[:, 0] - top[:, 1]
        g[~torch.isfinite(g)] = float("inf")                  # a forced position is no decision
        gaps.append(g)
    return out.sequences, ts.double(), torch.stack(gaps, 1)


def compare_with_hf(got_seq, got_logp, ref_seq, ref_ts, gaps, eos, pad, tol, max_excused=1):
    """rows whose ids agree: |token_logprobs - transformers| <= tol on the positions up to the row's first EOS.  A row that differs
    passes only if the oracle's own top-1 / top-2 gap at the first differing position is below beam_checks.MARGIN, and at most
    `max_excused` rows may.  Returns (largest |delta logp|, rows excused)."""
    n = ref_seq.shape[0]
    T = max(got_seq.shape[1], ref_seq.shape[1])
    padto = lambda t, v: torch.nn.functional.pad(t, (0, T - t.shape[1]), value=v) if t.shape[1] < T else t
    g, r = padto(got_seq.long(), pad), padto(ref_seq.long(), pad)
    worst, excused, failures = 0.0, 0, []
    for b in range(n):
        if not torch.equal(g[b], r[b]):
            p = int((g[b] != r[b]).nonzero()[0])
            gap = float(gaps[b, p - 1]) if p - 1 < gaps.shape[1] else float("inf")
            if gap < BC.MARGIN:
                excused += 1
            else:
                failures.append({"row": b, "position": p, "gap": gap, "got": g[b].tolist(), "ref": r[b].tolist()})
            continue
        gen = ref_seq.shape[1] - 1
        end = next((p for p in range(1, gen + 1) if int(r[b, p]) == eos), gen)
        d = (got_logp[b, :end].double() - ref_ts[b, :end]).abs()
        worst = max(worst, float(d.max()))
        if float(d.max()) > tol:
            failures.append({"row": b, "max_dlogp": float(d.max()), "got": got_logp[b, :end].tolist(), "ref": ref_ts[b, :end].tolist()})
    assert not failures, failures[:3]
    assert excused <= max_excused, f"{excused} rows below the margin (at most {max_excused})"
    return worst, excused


def captioner_vs_hf(n, seed, eos_prone, max_new, device_pixels=False, R=64, tol=None):
    """Florence2Captioner.generate(output_scores=True) against transformers on n seeded RxR crops.  Returns the captioner, the
    pixels, its output and the largest |delta logp| (printed before it is compared: the measurement of TOL_LOGP)."""
    from omniparser_amd.florence import Florence2Captioner
    from tools.make_weights import ensure_caption_checkpoint
    pix = torch.randn(n, 3, R, R, generator=torch.Generator().manual_seed(seed))
    model = BC.oracle_model(0, eos_prone)
    try:
        ref_seq, ref_ts, gaps = hf_greedy_scores(model, pix, max_new)
        eos = model.generation_config.eos_token_id
    finally:
        model.generation_config.eos_token_id = 2
    d = BC.eos_prone_checkpoint(0) if eos_prone else ensure_caption_checkpoint(0)
    cap = Florence2Captioner(d, "cuda", precision="f32", resolution=R)
    px = pix.cuda() if device_pixels else pix
    out = cap.generate(pixel_values=px, max_new_tokens=max_new, output_scores=True, return_dict_in_generate=True)
    assert out.sequences_scores is None and out.token_logprobs.dtype == torch.float32
    assert tuple(out.token_logprobs.shape) == (n, out.sequences.shape[1] - 1)
    worst, excused = compare_with_hf(out.sequences, out.token_logprobs, ref_seq, ref_ts, gaps, eos, cap.w.pad, float("inf"))
    print(f"token scores vs transformers: n={n} eos_prone={eos_prone} max_new={max_new}: max |dlogp| = {worst:.3e}, {excused} rows "
          f"below the margin, lengths {sorted(int((r != cap.w.pad).sum()) for r in ref_seq)}")
    compare_with_hf(out.sequences, out.token_logprobs, ref_seq, ref_ts, gaps, eos, cap.w.pad, TOL_LOGP if tol is None else tol)
    return cap, px, out, worst

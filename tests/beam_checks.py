"""Beam-search parity harness shared by the CPU (emulation) and GPU tests of OMNI_OP_BEAM_STEP / Florence2Captioner.generate(num_beams > 1).

The oracle is transformers' own `_beam_search` step helpers (hf:generation/utils.py:3008-3206), driven here step by step.  The same
replay also yields, per crop, the smallest decision gap the oracle met: between the 2k-th and (2k+1)-th accumulated score (top-2k
cut), the k-th and (k+1)-th running candidate (next running beams) and the k-th and (k+1)-th merged finished entry.  Gaps between
two -1e9 sentinels are not decisions (hf's sentinels tie by construction) and are skipped.  Margin rule: a crop whose result differs
from the oracle's passes only if that gap is below MARGIN — torch.topk orders ties and near-ties in its own way."""
import json
from types import SimpleNamespace

import torch

MARGIN = 2e-4
_SENTINEL = -5e8


def hf_helpers():
    """a (tiny) transformers generation model instance: the beam helpers are its methods and read no model state"""
    from transformers import BartConfig, BartForConditionalGeneration
    cfg = BartConfig(vocab_size=64, d_model=16, encoder_layers=1, decoder_layers=1, encoder_attention_heads=2,
                     decoder_attention_heads=2, encoder_ffn_dim=16, decoder_ffn_dim=16, max_position_embeddings=64)
    return BartForConditionalGeneration(cfg).eval()


def _cut_gap(values: torch.Tensor, k: int) -> torch.Tensor:
    """per row: |v[k-1] - v[k]| of the descending sort, inf where either side is a sentinel / -inf or there is no k-th entry"""
    if values.shape[1] <= k:
        return torch.full((values.shape[0],), float("inf"))
    s = values.sort(dim=1, descending=True).values
    a, b = s[:, k - 1].double(), s[:, k].double()
    gap = (a - b).abs()
    gap[(a < _SENTINEL) | (b < _SENTINEL)] = float("inf")
    return gap


def hf_beam_replay(model, logprobs_at, B, k, V, max_new, start, pad, eos, length_penalty=1.0, early_stopping=False):
    """transformers' _beam_search loop (decoder prompt = the start token) with its own helpers; `logprobs_at(t, flat_running_ids)` returns
    the PROCESSED log-probs [B k, V] of step t (log_softmax + logits processors).  Returns the final state and per-crop min gaps."""
    max_length = max_new + 1
    cur_len, prompt = 1, 1
    K2 = 2 * k
    top_mask = torch.cat((torch.ones(k, dtype=torch.bool), torch.zeros(K2 - k, dtype=torch.bool)))
    running = torch.full((B, k, max_length), pad, dtype=torch.int64)
    running[:, :, 0] = start
    sequences = running.clone()
    run_scores = torch.zeros((B, k))
    run_scores[:, 1:] = -1e9
    beam_scores = torch.full((B, k), -1e9)
    fin = torch.zeros((B, k), dtype=torch.bool)
    unsat = torch.ones((B, 1), dtype=torch.bool)
    run_bi = torch.full((B, k, max_length - 1), -1, dtype=torch.int32)
    beam_indices = run_bi.clone()
    gaps = torch.full((B,), float("inf"), dtype=torch.float64)
    frozen = torch.zeros(B, dtype=torch.bool)
    steps = 0
    while True:
        flat = running[:, :, :cur_len].reshape(B * k, cur_len)
        lp = logprobs_at(steps, flat).float()
        acc = (lp.view(B, k, V) + run_scores[:, :, None]).reshape(B, k * V)
        live = ~frozen
        gaps[live] = torch.minimum(gaps[live], _cut_gap(acc, K2)[live])
        topk_lp, topk_seq, topk_bi = model._get_top_k_continuations(acc, running, run_bi, cur_len, prompt, False, K2, k, V, B)
        stop = (topk_seq[:, :, cur_len] == eos) | (cur_len + 1 >= max_length)
        gaps[live] = torch.minimum(gaps[live], _cut_gap(topk_lp + stop.float() * -1e9, k)[live])
        running, run_scores, run_bi = model._get_running_beams_for_next_iteration(topk_lp, topk_seq, topk_bi, stop, k)
        # finished-merge cut, recomputed the way _update_finished_beams scores the candidates
        fl = topk_lp / ((cur_len + 1 - prompt) ** length_penalty)
        fl = fl + (torch.all(fin, -1, keepdim=True) & (early_stopping is True)).float() * -1e9
        fl = fl + (~unsat).float() * -1e9
        fl = fl + (~(stop & top_mask[None, :])) * -1e9
        gaps[live] = torch.minimum(gaps[live], _cut_gap(torch.cat((beam_scores, fl), 1), k)[live])
        sequences, beam_scores, beam_indices, fin = model._update_finished_beams(
            sequences, topk_seq, beam_scores, topk_lp, beam_indices, topk_bi, unsat, fin, stop, top_mask, k, cur_len, prompt,
            length_penalty, early_stopping)
        cur_len += 1
        steps += 1
        unsat = model._check_early_stop_heuristic(unsat, run_scores, beam_scores, fin, cur_len, max_length, prompt, early_stopping,
                                                  length_penalty)
        frozen = frozen | ~unsat[:, 0] | (fin.all(-1) & (early_stopping is True)) | stop.all(-1)
        if not bool(model._beam_search_has_unfinished_sequences(unsat, fin, stop, early_stopping)):
            break
    lengths = ((beam_indices + 1).bool()).sum(-1)
    return SimpleNamespace(sequences=sequences, scores=beam_scores, finished=fin, lengths=lengths, gaps=gaps, steps=steps)


def hf_processed_logprobs(logits, flat_ids, ngram, forced_bos, forced_eos, max_length, bias=None):
    """log_softmax in f32 + hf's processors in hf's order (NoRepeatNGram, ForcedBOS, ForcedEOS)"""
    from transformers.generation.logits_process import (ForcedBOSTokenLogitsProcessor, ForcedEOSTokenLogitsProcessor,
                                                        NoRepeatNGramLogitsProcessor)
    x = logits.float() + (bias if bias is not None else 0.0)
    lp = torch.nn.functional.log_softmax(x, dim=-1)
    if ngram > 0:
        lp = NoRepeatNGramLogitsProcessor(ngram)(flat_ids, lp)
    if forced_bos >= 0:
        lp = ForcedBOSTokenLogitsProcessor(forced_bos)(flat_ids, lp)
    if forced_eos >= 0:
        lp = ForcedEOSTokenLogitsProcessor(max_length, forced_eos)(flat_ids, lp)
    return lp


def compare_crops(got_ids, got_scores, ref_ids, ref_scores, gaps, nrs, pad, score_rtol):
    """per crop (nrs rows each): ids equal (trailing pad ignored) and scores within score_rtol, or the oracle's gap below MARGIN.
    Returns (crops compared, below-margin cases, failures)."""
    n = gaps.shape[0]
    below, failures = 0, []
    T = max(got_ids.shape[1], ref_ids.shape[1])
    pad_to = lambda t: torch.cat((t, torch.full((t.shape[0], T - t.shape[1]), pad, dtype=t.dtype)), 1) if t.shape[1] < T else t
    g, r = pad_to(got_ids.long()), pad_to(ref_ids.long())
    for c in range(n):
        rows = slice(c * nrs, (c + 1) * nrs)
        ok = torch.equal(g[rows], r[rows])
        if ok and ref_scores is not None:
            rs, gs = ref_scores[rows].double(), got_scores[rows].double()
            ok = bool(((gs - rs).abs() <= score_rtol * rs.abs().clamp_min(1e-30)).all())
        if ok:
            continue
        if float(gaps[c]) < MARGIN:
            below += 1
        else:
            failures.append({"crop": c, "gap": float(gaps[c]), "got": g[rows].tolist(), "ref": r[rows].tolist(),
                             "got_scores": None if got_scores is None else got_scores[rows].tolist(),
                             "ref_scores": None if ref_scores is None else ref_scores[rows].tolist()})
    return n, below, failures


# ---------------------------------------------------------------------------------------------- whole captioner vs transformers
EOS_PRONE_TOKEN = 13840


def eos_prone_checkpoint(seed=0):
    """The stand-in caption checkpoint with `eos_token_id` = 13840 in generation_config.json (same weights, same decoder start token 2
    and forced EOS 2): a token the stand-in emits often but rarely first, so beam hypotheses finish at several lengths before
    max_new_tokens.  Calibration (transformers 5.15 on the CPU, generate(num_beams=3, max_new_tokens=20), 32 seeded 64x64 crops,
    seed 101, as in tests/test_gpu_l_beam_search.py): generated lengths of the best hypotheses 2 (x21), 8 (x3), 11 (x1), 17 (x1),
    20 (x6); with the stock eos_token_id = 2 every one of them is 20.  The transformers model of a test must get the same setting
    (`oracle_model`)."""
    from tools.make_weights import ensure_caption_checkpoint
    src = ensure_caption_checkpoint(seed)
    dst = src.with_name(src.name + "_eos13840")
    if not (dst / "model.safetensors").exists():
        dst.mkdir(parents=True, exist_ok=True)
        for f in ("model.safetensors", "config.json"):
            if not (dst / f).exists():
                (dst / f).symlink_to(src / f)
        gen = json.loads((src / "generation_config.json").read_text())
        gen["eos_token_id"] = EOS_PRONE_TOKEN
        (dst / "generation_config.json").write_text(json.dumps(gen))
    return dst


def oracle_model(seed=0, eos_prone=False):
    """transformers' Florence-2 stand-in with the generation settings of the checkpoint the device loads"""
    from tools.make_weights import shared_random_captioner
    m = shared_random_captioner(seed)
    m.generation_config.eos_token_id = EOS_PRONE_TOKEN if eos_prone else 2
    return m


def hf_generate_beams(model, pix, k, max_new, nrs=1, length_penalty=None, early_stopping=None):
    """transformers generate(num_beams=k) on the fixed <CAPTION> prompt + the replay of its processed scores (gaps)"""
    from omniparser_amd.florence import PROMPT_IDS
    cfg, gc = model.config, model.generation_config
    n = pix.shape[0]
    n_img = (pix.shape[-1] // 32) ** 2 + 1
    inp = torch.tensor([[cfg.image_token_id] * n_img + PROMPT_IDS] * n)
    kw = {}
    if length_penalty is not None:
        kw["length_penalty"] = length_penalty
    if early_stopping is not None:
        kw["early_stopping"] = early_stopping
    with torch.inference_mode():
        out = model.generate(input_ids=inp, pixel_values=pix, max_new_tokens=max_new, num_beams=k, do_sample=False,
                             num_return_sequences=nrs, return_dict_in_generate=True, output_scores=True, **kw)
    steps = out.scores
    V = steps[0].shape[-1]
    pick = lambda *v: next(x for x in v if x is not None)
    tc = cfg.get_text_config()
    rep = hf_beam_replay(hf_helpers(), lambda t, ids: steps[t], n, k, V, max_new,
                         pick(gc.decoder_start_token_id, tc.decoder_start_token_id), pick(gc.pad_token_id, tc.pad_token_id),
                         gc.eos_token_id, pick(length_penalty, gc.length_penalty, 1.0), pick(early_stopping, gc.early_stopping, False))
    return out, rep

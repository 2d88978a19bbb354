"""Beam-search decoding of the captioner (OMNI_OP_BEAM_STEP, the position table of OMNI_OP_ATTN_DECODE, Florence2Captioner.generate with
num_beams > 1) on the host emulation of the HIP kernels (tests/emu), against transformers' own beam-search step helpers and its
generate(num_beams=3).  Margin rule and oracle replay: tests/beam_checks.py."""
import itertools

import pytest
import torch

from omniparser_amd import _lib as L

START, PAD, EOS, BOS = 2, 1, 2, 0


def _beam_op(logits, ids, run_score, table, fin_ids, step, state, B, k, V, T, max_new, ngram, fbos, feos, lp, es):
    from omniparser_amd.florence import _EARLY_STOPPING_CODE
    return L.make_op(L.OP_BEAM_STEP, L.F32,
                     p=[logits.data_ptr(), None, ids.data_ptr(), run_score.data_ptr(), table.data_ptr(), fin_ids.data_ptr(),
                        step.data_ptr(), state.data_ptr()],
                     i={0: B, 1: V, 2: V, 3: T, 4: max_new, 5: ngram, 6: k, 7: EOS, 8: PAD, 9: fbos, 10: feos, 11: 1,
                        12: _EARLY_STOPPING_CODE[es]},
                     f={0: lp})


def _scripted_logits(B, k, V, steps, seed):
    """seeded logits per step with EOS boosted on chosen (crop, beam, step) cells, so hypotheses finish at several lengths"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for t in range(steps):
        x = torch.randn(B * k, V, generator=g) * 3.0
        boost = torch.rand(B * k, generator=g) < 0.25
        x[boost, EOS] += 4.0 + 4.0 * torch.rand(int(boost.sum()), generator=g)
        out.append(x.contiguous())
    return out


CASES = [(k, lp, es, ng, forced, nrs)
         for (k, lp, es), ng, forced in zip(itertools.product((2, 3, 5), (1.0, 0.0, 2.0, -0.5), (False, True, "never")),
                                            itertools.cycle((3, 0)), itertools.cycle((True, True, False)))
         for nrs in ((1,) if (k + int(lp * 2)) % 2 else (k,))]


@pytest.mark.parametrize("k,lp,es,ngram,forced,nrs", CASES)
def test_beam_step_matches_hf_helpers(emu, k, lp, es, ngram, forced, nrs):
    """OMNI_OP_BEAM_STEP over 16 steps of scripted logits vs hf's _beam_search helpers on the same logits: finished ids, scores
    (1e-5 relative), flags and lengths of the returned hypotheses, under the margin rule."""
    import beam_checks as BC
    B, V, max_new = 6, 2003, 16
    T = max_new + 1
    fbos, feos = (BOS, EOS) if forced else (-1, -1)
    seq = _scripted_logits(B, k, V, max_new, seed=k * 100 + int(lp * 10) + ngram + (7 if forced else 0))
    ref = BC.hf_beam_replay(BC.hf_helpers(),
                            lambda t, ids: BC.hf_processed_logprobs(seq[t], ids, ngram, fbos, feos, max_new + 1),
                            B, k, V, max_new, START, PAD, EOS, lp, es)
    # device state, initialised as _StepPlans._reset_beams does
    ids = torch.full((B * k, T), PAD, dtype=torch.int32); ids[:, 0] = START
    table = torch.arange(B * k, dtype=torch.int32)[:, None].expand(B * k, T).contiguous()
    run_score = torch.zeros(B, k); run_score[:, 1:] = -1e9; run_score = run_score.reshape(-1).contiguous()
    fin_ids = torch.full((B, k, T), PAD, dtype=torch.int32); fin_ids[:, :, 0] = START
    state = torch.zeros(B * (3 * k + 2), dtype=torch.int32)
    state[:B * k].view(torch.float32).fill_(-1e9)
    state[3 * B * k:3 * B * k + B] = 1
    step = torch.zeros(1, dtype=torch.int32)
    logits = torch.empty(B * k, V)
    op = _beam_op(logits, ids, run_score, table, fin_ids, step, state, B, k, V, T, max_new, ngram, fbos, feos, lp, es)
    for t in range(max_new):
        logits.copy_(seq[t])
        L.launch(op)
        # the position table always names a row of the same crop, and position t + 1 the row itself
        crop_of = table[:, :t + 1] // k
        assert torch.equal(crop_of, (torch.arange(B * k) // k)[:, None].expand_as(crop_of))
        assert torch.equal(table[:, t + 1], torch.arange(B * k, dtype=torch.int32))
    frozen = state[3 * B * k + B:]
    assert bool(frozen.all())
    fs = state[:B * k].view(torch.float32).view(B, k)
    flag = state[B * k:2 * B * k].view(B, k)
    length = state[2 * B * k:3 * B * k].view(B, k)
    got_ids = fin_ids[:, :nrs].reshape(B * nrs, T)
    n, below, failures = BC.compare_crops(got_ids, fs[:, :nrs].reshape(-1), ref.sequences[:, :nrs].reshape(B * nrs, -1),
                                          ref.scores[:, :nrs].reshape(-1), ref.gaps, nrs, PAD, 1e-5)
    assert not failures, failures
    same = [c for c in range(B) if torch.equal(fin_ids[c].long(), ref.sequences[c])]
    for c in same:
        assert torch.equal(flag[c].bool(), ref.finished[c]), c
        assert torch.equal(length[c].long(), ref.lengths[c].long()), c
    assert len(same) + below >= B
    print(f"k={k} lp={lp} es={es}: {n} crops, {below} below the margin")


def test_beam_step_covers_early_finishing_hypotheses(emu):
    """the scripted logits of the parity cases do finish hypotheses before max_new_tokens (the finished-merge and heuristic paths run)"""
    import beam_checks as BC
    B, k, V, max_new = 6, 3, 2003, 16
    seq = _scripted_logits(B, k, V, max_new, seed=5)
    ref = BC.hf_beam_replay(BC.hf_helpers(), lambda t, ids: BC.hf_processed_logprobs(seq[t], ids, 3, BOS, EOS, max_new + 1),
                            B, k, V, max_new, START, PAD, EOS, 1.0, False)
    assert (ref.lengths[ref.finished] < max_new).any()


def test_attn_decode_position_table_equals_gathered_cache(emu):
    """OMNI_OP_ATTN_DECODE self-attention through a position table == the same step on a physically gathered cache, bit for bit"""
    torch.manual_seed(0)
    Bn, T, heads, D = 6, 9, 2, 128
    st = 5
    kc = torch.randn(Bn, T, D); vc = torch.randn(Bn, T, D)
    qkv = torch.randn(Bn, 3 * D)
    table = torch.randint(0, Bn, (Bn, T), dtype=torch.int32)
    table[:, st] = torch.arange(Bn, dtype=torch.int32)
    step = torch.tensor([st], dtype=torch.int32)

    def run(kcache, vcache, tab):
        o = torch.zeros(Bn, D)
        op = L.make_op(L.OP_ATTN_DECODE, L.F32,
                       p=[qkv.data_ptr(), qkv.data_ptr(), qkv.data_ptr(), kcache.data_ptr(), o.data_ptr(), vcache.data_ptr(),
                          step.data_ptr()] + ([tab.data_ptr()] if tab is not None else []),
                       i={0: 3 * D, 1: 0, 2: 3 * D, 3: D, 4: 2 * D, 5: D, 6: heads, 7: 0, 8: T, 9: D, 10: Bn, 11: D},
                       f={0: 64 ** -0.5})
        L.launch(op)
        return o

    k1, v1 = kc.clone(), vc.clone()
    o_table = run(k1, v1, table)
    pos = torch.arange(T)
    kg = kc[table.long(), pos[None, :]].contiguous(); vg = vc[table.long(), pos[None, :]].contiguous()
    o_gather = run(kg, vg, None)
    assert torch.equal(o_table, o_gather)
    assert torch.equal(k1[:, st], kg[:, st]) and torch.equal(k1[:, st], qkv[:, D:2 * D])      # appended at (row, step)


def test_attn_decode_cross_rows_per_kv_row(emu):
    """cross-attention with i12 = k: k query rows read one K/V row == the same rows against a k-times repeated K/V"""
    torch.manual_seed(1)
    crops, k, S, heads, D = 3, 3, 11, 2, 128
    q = torch.randn(crops * k, D)
    kv = torch.randn(crops, S, 2 * D)
    esz = 4

    def run(kvt, div):
        o = torch.zeros(crops * k, D)
        op = L.make_op(L.OP_ATTN_DECODE, L.F32, p=[q.data_ptr(), None, None, kvt.data_ptr(), o.data_ptr(), kvt.data_ptr() + D * esz, None],
                       i={0: D, 1: 0, 2: 0, 3: 0, 4: 0, 5: D, 6: heads, 7: S, 8: S, 9: D, 10: crops * k, 11: 2 * D,
                          **({12: div} if div > 1 else {})}, f={0: 64 ** -0.5})
        L.launch(op)
        return o

    assert torch.equal(run(kv, k), run(kv.repeat_interleave(k, 0).contiguous(), 1))


@pytest.mark.parametrize("eos_prone", [False, True])
def test_captioner_beam_search_matches_transformers_r64(emu, eos_prone):
    """Florence2Captioner.generate(num_beams=3, max_new_tokens=4) at 64x64 on 2 crops vs transformers generate(num_beams=3): ids under
    the margin rule, sequences_scores within 1e-4 relative; the greedy plan's op list has no beam op and the beam plan no greedy op."""
    import beam_checks as BC
    from omniparser_amd.florence import Florence2Captioner
    from tools.make_weights import ensure_caption_checkpoint
    max_new, k = 4, 3
    pix = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(31))
    model = BC.oracle_model(0, eos_prone)
    try:
        ref, rep = BC.hf_generate_beams(model, pix, k, max_new)
    finally:
        model.generation_config.eos_token_id = 2
    d = BC.eos_prone_checkpoint(0) if eos_prone else ensure_caption_checkpoint(0)
    cap = Florence2Captioner(d, "cuda", precision="f32", resolution=64)
    out = cap.generate(pixel_values=pix, max_new_tokens=max_new, num_beams=k, return_dict_in_generate=True)
    assert torch.equal(rep.sequences[:, 0, :ref.sequences.shape[1]], ref.sequences)          # the replay IS hf's search
    n, below, failures = BC.compare_crops(out.sequences, out.sequences_scores, ref.sequences, ref.sequences_scores, rep.gaps, 1,
                                          cap.w.pad, 1e-4)
    assert not failures, failures
    assert out.sequences.shape == ref.sequences.shape or below
    print(f"eos_prone={eos_prone}: {n} crops, {below} below the margin")
    beam_plan = cap.plans(cap.bucket(2), 64, max_new, beam=cap.beam_config(k))
    kinds = [op.kind for op in beam_plan.step_plan.ops]
    assert L.OP_BEAM_STEP in kinds and L.OP_GREEDY_STEP not in kinds


def test_beam_step_op_kind_mirrors_the_header():
    """OMNI_OP_BEAM_STEP is the enumerator after OMNI_OP_MLP_FUSED (= 24), i.e. 25, in include/omni_amd.h and in _lib"""
    import re
    from pathlib import Path
    hdr = (Path(__file__).resolve().parents[1] / "include" / "omni_amd.h").read_text()
    assert re.search(r"OMNI_OP_MLP_FUSED = 24,\s*(/\*.*?\*/\s*)?OMNI_OP_BEAM_STEP,\s*OMNI_OP__COUNT", hdr, re.S)
    assert L.OP_BEAM_STEP == 25 == L.OP_MLP_FUSED + 1


def test_generate_argument_validation(emu):
    from omniparser_amd.florence import Florence2Captioner
    from tools.make_weights import ensure_caption_checkpoint
    cap = Florence2Captioner(ensure_caption_checkpoint(0), "cuda", precision="f32", resolution=64)
    pix = torch.zeros(1, 3, 64, 64)
    with pytest.raises(ValueError):
        cap.generate(pixel_values=pix, num_beams=9)
    with pytest.raises(ValueError):
        cap.generate(pixel_values=pix, num_beams=3, num_return_sequences=4)
    with pytest.raises(ValueError):
        cap.generate(pixel_values=pix, num_beams=1, num_return_sequences=2)
    with pytest.raises(ValueError):
        cap.generate(pixel_values=pix, num_beams=3, early_stopping="sometimes")
    with pytest.raises(NotImplementedError):
        cap.generate(pixel_values=pix, num_beams=3, do_sample=True)
    with pytest.raises(ValueError):
        cap.caption_crops(torch.zeros(64, 64, 3, dtype=torch.uint8), [[0, 0, 8, 8]], num_beams=0)
    assert cap._plans == {}                  # nothing was built for a refused call

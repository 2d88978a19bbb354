"""Generation-control checks shared by the CPU (emulation) and GPU tests of OMNI_OP_GREEDY_CTRL_STEP and of
Florence2Captioner.generate(repetition_penalty=..., no_repeat_ngram_size=..., min_new_tokens=..., suppress_tokens=...,
begin_suppress_tokens=..., bad_words_ids=...): the kernel against transformers' own logits processors applied to the f32 scores, the
captioner against transformers' generate() on the CPU, and the plan / default-path rules.

Kernel expectation: logits + final_logits_bias in f32, then transformers' RepetitionPenalty, NoRepeatNGram, NoBadWords,
MinNewTokensLength, ForcedBOS, ForcedEOS, SuppressTokens and SuppressTokensAtBegin processors in that order, all in f32 — exactly what
the kernel computes, so the token must be EQUAL — then an f64 log-softmax of those f32 values for the log-probability, held to the
derived two-pass bound of long_checks.expect_greedy / score_checks (it scales with the largest finite processed value, so the
penalty's products and quotients are covered).  Model tolerance: long_checks.TOL_LOGP_LONG, as it stands."""
import ctypes

import torch

import caption_f64 as CF
import long_checks as LC
import score_checks as SC

START, PAD, EOS, BOS = SC.START, SC.PAD, SC.EOS, SC.BOS
GB, GT, GMAX_NEW, GSTEP = LC.GB, LC.GT, LC.GMAX_NEW, LC.GSTEP
FREE = 1                   # the row of long_greedy_inputs without n-gram structure (distinct tokens 100..221): the scripted row
POISON_WORDS = 32          # 0xFF words behind the control block inside the arena


def controls(**kw):
    from omniparser_amd.florence import GenerationControls
    return GenerationControls(**kw)


# ---------------------------------------------------------------------------------------------- expectation
def expect(logits, bias, ids, fin, st, max_new, op_ngram, fbos, feos, gc):
    """(tokens, logp, finished after, per-row bound, processed f32 scores) of one step: transformers' processors on the f32 scores"""
    from transformers.generation.logits_process import (ForcedBOSTokenLogitsProcessor, ForcedEOSTokenLogitsProcessor,
                                                        MinNewTokensLengthLogitsProcessor, NoBadWordsLogitsProcessor,
                                                        NoRepeatNGramLogitsProcessor, RepetitionPenaltyLogitsProcessor,
                                                        SuppressTokensAtBeginLogitsProcessor, SuppressTokensLogitsProcessor)
    B, V = logits.shape
    x = logits.float() + (bias.float() if bias is not None else 0.0)
    assert x.dtype == torch.float32
    prefix = ids[:, :st + 1].long()
    if gc.repetition_penalty is not None and gc.repetition_penalty != 1.0:
        x = RepetitionPenaltyLogitsProcessor(gc.repetition_penalty)(prefix, x)
    ngram = op_ngram if gc.no_repeat_ngram_size is None else gc.no_repeat_ngram_size
    if ngram > 0:
        x = NoRepeatNGramLogitsProcessor(ngram)(prefix, x)
    if gc.bad_words_ids:
        x = NoBadWordsLogitsProcessor([list(w) for w in gc.bad_words_ids], EOS)(prefix, x)
    if gc.min_new_tokens:
        x = MinNewTokensLengthLogitsProcessor(1, gc.min_new_tokens, EOS, device="cpu")(prefix, x)
    if fbos >= 0:
        x = ForcedBOSTokenLogitsProcessor(fbos)(prefix, x)
    if feos >= 0:
        x = ForcedEOSTokenLogitsProcessor(max_new + 1, feos, device="cpu")(prefix, x)
    if gc.suppress_tokens:
        x = SuppressTokensLogitsProcessor(list(gc.suppress_tokens), device="cpu")(prefix, x)
    if gc.begin_suppress_tokens:
        x = SuppressTokensAtBeginLogitsProcessor(list(gc.begin_suppress_tokens), 2 if fbos >= 0 else 1, device="cpu")(prefix, x)
    assert x.dtype == torch.float32
    forced = (fbos >= 0 and st == 0) or (feos >= 0 and st + 1 == max_new)
    lsm = torch.log_softmax(x.double(), dim=-1)
    toks, lps, bounds, fin2 = [], [], [], fin.clone()
    for b in range(B):
        finite = x[b][torch.isfinite(x[b])]
        tok = int(torch.argmax(x[b])) if finite.numel() else 0
        if forced:
            tok = fbos if st == 0 and fbos >= 0 else feos       # a suppressed forced token would leave hf an all -inf row
        bounds.append(2.0 ** -23 * (V / 256 + 16) + 4 * SC.ulp_f32(float(finite.abs().max())) if finite.numel() else float("inf"))
        lp = 0.0 if forced else float(lsm[b, tok])
        if fin[b]:
            tok, lp = PAD, 0.0
        elif tok == EOS:
            fin2[b] = 1
        toks.append(tok); lps.append(lp)
    return toks, lps, fin2, bounds, x


# ---------------------------------------------------------------------------------------------- one launch inside guard bands
def ctrl_op(L, dtype, ptrs, B, V, T, max_new, ngram, fbos, feos, ctrl_bytes, kind=None):
    return L.make_op(L.OP_GREEDY_CTRL_STEP if kind is None else kind, dtype,
                     p=[ptrs["logits"], ptrs.get("bias"), ptrs["ids"], ptrs["fin"], ptrs.get("logp"), None, ptrs["step"], ptrs.get("ctrl")],
                     i={0: B, 1: V, 2: V, 3: T, 4: max_new, 5: ngram, 6: BOS, 7: EOS, 8: PAD, 9: fbos, 10: feos, 11: 1, 12: ctrl_bytes})


def launch(L, dev, sync, dtype, logits, bias, ids, fin, st, max_new, op_ngram, fbos, feos, scores, block=None, slack=0, what="ctrl"):
    """one launch with every operand in one caption_f64.Arena (0xFF guard bands; logp may only be written in column st + 1, which
    must be written): OMNI_OP_GREEDY_CTRL_STEP with the control block `block` (i32 words) followed by POISON_WORDS 0xFF words, of which
    `slack` count into i12 — or, block None, OMNI_OP_GREEDY_STEP on the same operands.  Returns host (ids, fin, step, logp or None)."""
    B, V = logits.shape
    T = ids.shape[1]
    ar = CF.Arena()
    ar.add("logits", logits.dtype, B, V, data=((0, logits),))
    if bias is not None:
        ar.add("bias", torch.float32, 1, V, data=((0, bias.view(1, V)),))
    ar.add("ids", torch.int32, B, T, data=((0, ids),))
    ar.add("fin", torch.int32, 1, B, data=((0, fin.view(1, B)),))
    ar.add("step", torch.int32, 1, 1, data=((0, torch.tensor([[st]], dtype=torch.int32)),))
    if scores:
        ar.add("logp", torch.float32, B, T, out=((st + 1, 1),))
    if block is not None:
        ar.add("ctrl", torch.int32, 1, block.numel() + POISON_WORDS, data=((0, block.view(1, -1)),))
    ar.build(dev)
    names = ["logits", "ids", "fin", "step"] + (["bias"] if bias is not None else []) + (["logp"] if scores else []) \
        + (["ctrl"] if block is not None else [])
    ptrs = {n: ar.ptr(n) for n in names}
    nbytes = (block.numel() + slack) * 4 if block is not None else 0
    L.launch(ctrl_op(L, dtype, ptrs, B, V, T, max_new, op_ngram, fbos, feos, nbytes, kind=None if block is not None else L.OP_GREEDY_STEP))
    sync()
    ar.fetch(what)
    return (ar.get("ids", 0, T), ar.get("fin", 0, B).view(-1), int(ar.get("step", 0, 1)),
            ar.get("logp", st + 1, 1).view(-1) if scores else None)


def run_case(L, dev, sync, f16, scores, inputs, st, gc, op_ngram=3, fbos=BOS, feos=EOS, max_new=GMAX_NEW, slack=0, what="case"):
    """launch + compare with `expect`: token equal, logp inside the bound (exactly 0.0 where hf's is), bookkeeping, nothing but
    column st + 1 of ids changed.  Returns (tokens, processed scores, worst logp error as a fraction of its bound)."""
    dtype = L.F16 if f16 else L.F32
    ids, logits, bias, fin = inputs
    V = logits.shape[1]
    toks, lps, fin_r, bounds, proc = expect(logits, bias, ids, fin, st, max_new, op_ngram, fbos, feos, gc)
    block = gc.pack(V, fbos)
    got_ids, got_fin, got_step, got_lp = launch(L, dev, sync, dtype, logits, bias, ids, fin, st, max_new, op_ngram, fbos, feos, scores,
                                                block, slack, what)
    assert got_ids[:, st + 1].tolist() == toks, (what, st, got_ids[:, st + 1].tolist(), toks)
    keep = torch.ones(ids.shape[1], dtype=torch.bool); keep[st + 1] = False
    assert torch.equal(got_ids[:, keep], ids[:, keep]), f"{what}: ids outside the written column changed"
    assert torch.equal(got_fin, fin_r) and got_step == st + 1, what
    worst = 0.0
    if scores:
        for b in range(ids.shape[0]):
            got = float(got_lp[b])
            if lps[b] == 0.0:
                assert got == 0.0, (what, st, b, got)
            else:
                err = abs(got - lps[b])
                print(f"{what} step {st} row {b}: logp {got:.6f} vs {lps[b]:.6f}: {err:.3e} (bound {bounds[b]:.3e})")
                assert err <= bounds[b], f"{what} step {st} row {b}: {got} vs {lps[b]}: {err:.3e} > {bounds[b]:.3e}"
                worst = max(worst, err / bounds[b])
    return toks, proc, worst


def base_inputs(V, f16, seed=0):
    """long_greedy_inputs (B = 4, T = 130, 122 tokens of history; row 2 finished) with the scripted row's positive top value"""
    tdt = torch.float16 if f16 else torch.float32
    ids, logits, bias, fin, xs = LC.long_greedy_inputs(V, tdt, seed)
    logits = logits.float()
    top = float((logits + bias).max())
    assert top > 1.0
    return ids, logits, bias, fin, xs, top, tdt


def _set(logits, bias, row, tok, value):
    logits[row, tok] = value - float(bias[tok])


def _raw_top(logits, bias, row, tdt):
    return int(torch.argmax(logits[row].to(tdt).float() + bias))


# ---------------------------------------------------------------------------------------------- the cases
def check_repetition_penalty(L, dev, V, f16, scores, sync=lambda: None):
    """row 1: the seen set holds 0, V - 1, 64, 65 (two bits of one word) with positive and negative scores, and token 500 three
    times, the row's raw maximum at 2 top — divided once by 1.3 it falls behind the unseen token 700 at 1.7 top (three divisions
    would change nothing here, so row 3 covers "once": its token 93 occurs 41 times at 2 top against the unseen 701 at 1.2 top and
    still wins).  Penalty 0.8 rewards repeats: the seen maximum grows."""
    ids, logits, bias, fin, xs, top, tdt = base_inputs(V, f16)
    for pos, tok in ((5, 0), (17, V - 1), (40, 64), (41, 65), (60, 500), (77, 500), (101, 500)):
        ids[FREE, pos] = tok
    for tok, val in ((0, 0.6 * top), (V - 1, -4.0), (64, 0.7 * top), (65, -2.5), (500, 2.0 * top), (700, 1.7 * top)):
        _set(logits, bias, FREE, tok, val)
    assert 93 not in xs[3] and 701 not in xs[3]
    _set(logits, bias, 3, 93, 2.0 * top + 30.0)          # above the scripted (banned) followers of row 3, which reach top + 21.5
    _set(logits, bias, 3, 701, (2.0 * top + 30.0) / 1.3 ** 2)
    inputs = (ids, logits.to(tdt).contiguous(), bias, fin)
    assert _raw_top(logits, bias, FREE, tdt) == 500
    toks, proc, worst = run_case(L, dev, sync, f16, scores, inputs, GSTEP, controls(repetition_penalty=1.3), what="penalty 1.3")
    assert toks[FREE] == 700 and toks[3] == 93, toks
    assert float(proc[FREE, V - 1]) < -4.5 and float(proc[FREE, 64]) < 0.6 * top       # multiplied / divided
    toks8, proc8, w8 = run_case(L, dev, sync, f16, scores, inputs, GSTEP, controls(repetition_penalty=0.8), what="penalty 0.8")
    assert toks8[FREE] == 500 and float(proc8[FREE, 500]) > 2.4 * top
    return max(worst, w8)


def check_min_new_tokens(L, dev, V, f16, scores, sync=lambda: None):
    """EOS is the scripted row's maximum at step 121 (cur_len - 1 = 121): min_new_tokens = 122 bans it, 121 allows it"""
    ids, logits, bias, fin, xs, top, tdt = base_inputs(V, f16)
    _set(logits, bias, FREE, EOS, 2.0 * top)
    inputs = (ids, logits.to(tdt).contiguous(), bias, fin)
    banned, _, w0 = run_case(L, dev, sync, f16, scores, inputs, GSTEP, controls(min_new_tokens=GSTEP + 1), what="min_new 122")
    allowed, _, w1 = run_case(L, dev, sync, f16, scores, inputs, GSTEP, controls(min_new_tokens=GSTEP), what="min_new 121")
    assert banned[FREE] != EOS and allowed[FREE] == EOS
    return max(w0, w1)


def check_suppress(L, dev, V, f16, scores, sync=lambda: None):
    """suppress {0, V - 1, 64, 65}, the four largest entries of the scripted row; at the begin index (2 behind the forced BOS) and
    one step later for begin_suppress_tokens"""
    ids, logits, bias, fin, xs, top, tdt = base_inputs(V, f16)
    four = [0, V - 1, 64, 65]
    for k, tok in enumerate(four):
        _set(logits, bias, FREE, tok, top + 1.0 + k)
    inputs = (ids, logits.to(tdt).contiguous(), bias, fin)
    toks, _, worst = run_case(L, dev, sync, f16, scores, inputs, GSTEP, controls(suppress_tokens=four), what="suppress")
    assert _raw_top(logits, bias, FREE, tdt) == 65 and toks[FREE] not in four
    at, _, w1 = run_case(L, dev, sync, f16, scores, inputs, 1, controls(begin_suppress_tokens=four), what="begin-suppress at")
    after, _, w2 = run_case(L, dev, sync, f16, scores, inputs, 2, controls(begin_suppress_tokens=four), what="begin-suppress after")
    assert at[FREE] not in four and after[FREE] == 65
    first, _, w3 = run_case(L, dev, sync, f16, scores, inputs, 0, controls(begin_suppress_tokens=four), fbos=-1, what="begin-suppress, no forced BOS")
    second, _, w4 = run_case(L, dev, sync, f16, scores, inputs, 1, controls(begin_suppress_tokens=four), fbos=-1, what="begin-suppress + 1, no forced BOS")
    assert first[FREE] not in four and second[FREE] == 65
    return max(worst, w1, w2, w3, w4)


def check_bad_words(L, dev, V, f16, scores, sync=lambda: None):
    """the scripted row ends in ..., 220, 221.  [221, A] and [220, 221, B] match and ban A and B, [221, D] shares the prefix and
    bans D, [222, C] does not match: C wins.  At step 0 (history = one token) a 2-token and a 3-token sequence are both longer
    than the history and ban nothing.  64 sequences of 8 tokens whose prefixes are the row's last 7 tokens ban the row's 64
    largest entries."""
    ids, logits, bias, fin, xs, top, tdt = base_inputs(V, f16)
    assert ids[FREE, GSTEP - 1] == 220 and ids[FREE, GSTEP] == 221
    A, Bt, D, C = 600, 601, 602, 603
    for tok, val in ((A, top + 4.0), (Bt, top + 3.0), (D, top + 2.0), (C, top + 1.0)):
        _set(logits, bias, FREE, tok, val)
    inputs = (ids, logits.to(tdt).contiguous(), bias, fin)
    gc = controls(bad_words_ids=[[221, A], [220, 221, Bt], [222, C], [221, D]])
    toks, proc, worst = run_case(L, dev, sync, f16, scores, inputs, GSTEP, gc, what="bad words")
    assert toks[FREE] == C and all(float(proc[FREE, t]) == float("-inf") for t in (A, Bt, D))
    first = int(ids[FREE, 0])
    gc0 = controls(bad_words_ids=[[first, A], [7, first, Bt]])
    toks0, _, w0 = run_case(L, dev, sync, f16, scores, inputs, 0, gc0, fbos=-1, what="bad words longer than the history")
    assert toks0[FREE] == A
    order = torch.argsort(logits[FREE].to(tdt).float() + bias, descending=True).tolist()
    tail = ids[FREE, GSTEP - 6:GSTEP + 1].tolist()
    gc64 = controls(bad_words_ids=[tail + [t] for t in order[:64]])
    assert len(gc64.bad_words_ids) == 64 and int(gc64.pack(V, BOS)[5]) == 9
    toks64, _, w64 = run_case(L, dev, sync, f16, scores, inputs, GSTEP, gc64, what="64 bad words of 8 tokens")
    assert toks64[FREE] == order[64]
    return max(worst, w0, w64)


def check_ngram_from_block(L, dev, V, f16, scores, sync=lambda: None):
    """the op's i5 is 3.  Block 2: the scripted row holds (.., 221, Z) earlier and ends in (220, 221), so only the 2-gram rule
    bans Z, its maximum; block -1: the op's 3 (rows 0 and 3 lose their 40 followers, Z wins row 1); block 0: nothing is banned
    (row 0's largest follower wins)."""
    ids, logits, bias, fin, xs, top, tdt = base_inputs(V, f16)
    Z = 610
    ids[FREE, 50], ids[FREE, 51] = 221, Z
    _set(logits, bias, FREE, Z, top + 1.0)
    inputs = (ids, logits.to(tdt).contiguous(), bias, fin)
    two, _, w2 = run_case(L, dev, sync, f16, scores, inputs, GSTEP, controls(no_repeat_ngram_size=2), what="ngram 2 from the block")
    dflt, _, w3 = run_case(L, dev, sync, f16, scores, inputs, GSTEP, controls(), what="ngram -1: the op's 3")
    off, _, w0 = run_case(L, dev, sync, f16, scores, inputs, GSTEP, controls(no_repeat_ngram_size=0), what="ngram 0 from the block")
    assert two[FREE] != Z and dflt[FREE] == Z and off[FREE] == Z
    assert dflt[0] not in xs[0] and two[0] not in xs[0] and off[0] == xs[0][-1]
    return max(w2, w3, w0)


def everything(V, A=600, Bt=601):
    return controls(repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=GSTEP + 1, suppress_tokens=[V - 1, 64, 65],
                    begin_suppress_tokens=[64, 700], bad_words_ids=[[221, A], [220, 221, Bt], [5]])


def check_everything_and_forced(L, dev, V, f16, scores, sync=lambda: None):
    """every control at once at step 121, with the control block's slack (poison words inside i12, as in a plan's buffer); then the
    forced BOS step (0) and the forced EOS step (max_new - 1) with the same controls: the forced token, logp exactly 0.0; the
    finished row 2 emits pad with logp 0.0 in every launch"""
    ids, logits, bias, fin, xs, top, tdt = base_inputs(V, f16)
    for tok, val in ((EOS, 2.0 * top), (600, top + 4.0), (601, top + 3.0), (V - 1, top + 2.5), (5, top + 2.0), (500, 1.9 * top)):
        _set(logits, bias, FREE, tok, val)
    ids[FREE, 60] = 500
    inputs = (ids, logits.to(tdt).contiguous(), bias, fin)
    gc = everything(V)
    toks, proc, worst = run_case(L, dev, sync, f16, scores, inputs, GSTEP, gc, slack=POISON_WORDS, what="everything")
    assert toks[FREE] not in (EOS, 600, 601, V - 1, 5) and toks[2] == PAD
    for st, tok in ((0, BOS), (GMAX_NEW - 1, EOS)):
        forced, _, _ = run_case(L, dev, sync, f16, scores, inputs, st, gc, what=f"forced step {st}")
        assert forced == [tok, tok, PAD, tok]
    at, _, w1 = run_case(L, dev, sync, f16, scores, inputs, 1, gc, what="everything at the begin index")
    return max(worst, w1)


def check_degenerate_rows(L, dev, V, sync=lambda: None):
    """an all-NaN row, an all -inf row and a row whose only finite entries (64, 65) are suppressed: token 0, in range, with and
    without p4; the ordinary row next to them keeps its token"""
    ids = torch.arange(GB * GT, dtype=torch.int32).view(GB, GT) % (V - 10) + 3
    ids[:, 0] = START
    logits = torch.randn(GB, V, generator=torch.Generator().manual_seed(0))
    logits[1] = float("nan")
    logits[2] = float("-inf")
    logits[3] = float("-inf")
    logits[3, 64], logits[3, 65] = 1.0, 2.0
    fin = torch.zeros(GB, dtype=torch.int32)
    gc = controls(repetition_penalty=1.3, suppress_tokens=[64, 65])
    want0 = expect(logits, None, ids, fin, 50, GMAX_NEW, 3, -1, -1, gc)[0][0]
    for scores in (False, True):
        got, _, _, lp = launch(L, dev, sync, L.F32, logits, None, ids, fin, 50, GMAX_NEW, 3, -1, -1, scores, gc.pack(V, -1), what="degenerate")
        new = got[:, 51].tolist()
        assert new == [want0, 0, 0, 0], new


def check_neutral_equals_greedy_step(L, dev, V, f16, sync=lambda: None):
    """a neutral block (penalty 1.0, n-gram -1, nothing else) against OMNI_OP_GREEDY_STEP on the same operands: ids, finished, step
    and the BITS of logp, at max_new = 16 (there OMNI_OP_GREEDY_STEP runs its list form) and at max_new = 129 (its bitmap form)"""
    ids, logits, bias, fin, xs, top, tdt = base_inputs(V, f16)
    dtype = L.F16 if f16 else L.F32
    logits = logits.to(tdt).contiguous()
    neutral = controls(repetition_penalty=1.0, suppress_tokens=[], begin_suppress_tokens=[], bad_words_ids=[], min_new_tokens=0)
    assert neutral.neutral
    block = neutral.pack(V, BOS)
    for max_new, T, st in ((16, 17, 13), (GMAX_NEW, GT, GSTEP)):
        # at T = 17 the history (a, b, x1, a, b, x2, ..., a, b) still ends in a repeated 2-gram prefix: rows 0 and 3 ban four followers
        sub = ids[:, :T].contiguous()
        for scores in (False, True):
            a = launch(L, dev, sync, dtype, logits, bias, sub, fin, st, max_new, 3, BOS, EOS, scores, None, what="greedy_step")
            b = launch(L, dev, sync, dtype, logits, bias, sub, fin, st, max_new, 3, BOS, EOS, scores, block, what="neutral block")
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2] == st + 1, (max_new, scores)
            if scores:
                assert torch.equal(a[3].view(torch.int32), b[3].view(torch.int32)), f"max_new {max_new}: logp bits differ"
        assert int(a[0][0, st + 1]) not in xs[0][:4]
    assert int(a[0][0, GSTEP + 1]) not in xs[0]                       # the bans were live: row 0's 40 largest entries are its followers


def check_short_block(L, dev, V, sync=lambda: None):
    """a block whose header claims two bad-word sequences of stride 3 with an i12 that ends behind the bitmaps, and an i12 that does
    not even hold the bitmaps: OMNI_E_ARG from omni_op_launch (a host-side argument check; nothing is launched, nothing written)"""
    ids, logits, bias, fin, xs, top, tdt = base_inputs(V, False)
    gc = controls(bad_words_ids=[[221, 600], [221, 601]])
    block = gc.pack(V, BOS)
    nw = (V + 31) // 32
    assert block.numel() == 8 + 2 * nw + 6 and block[4:6].tolist() == [2, 3]
    d = {"logits": logits.to(dev), "bias": bias.to(dev), "ids": ids.to(dev), "fin": fin.to(dev),
         "step": torch.tensor([GSTEP], dtype=torch.int32, device=dev), "ctrl": block.to(dev)}
    sync()
    ptrs = {k: v.data_ptr() for k, v in d.items()}
    seen = []
    for nbytes in ((8 + 2 * nw) * 4, (8 + 2 * nw + 5) * 4, (8 + nw) * 4, 0):
        op = ctrl_op(L, L.F32, ptrs, GB, V, GT, GMAX_NEW, 3, BOS, EOS, nbytes)
        rc = L.lib().omni_op_launch(ctypes.byref(op), L._stream_ptr(None))
        assert rc == -1, (nbytes, rc)                                 # OMNI_E_ARG
        seen.append(L.lib().omni_last_error().decode())
    sync()
    assert torch.equal(d["ids"].cpu(), ids) and int(d["step"].cpu()) == GSTEP
    op = ctrl_op(L, L.F32, ptrs, GB, V, GT, GMAX_NEW, 3, BOS, EOS, block.numel() * 4)
    L.launch(op)                                                      # the full size is accepted
    sync()
    assert int(d["step"].cpu()) == GSTEP + 1
    return seen


# ---------------------------------------------------------------------------------------------- host side
def check_packed_block(V=1037):
    """the packed block of a known setting, word for word, against include/omni_amd.h"""
    import struct
    gc = controls(repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=12, suppress_tokens=[0, V - 1, 64, 65],
                  begin_suppress_tokens=[31, 32], bad_words_ids=[[7], [221, 600], [220, 221, 601], [7]])
    w = gc.pack(V, forced_bos=0)
    nw = (V + 31) // 32
    assert w.dtype == torch.int32 and w.numel() == 8 + 2 * nw + 2 * 4
    u = [int(x) & 0xFFFFFFFF for x in w.tolist()]
    assert u[0] == struct.unpack("<I", struct.pack("<f", 1.3))[0]
    assert w[1:8].tolist() == [2, 12, 2, 2, 4, 0, 0]
    supp = u[8:8 + nw]
    want = [0] * nw
    for t in (0, V - 1, 64, 65, 7):
        want[t >> 5] |= 1 << (t & 31)
    assert supp == want and supp[2] == 3
    beg = u[8 + nw:8 + 2 * nw]
    assert beg[0] == 1 << 31 and beg[1] == 1 and sum(beg) == (1 << 31) + 1
    assert w[8 + 2 * nw:].tolist() == [2, 221, 600, 0, 3, 220, 221, 601]
    n = controls().pack(V, forced_bos=-1)
    assert n.numel() == 8 + 2 * nw and [int(x) & 0xFFFFFFFF for x in n[:8].tolist()] == [0x3F800000, 0xFFFFFFFF, 0, 1, 0, 0, 0, 0]
    assert int(n[8:].abs().sum()) == 0
    from omniparser_amd.florence import gen_ctrl_words
    assert gen_ctrl_words(V) == 8 + 2 * nw + 64 * 9


# ---------------------------------------------------------------------------------------------- whole captioner vs transformers
N_CROPS, SEED, MAX_NEW, R = 4, 403, 32, 64
SETTING_NAMES = ("repetition_penalty", "min_new_tokens", "suppress_tokens", "begin_suppress_tokens", "bad_words_ids",
                 "no_repeat_ngram_size", "all")
# the combined setting has its own seed: with seed 403 the oracle's smallest top-1 / top-2 gap on the stock checkpoint is 8.2e-5, below
# beam_checks.MARGIN (the reference alone could then not hold a cap of 0 excused rows).  404 is the first seed after it whose
# gaps are above the margin on both checkpoints (3.4e-4 stock, 5.2e-4 EOS-prone; transformers on the CPU); 4 rows change on both
SEED_OF = {"all": 404}
_ORACLE, _CAPS = {}, {}


def pixels(seed=SEED):
    return torch.randn(N_CROPS, 3, R, R, generator=torch.Generator().manual_seed(seed))


def _hf(model, pix, **kw):
    from omniparser_amd.florence import PROMPT_IDS
    cfg = model.config
    n_img = (pix.shape[-1] // 32) ** 2 + 1
    inp = torch.tensor([[cfg.image_token_id] * n_img + PROMPT_IDS] * pix.shape[0])
    with torch.inference_mode():
        out = model.generate(input_ids=inp, pixel_values=pix, max_new_tokens=MAX_NEW, num_beams=1, do_sample=False,
                             output_scores=True, return_dict_in_generate=True, **kw)
        ts = model.compute_transition_scores(out.sequences, out.scores, normalize_logits=True)
    gaps = []
    for s in out.scores:
        top = s.double().topk(2, dim=-1).values
        g = top[:, 0] - top[:, 1]
        g[~torch.isfinite(g)] = float("inf")                  # a forced position is no decision
        gaps.append(g)
    return out.sequences, ts.double(), torch.stack(gaps, 1)


def settings_for(eos_prone, seed=SEED):
    """the seven settings; t = the token the oracle's default output (on the pixels of `seed`) repeats most, u = its second most
    frequent one (no special token)"""
    import beam_checks as BC
    seq = oracle(eos_prone, "default", seed)[0]
    eos = BC.EOS_PRONE_TOKEN if eos_prone else 2
    counts = {}
    for tok in seq[:, 1:].flatten().tolist():
        if tok not in (0, 1, 2, eos):
            counts[tok] = counts.get(tok, 0) + 1
    ranked = sorted(counts, key=lambda k: (-counts[k], k))
    t, u = ranked[0], ranked[1]
    s = {"repetition_penalty": dict(repetition_penalty=1.3), "min_new_tokens": dict(min_new_tokens=12),
         "suppress_tokens": dict(suppress_tokens=[t]), "begin_suppress_tokens": dict(begin_suppress_tokens=[t]),
         "bad_words_ids": dict(bad_words_ids=[[t, t], [u]]), "no_repeat_ngram_size": dict(no_repeat_ngram_size=2)}
    s["all"] = {k: v for d in s.values() for k, v in d.items()}
    return s


def oracle(eos_prone, name, seed=None):
    """transformers on the CPU, computed once per (checkpoint, setting, seed): (sequences, transition scores, gaps); the seed of a
    setting is SEED_OF's or SEED, "default" takes the one asked for"""
    import beam_checks as BC
    seed = SEED_OF.get(name, SEED) if seed is None else seed
    key = (eos_prone, name, seed)
    if key not in _ORACLE:
        kw = {} if name == "default" else settings_for(eos_prone, seed)[name]
        model = BC.oracle_model(0, eos_prone)
        try:
            _ORACLE[key] = _hf(model, pixels(seed), **kw)
        finally:
            model.generation_config.eos_token_id = 2
    return _ORACLE[key]


def captioner(eos_prone):
    import beam_checks as BC
    from omniparser_amd.florence import Florence2Captioner
    from tools.make_weights import ensure_caption_checkpoint
    if eos_prone not in _CAPS:
        d = BC.eos_prone_checkpoint(0) if eos_prone else ensure_caption_checkpoint(0)
        _CAPS[eos_prone] = Florence2Captioner(d, "cuda", precision="f32", resolution=R)
    return _CAPS[eos_prone]


def captioner_vs_hf(eos_prone, name, device_pixels=False, cap=None):
    """generate(**setting, output_scores=True) against transformers with the same setting: no row excused; the largest |delta logp|
    is printed, then held to long_checks.TOL_LOGP_LONG.  Returns (largest |delta logp|, rows in which the reference differs from
    the reference's default output)."""
    import beam_checks as BC
    seed = SEED_OF.get(name, SEED)
    ref_seq, ref_ts, gaps = oracle(eos_prone, name)
    dflt = oracle(eos_prone, "default", seed)[0]
    kw = settings_for(eos_prone, seed)[name]
    cap = cap or captioner(eos_prone)
    pix = pixels(seed)
    out = cap.generate(pixel_values=pix.cuda() if device_pixels else pix, max_new_tokens=MAX_NEW, output_scores=True,
                       return_dict_in_generate=True, **kw)
    eos = BC.EOS_PRONE_TOKEN if eos_prone else 2
    worst, _ = SC.compare_with_hf(out.sequences, out.token_logprobs, ref_seq, ref_ts, gaps, eos, cap.w.pad, float("inf"), max_excused=0)
    changed = rows_changed(ref_seq, dflt, cap.w.pad)
    finite = gaps[torch.isfinite(gaps)]
    print(f"controls vs transformers: eos_prone={eos_prone} {name} seed {seed} {kw}: max |dlogp| = {worst:.3e}, smallest oracle gap "
          f"{float(finite.min()):.3e}, {changed} rows differ from the default output")
    assert float(finite.min()) >= BC.MARGIN, "the oracle's own gap is below the margin: choose another seed for this setting"
    SC.compare_with_hf(out.sequences, out.token_logprobs, ref_seq, ref_ts, gaps, eos, cap.w.pad, LC.TOL_LOGP_LONG, max_excused=0)
    return worst, changed


def rows_changed(a, b, pad):
    T = max(a.shape[1], b.shape[1])
    padto = lambda t: torch.nn.functional.pad(t, (0, T - t.shape[1]), value=pad)
    return int((padto(a) != padto(b)).any(1).sum())


def check_not_vacuous(names=SETTING_NAMES):
    """for every setting the REFERENCE output differs from the reference default output in at least one row on at least one of the
    two checkpoints"""
    for name in names:
        changed = [rows_changed(oracle(ep, name)[0], oracle(ep, "default", SEED_OF.get(name, SEED))[0], 1) for ep in (False, True)]
        print(f"{name}: rows changed (stock, EOS-prone) = {changed}")
        assert max(changed) >= 1, name


# ---------------------------------------------------------------------------------------------- plans and defaults
def check_plans_and_defaults(cap, device_pixels=False, MAX_NEW=MAX_NEW, n_boxes=5):
    """controls do not leak into the next call, every setting runs on ONE controls plan, default and neutral calls take the default
    plan and build no controls plan, caption_crops(controls=...) equals generate on the same pixels.  Starts from an empty plan
    cache (the captioner may have served other tests)."""
    import gpu_checks as G
    pix = pixels()
    px = pix.cuda() if device_pixels else pix
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    cap.clear_plans()
    has_ctrl = lambda: [k for k in cap._plans if "controls" in k]
    first = cap.generate(pixel_values=px, max_new_tokens=MAX_NEW)
    assert not has_ctrl(), "a default call built a controls plan"
    n_plans = len(cap._plans)
    if n_boxes:                                                       # (not on the emulated twin: every call is an emulated encode)
        neutral = cap.generate(pixel_values=px, max_new_tokens=MAX_NEW, repetition_penalty=1.0, suppress_tokens=[], begin_suppress_tokens=[],
                               bad_words_ids=[], min_new_tokens=0)
        assert torch.equal(neutral, first) and not has_ctrl() and len(cap._plans) == n_plans
    assert cap.generation_controls(dict(repetition_penalty=1.0, suppress_tokens=[], begin_suppress_tokens=[], bad_words_ids=[],
                                        min_new_tokens=0), MAX_NEW) is None     # neutral controls ARE the default call
    a = cap.generate(pixel_values=px, max_new_tokens=MAX_NEW, repetition_penalty=1.3)
    assert len(has_ctrl()) == 1
    plan = cap._plans[has_ctrl()[0]]
    assert plan is cap.plans(cap.bucket(N_CROPS), R, MAX_NEW, controls=True)
    kinds = [op.kind for op in plan.step_plan.ops]
    assert kinds[-1] == cap_lib().OP_GREEDY_CTRL_STEP and cap_lib().OP_GREEDY_STEP not in kinds
    dflt_plan = cap.plans(cap.bucket(N_CROPS), R, MAX_NEW)
    assert [op.kind for op in dflt_plan.step_plan.ops][-1] == cap_lib().OP_GREEDY_STEP and dflt_plan.ctrl is None
    nbytes = cap.plan_cache_bytes()
    tok = int(first[0, 2])
    b = cap.generate(pixel_values=px, max_new_tokens=MAX_NEW, suppress_tokens=[tok], min_new_tokens=3)
    assert len(has_ctrl()) == 1 and cap._plans[has_ctrl()[0]] is plan and cap.plan_cache_bytes() == nbytes
    assert rows_changed(a, first, cap.w.pad) >= 1, "the penalty changed nothing"
    assert not bool((b[:, 1:] == tok).any())
    again = cap.generate(pixel_values=px, max_new_tokens=MAX_NEW)
    assert torch.equal(again, first), "controls leaked into the next default call"
    if not n_boxes:                                                   # the emulated twin stops here: every call is an emulated encode
        return first, a, b
    a2 = cap.generate(pixel_values=px, max_new_tokens=MAX_NEW, repetition_penalty=1.3)
    assert torch.equal(a2, a), "a setting depends on the one that ran before it"
    # caption_crops on a frame = generate on the pixels the crop op produced
    from omniparser_amd.florence import GenerationControls
    from omniparser_amd.synth import synthetic_screenshot
    frame = torch.from_numpy(synthetic_screenshot(5))
    frame = frame.cuda() if device_pixels else frame
    boxes = G.real_crop_boxes(5, n_boxes)
    cp = cap.plans(cap.bucket(len(boxes)), R, MAX_NEW)
    G._fill_rows(cap, cp, frame, boxes, list(range(len(boxes))))
    crop_px = cp.x_in.t[:len(boxes), :, :, :3].permute(0, 3, 1, 2).float().clone()
    kw = dict(repetition_penalty=1.3, bad_words_ids=[[tok]])
    want = cap.generate(pixel_values=crop_px, max_new_tokens=MAX_NEW, output_scores=True, return_dict_in_generate=True, **kw)
    got = cap.caption_crops(frame, boxes, max_new_tokens=MAX_NEW, controls=kw)
    got2, lp2 = cap.caption_crops(frame, boxes, max_new_tokens=MAX_NEW, controls=GenerationControls(**kw), return_scores=True)
    assert torch.equal(got, want.sequences) and torch.equal(got2, got) and torch.equal(lp2, want.token_logprobs)
    assert torch.equal(cap.caption_crops(frame, boxes, max_new_tokens=MAX_NEW, controls={}), cap.caption_crops(frame, boxes, max_new_tokens=MAX_NEW))
    return first, a, b


def cap_lib():
    from omniparser_amd import _lib as L
    return L

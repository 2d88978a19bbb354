"""Long-form greedy decoding checks shared by the CPU (emulation) and GPU tests: the long-history form of OMNI_OP_GREEDY_STEP
(greedy_step_long_kernel: an exact n-gram ban for any history), the split-key self-attention of OMNI_OP_ATTN_DECODE
(attn_decode_self_kernel) and Florence2Captioner.generate(max_new_tokens=128) against transformers on the CPU.

Bounds: the greedy kernel's log-probability is held to score_checks' derived two-pass bound, the attention output to
caption_f64.bound("attn_decode" / "attn_decode_sharp") — the bound of the four-wave cross kernel at 585 keys; a softmax-weighted
mean does not grow in error with the key count.  The model tolerance TOL_LOGP_LONG is 5 x the largest |delta logp| measured
(profiles/long_decode_tolerance.json)."""
import torch

import caption_f64 as CF
import plan_interp as PI
import score_checks as SC

F64 = torch.float64
START, PAD, EOS, BOS = SC.START, SC.PAD, SC.EOS, SC.BOS

# |token_logprobs - transformers| of generate(max_new_tokens=128, output_scores=True), f32 plans, 64x64 crops, stand-in checkpoints
# (cases 1 and 2 of `captioner_long_vs_hf`): largest value measured, times the project's factor 5.
MEASURED_MAX_DLOGP_LONG = {"emulation": 1.526e-05, "mi355x": 2.766e-05}      # emulation: case 2 only (case 1 is 128 emulated steps)
TOL_LOGP_LONG = 5.0 * max(MEASURED_MAX_DLOGP_LONG.values())

# ---------------------------------------------------------------------------------------------- greedy kernel
GB, GT, GMAX_NEW, GSTEP = 4, 130, 129, 121
N_REP = 40


def _followers(V, seed, repeated):
    """40 followers: token 0, token V - 1, two tokens of one 32-bit bitmap word (64, 65), the rest seeded and distinct; `repeated`
    makes the second equal to the first (a follower that occurs twice)."""
    g = torch.Generator().manual_seed(seed)
    pool = [int(t) for t in torch.randperm(V - 200, generator=g)[:N_REP + 8] + 100]
    xs = [0, V - 1, 64, 65] + [t for t in pool if t not in (0, V - 1, 64, 65)][:N_REP - 4]
    order = [int(i) for i in torch.randperm(N_REP, generator=g)]
    xs = [xs[i] for i in order]
    if repeated:
        xs[1] = xs[0]
    return xs


def long_greedy_inputs(V, tdt, seed=0):
    """ids [4, 130] (122 tokens of history each, positions beyond seeded), logits [4, V] in `tdt`, bias [V], finished [4]:
    row 0: (a, b, x_i) x 40 then a, b; the 40 largest processed entries are exactly the distinct x_i, growing with i (x_40 the largest)
    row 1: distinct tokens, nothing banned
    row 2: finished
    row 3: as row 0 with its own a, b, x_i, of which x_2 == x_1 (40 start positions cannot hold 40 distinct followers AND a repeated
           one, so the repeated follower lives here; every launch covers all four rows)."""
    g = torch.Generator().manual_seed(seed + 7)
    cur = GSTEP + 1
    assert cur == 3 * N_REP + 2
    ids = torch.randint(3, V, (GB, GT), generator=g, dtype=torch.int32)
    logits = torch.randn(GB, V, generator=g) * 3.0
    bias = torch.randn(V, generator=g) * 0.5
    top = float((logits + bias).max())
    xs_rows = {}
    for row, (a, b, rep) in {0: (91, 92, False), 3: (93, 94, True)}.items():
        xs = _followers(V, seed + row, rep)
        assert a not in xs and b not in xs
        hist = []
        for x in xs:
            hist += [a, b, x]
        hist += [a, b]
        ids[row, :cur] = torch.tensor(hist, dtype=torch.int32)
        for i, x in enumerate(xs):
            logits[row, x] = top + 2.0 + 0.5 * i - float(bias[x])
        xs_rows[row] = xs
    ids[1, :cur] = torch.arange(100, 100 + cur, dtype=torch.int32)
    ids[2, :cur] = torch.arange(300, 300 + cur, dtype=torch.int32)
    fin = torch.zeros(GB, dtype=torch.int32)
    fin[2] = 1
    return ids, logits.to(tdt).contiguous(), bias, fin, xs_rows


def expect_greedy(logits, bias, ids, fin, st, max_new, ngram, fbos, feos):
    """(tokens, logp, finished after, per-row bound) of one step from the f64 processed scores (transformers' processors)"""
    B, V = logits.shape
    lsm, proc = SC.processed_logprobs_f64(logits, bias, ids[:, :st + 1].long(), ngram, fbos, feos, max_new + 1)
    forced = (fbos >= 0 and st == 0) or (feos >= 0 and st + 1 == max_new)
    toks, lps, bounds, fin2 = [], [], [], fin.clone()
    for b in range(B):
        tok = int(torch.argmax(proc[b]))
        finite = proc[b][torch.isfinite(proc[b])]
        bounds.append(2.0 ** -23 * (V / 256 + 16) + 4 * SC.ulp_f32(float(finite.abs().max())))
        lp = 0.0 if forced else float(lsm[b, tok])
        if fin[b]:
            tok, lp = PAD, 0.0
        elif tok == EOS:
            fin2[b] = 1
        toks.append(tok); lps.append(lp)
    return toks, lps, fin2, bounds


def launch_greedy(L, dev, sync, dtype, logits, bias, ids, fin, st, T, max_new, ngram, fbos, feos, scores):
    B, V = logits.shape
    d = {"logits": logits.to(dev), "bias": bias.to(dev) if bias is not None else None, "ids": ids.to(dev), "fin": fin.to(dev),
         "step": torch.tensor([st], dtype=torch.int32, device=dev), "logp": torch.zeros(B, T, device=dev) if scores else None}
    L.launch(SC.greedy_op(L, dtype, d["logits"], d["bias"], d["ids"], d["fin"], d["step"], d["logp"], B, V, T, max_new, ngram, fbos, feos))
    sync()
    return d["ids"].cpu(), d["fin"].cpu(), int(d["step"].cpu()), (d["logp"].cpu() if scores else None)


def check_greedy_long(L, dev, V, f16, scores, sync=lambda: None):
    """the launches of the long-history form on `long_greedy_inputs`: (ngram 3, step 121), (ngram 2, step 121), (ngram 3, forced EOS
    at step max_new - 1), (ngram 0: the list form, nothing banned).  Token = arg-max of the f64 processed scores, logp inside the
    derived bound, finished / step bookkeeping, nothing else of ids changed.  Returns the worst logp error as a fraction of its bound."""
    dtype, tdt = (L.F16, torch.float16) if f16 else (L.F32, torch.float32)
    ids, logits, bias, fin, xs = long_greedy_inputs(V, tdt)
    worst = 0.0
    for ngram, st, fbos, feos in ((3, GSTEP, BOS, EOS), (2, GSTEP, BOS, EOS), (3, GMAX_NEW - 1, BOS, EOS), (0, GSTEP, -1, -1)):
        toks, lps, fin_r, bounds = expect_greedy(logits, bias, ids, fin, st, GMAX_NEW, ngram, fbos, feos)
        got_ids, got_fin, got_step, got_lp = launch_greedy(L, dev, sync, dtype, logits, bias, ids, fin, st, GT, GMAX_NEW, ngram, fbos, feos, scores)
        assert got_ids[:, st + 1].tolist() == toks, (ngram, st, got_ids[:, st + 1].tolist(), toks)
        keep = torch.ones(GT, dtype=torch.bool); keep[st + 1] = False
        assert torch.equal(got_ids[:, keep], ids[:, keep]), "ids outside the written column changed"
        assert torch.equal(got_fin, fin_r) and got_step == st + 1
        if st == GSTEP and ngram:
            # the scripted rows: every x_i is banned, so the winner is none of them (the 32-slot list lets x_33.. through)
            for row in (0, 3):
                assert toks[row] not in xs[row], (row, toks[row])
        if scores:
            for b in range(GB):
                err = abs(float(got_lp[b, st + 1]) - lps[b])
                if lps[b] == 0.0:
                    assert float(got_lp[b, st + 1]) == 0.0, (ngram, st, b)
                else:
                    assert err <= bounds[b], f"ngram {ngram} step {st} row {b}: {float(got_lp[b, st + 1])} vs {lps[b]}: {err:.3e} > {bounds[b]:.3e}"
                    worst = max(worst, err / bounds[b])
            other = torch.ones(GT, dtype=torch.bool); other[st + 1] = False
            assert torch.equal(got_lp[:, other], torch.zeros(GB, GT - 1)), "logp outside the written column changed"
    return worst


def check_degenerate_rows_long(L, dev, V, sync=lambda: None):
    """all-NaN and all -inf rows on the long-history form (max_new 129, ngram 3): token 0, in range, with and without p4"""
    ids = torch.arange(GB * GT, dtype=torch.int32).view(GB, GT) % (V - 10) + 3
    ids[:, 0] = START
    logits = torch.randn(GB, V, generator=torch.Generator().manual_seed(0))
    logits[1] = float("nan")
    logits[2] = float("-inf")
    fin = torch.zeros(GB, dtype=torch.int32)
    for scores in (False, True):
        got, _, _, lp = launch_greedy(L, dev, sync, L.F32, logits, None, ids, fin, 50, GT, GMAX_NEW, 3, -1, -1, scores)
        new = got[:, 51].tolist()
        assert new == [int(torch.argmax(logits[0])), 0, 0, int(torch.argmax(logits[3]))], new
        if scores:
            for b in (0, 3):
                assert abs(float(lp[b, 51]) - float(torch.log_softmax(logits[b].double(), -1).max())) < 1e-5


def check_routing_boundary(L, dev, V, f16, sync=lambda: None):
    """max_new = 34 (the list form: 32 start positions) and max_new = 35 (the long-history form) with ngram 3 on one history of 31
    tokens with repeated 3-grams: identical ids and finished flags, bit-identical logp"""
    dtype, tdt = (L.F16, torch.float16) if f16 else (L.F32, torch.float32)
    B, T, st = 4, 36, 30
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(3, V, (B, T), generator=g, dtype=torch.int32)
    logits = torch.randn(B, V, generator=g) * 3.0
    bias = torch.randn(V, generator=g) * 0.5
    top = float((logits + bias).max())
    for row in (0, 1):                              # row 0: (a, b, x_i) x 9, a, b, a, b; row 1: the same shifted by one token
        hist = []
        for i in range(9):
            hist += [21, 22, 40 + 37 * i + row]
            logits[row, 40 + 37 * i + row] = top + 1.0 + i
        ids[row, :st + 1] = torch.tensor((hist + [21, 22, 21, 22, 21])[row:row + st + 1], dtype=torch.int32)
    logits = logits.to(tdt).contiguous()
    fin = torch.zeros(B, dtype=torch.int32); fin[3] = 1
    out = {}
    for max_new in (34, 35):
        out[max_new] = launch_greedy(L, dev, sync, dtype, logits, bias, ids, fin, st, T, max_new, 3, BOS, EOS, True)
    a, b = out[34], out[35]
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2]
    assert torch.equal(a[3].view(torch.int32), b[3].view(torch.int32)), "logp differs between the two forms"
    toks, _, _, _ = expect_greedy(logits, bias, ids, fin, st, 35, 3, BOS, EOS)
    assert a[0][:, st + 1].tolist() == toks
    banned = SC.processed_logprobs_f64(logits, bias, ids[:, :st + 1].long(), 3, -1, -1, 36)[1]
    assert int(torch.isinf(banned[0]).sum()) >= 9          # the history did ban something


# ---------------------------------------------------------------------------------------------- self-attention kernel
SELF_CAPS = (65, 130, 1025)
SELF_STEPS = (0, 1, 3, 4, 15, 16, 31, 32, 63, 64, -2, -1)      # negative: cap - 2, cap - 1


def self_steps(cap):
    return sorted({s if s >= 0 else cap + s for s in SELF_STEPS if (s if s >= 0 else cap + s) < cap})


def run_self_attn(L, dev, dtype, cap, st, scale, ldpad=64, seed=0, sync=lambda: None):
    """one OMNI_OP_ATTN_DECODE self-attention launch inside guard bands (caption_f64.Arena): B = 3, 2 heads, cache pitch C + ldpad,
    cache rows >= step NaN.  Asserts the append, the untouched rows and a finite output; returns the worst per-head error relative
    to the f64 reference (caption_f64.seg_err)."""
    B, heads = 3, 2
    C = heads * 64
    tdt = torch.float32 if dtype == L.F32 else torch.float16
    g = torch.Generator().manual_seed(seed)
    R = lambda *s: torch.randn(*s, generator=g)
    sharp = 8.0 if scale == "sharp" else 1.0
    ldo = C + 32
    qoff, koff, voff, ldq = 16, C + 32, 2 * C + 48, 3 * C + 64
    ldc = C + ldpad
    q, kn, vn = (R(B, C) * sharp).to(tdt), R(B, C).to(tdt), R(B, C).to(tdt)
    kc, vc = R(B, cap, C), R(B, cap, C)
    kc[:, st:] = float("nan"); vc[:, st:] = float("nan")
    kc, vc = kc.to(tdt), vc.to(tdt)
    ar = CF.Arena()
    ar.add("o", tdt, B, ldo, out=((0, C),))
    ar.add("qkv", tdt, B, ldq, data=((qoff, q), (koff, kn), (voff, vn)))
    ar.add("kc", tdt, B * cap, ldc, data=((0, kc.view(-1, C)),)).add("vc", tdt, B * cap, ldc, data=((0, vc.view(-1, C)),))
    ar.add("step", torch.int32, 1, 1, data=((0, torch.tensor([[st]], dtype=torch.int32)),))
    ar.build(dev)
    L.launch(L.make_op(L.OP_ATTN_DECODE, dtype, p=[ar.ptr("qkv"), ar.ptr("qkv"), ar.ptr("qkv"), ar.ptr("kc"), ar.ptr("o"), ar.ptr("vc"), ar.ptr("step")],
                       i={0: ldq, 1: qoff, 2: ldq, 3: koff, 4: voff, 5: ldo, 6: heads, 7: 0, 8: cap, 9: C, 10: B, 11: ldc}, f={0: 0.125}))
    sync(); ar.fetch(f"attn_decode_self cap {cap} step {st}")
    what = f"attn_decode self cap {cap} step {st} {scale} pad {ldpad}"
    bits = {2: torch.int16, 4: torch.int32}[kc.element_size()]
    for name, before, new in (("kc", kc, kn), ("vc", vc, vn)):
        after = ar.get(name, 0, C).view(B, cap, C)
        assert torch.equal(after[:, st], new), what + ": cache append"
        assert torch.equal(after[:, :st], before[:, :st]), what + ": cache rows below the step changed"
        assert torch.equal(after[:, st + 1:].view(bits), before[:, st + 1:].view(bits)), what + ": cache rows beyond the step changed"
    o = ar.get("o", 0, C)
    assert bool(torch.isfinite(o).all()), what + ": output not finite (a row beyond the step was read)"
    ref = PI.attn_decode_self_ref(q, kc[:, :st], vc[:, :st], kn, vn, heads, 0.125, F64)
    return CF.seg_err(o, ref, 64)[0]


def check_self_attn(L, dev, dtype, cap, scale, ldpad=64, sync=lambda: None):
    """every step of `self_steps(cap)`: inside caption_f64's decode-attention bound; returns the worst fraction of the bound"""
    bnd = CF.bound("attn_decode_sharp" if scale == "sharp" else "attn_decode", dtype)
    worst = 0.0
    for n, st in enumerate(self_steps(cap)):
        e = run_self_attn(L, dev, dtype, cap, st, scale, ldpad, seed=cap + n, sync=sync)
        print(f"attn_decode self cap={cap} step={st} {scale} pad={ldpad}: {e:.3e} = {e / bnd:.3f} of the bound")
        assert e <= bnd, f"attn_decode self cap {cap} step {st} {scale}: {e:.3e} > {bnd:.1e}"
        worst = max(worst, e / bnd)
    return worst


# ---------------------------------------------------------------------------------------------- whole captioner vs transformers
LONG_CASES = {1: dict(n=4, seed=403, eos_prone=False, max_new=128), 2: dict(n=4, seed=311, eos_prone=True, max_new=128)}


def captioner_long_vs_hf(case, tol=None, device_pixels=False, R=64):
    """generate(max_new_tokens=128, output_scores=True) against transformers on the CPU, no row excused (the oracle's smallest
    top-1 / top-2 gap is above beam_checks.MARGIN in both cases); the sequences also equal generate() without scores.  Prints the
    largest |delta logp| before it is compared.  Returns (captioner, output, largest |delta logp|, reference sequences)."""
    import beam_checks as BC
    from omniparser_amd.florence import Florence2Captioner
    from tools.make_weights import ensure_caption_checkpoint
    c = LONG_CASES[case]
    n, max_new, eos_prone = c["n"], c["max_new"], c["eos_prone"]
    pix = torch.randn(n, 3, R, R, generator=torch.Generator().manual_seed(c["seed"]))
    model = BC.oracle_model(0, eos_prone)
    try:
        ref_seq, ref_ts, gaps = SC.hf_greedy_scores(model, pix, max_new)
        eos = model.generation_config.eos_token_id
    finally:
        model.generation_config.eos_token_id = 2
    d = BC.eos_prone_checkpoint(0) if eos_prone else ensure_caption_checkpoint(0)
    cap = Florence2Captioner(d, "cuda", precision="f32", resolution=R)
    px = pix.cuda() if device_pixels else pix
    out = cap.generate(pixel_values=px, max_new_tokens=max_new, output_scores=True, return_dict_in_generate=True)
    worst, _ = SC.compare_with_hf(out.sequences, out.token_logprobs, ref_seq, ref_ts, gaps, eos, cap.w.pad, float("inf"), max_excused=0)
    lengths = [int((r != cap.w.pad).sum()) - 1 for r in ref_seq]
    print(f"long decode vs transformers: case {case} max_new={max_new}: max |dlogp| = {worst:.3e}, generated lengths {lengths}, "
          f"{cap.last_steps} steps issued")
    SC.compare_with_hf(out.sequences, out.token_logprobs, ref_seq, ref_ts, gaps, eos, cap.w.pad, TOL_LOGP_LONG if tol is None else tol,
                       max_excused=0)
    plain = cap.generate(pixel_values=px, max_new_tokens=max_new)
    assert torch.equal(plain, out.sequences), "generate() without scores gives other sequences"
    return cap, out, worst, ref_seq

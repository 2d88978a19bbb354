"""Closed-vocabulary checks shared by the CPU (emulation) and GPU tests of OMNI_OP_GREEDY_VOCAB_STEP and of
Florence2Captioner.generate(vocabulary=...): the kernel against transformers' own logits processors applied to the f32 scores, the
captioner against transformers' generate(prefix_allowed_tokens_fn=...) on the CPU, and the plan / default-path rules.

Kernel expectation: logits + final_logits_bias in f32, then transformers' NoRepeatNGram, PrefixConstrained (fn = the children of
the row's node), ForcedBOS and ForcedEOS processors in that order, all in f32 — masks and copies, so the token must be EQUAL — then
an f64 log-softmax of those f32 values for the log-probability, held to the per-row bound expression of gen_ctrl_checks.expect
(it over-covers: the kernel sums the allowed children only, not V terms).  transformers requires a non-empty list from fn, so a row
without an allowed token (node -1, a leaf, a node outside the trie) is an all -inf row here, for which every greedy kernel of the
project emits id 0 with an unspecified log-probability.  Edge tokens >= V are no index of the row and are left out of fn's list
(the kernel skips them).  Model tolerance: long_checks.TOL_LOGP_LONG, as it stands."""
import ctypes

import torch

import caption_f64 as CF
import gen_ctrl_checks as GC
import long_checks as LC
import score_checks as SC

START, PAD, EOS, BOS = SC.START, SC.PAD, SC.EOS, SC.BOS
GB, GT, GMAX_NEW, GSTEP = LC.GB, LC.GT, LC.GMAX_NEW, LC.GSTEP
POISON_WORDS = 32          # 0xFF words behind the trie block inside the arena
LOUD = 5                   # a token no test trie allows: the raw top-1 of every row sits here


def vocabulary(labels):
    from omniparser_amd.florence import CaptionVocabulary
    return CaptionVocabulary(labels)


def parse_block(block):
    """(first, edge_tok, edge_dst) of a packed trie block — read from the words, not from the object that packed them"""
    n, e = int(block[0]), int(block[1])
    first = block[8:8 + n + 1].tolist()
    tok = block[8 + n + 1:8 + n + 1 + e].tolist()
    dst = block[8 + n + 1 + e:8 + n + 1 + 2 * e].tolist()
    return first, tok, dst


def edges_of(block, node):
    first, tok, dst = parse_block(block)
    if not 0 <= node < len(first) - 1:
        return {}
    return {tok[k]: dst[k] for k in range(first[node], first[node + 1])}


# ---------------------------------------------------------------------------------------------- expectation
def expect(logits, bias, ids, fin, nodes, block, st, max_new, ngram, fbos, feos):
    """(tokens, logp, finished after, nodes after, per-row bound, allowed tokens per row) of one step: transformers' processors on
    the f32 scores"""
    from transformers.generation.logits_process import (ForcedBOSTokenLogitsProcessor, ForcedEOSTokenLogitsProcessor,
                                                        NoRepeatNGramLogitsProcessor, PrefixConstrainedLogitsProcessor)
    B, V = logits.shape
    x = logits.float() + (bias.float() if bias is not None else 0.0)
    assert x.dtype == torch.float32
    prefix = ids[:, :st + 1].long()
    if ngram > 0:
        x = NoRepeatNGramLogitsProcessor(ngram)(prefix, x)
    allowed = [sorted(t for t in edges_of(block, int(nodes[b])) if 0 <= t < V) for b in range(B)]
    x = PrefixConstrainedLogitsProcessor(lambda b, sent: allowed[b] or [PAD], 1)(prefix, x)
    for b in range(B):
        if not allowed[b]:
            x[b] = float("-inf")               # fn may not return an empty list: such a row has no allowed token at all
    if fbos >= 0:
        x = ForcedBOSTokenLogitsProcessor(fbos)(prefix, x)
    if feos >= 0:
        x = ForcedEOSTokenLogitsProcessor(max_new + 1, feos, device="cpu")(prefix, x)
    assert x.dtype == torch.float32
    forced = (fbos >= 0 and st == 0) or (feos >= 0 and st + 1 == max_new)
    lsm = torch.log_softmax(x.double(), dim=-1)
    toks, lps, bounds, fin2, nodes2 = [], [], [], fin.clone(), nodes.clone()
    for b in range(B):
        finite = x[b][torch.isfinite(x[b])]
        tok = int(torch.argmax(x[b])) if finite.numel() else 0
        if forced:
            tok = fbos if st == 0 and fbos >= 0 else feos
        bounds.append(2.0 ** -23 * (V / 256 + 16) + 4 * SC.ulp_f32(float(finite.abs().max())) if finite.numel() else float("inf"))
        lp = 0.0 if forced else (float(lsm[b, tok]) if finite.numel() else None)        # None: unspecified
        if fin[b]:
            tok, lp = PAD, 0.0
        else:
            nodes2[b] = edges_of(block, int(nodes[b])).get(tok, -1)
            if tok == EOS:
                fin2[b] = 1
        toks.append(tok); lps.append(lp)
    return toks, lps, fin2, nodes2, bounds, allowed


# ---------------------------------------------------------------------------------------------- one launch inside guard bands
def vocab_op(L, dtype, ptrs, B, V, T, max_new, ngram, fbos, feos, trie_bytes):
    return L.make_op(L.OP_GREEDY_VOCAB_STEP, dtype,
                     p=[ptrs["logits"], ptrs.get("bias"), ptrs["ids"], ptrs["fin"], ptrs.get("logp"), ptrs["node"], ptrs["step"], ptrs["trie"]],
                     i={0: B, 1: V, 2: V, 3: T, 4: max_new, 5: ngram, 6: BOS, 7: EOS, 8: PAD, 9: fbos, 10: feos, 11: 1, 12: trie_bytes})


def launch(L, dev, sync, dtype, logits, bias, ids, fin, nodes, block, st, max_new, ngram, fbos, feos, scores, slack=0, what="vocab"):
    """one launch with every operand in one caption_f64.Arena (0xFF guard bands; logp may only be written in column st + 1, which
    must be written); the trie block is followed by POISON_WORDS 0xFF words, of which `slack` count into i12.
    Returns host (ids, fin, step, logp or None, nodes)."""
    B, V = logits.shape
    T = ids.shape[1]
    ar = CF.Arena()
    ar.add("logits", logits.dtype, B, V, data=((0, logits),))
    ar.add("bias", torch.float32, 1, V, data=((0, bias.view(1, V)),))
    ar.add("ids", torch.int32, B, T, data=((0, ids),))
    ar.add("fin", torch.int32, 1, B, data=((0, fin.view(1, B)),))
    ar.add("node", torch.int32, 1, B, data=((0, nodes.view(1, B)),))
    ar.add("step", torch.int32, 1, 1, data=((0, torch.tensor([[st]], dtype=torch.int32)),))
    if scores:
        ar.add("logp", torch.float32, B, T, out=((st + 1, 1),))
    ar.add("trie", torch.int32, 1, block.numel() + POISON_WORDS, data=((0, block.view(1, -1)),))
    ar.build(dev)
    ptrs = {n: ar.ptr(n) for n in ar.parts}
    L.launch(vocab_op(L, dtype, ptrs, B, V, T, max_new, ngram, fbos, feos, (block.numel() + slack) * 4))
    sync()
    ar.fetch(what)
    assert torch.equal(ar.get("trie", 0, block.numel()).view(-1), block), f"{what}: the trie block was written"
    return (ar.get("ids", 0, T), ar.get("fin", 0, B).view(-1), int(ar.get("step", 0, 1)),
            ar.get("logp", st + 1, 1).view(-1) if scores else None, ar.get("node", 0, B).view(-1))


def run_case(L, dev, sync, f16, scores, inputs, nodes, block, st=GSTEP, ngram=3, fbos=BOS, feos=EOS, max_new=GMAX_NEW, slack=0, what="case"):
    """launch + compare with `expect`: token equal, logp inside the bound (exactly 0.0 where hf's is), finished / step / node
    bookkeeping, nothing but column st + 1 of ids changed; the raw top-1 of every row is outside its allowed set.
    Returns (tokens, nodes after, worst logp error as a fraction of its bound)."""
    dtype, tdt = (L.F16, torch.float16) if f16 else (L.F32, torch.float32)
    ids, logits, bias, fin = inputs
    nodes = torch.tensor(nodes, dtype=torch.int32)
    toks, lps, fin_r, nodes_r, bounds, allowed = expect(logits, bias, ids, fin, nodes, block, st, max_new, ngram, fbos, feos)
    raw = (logits.float() + bias).argmax(1).tolist()
    assert all(raw[b] not in allowed[b] for b in range(ids.shape[0])), f"{what}: a raw top-1 is allowed, the case proves nothing"
    got_ids, got_fin, got_step, got_lp, got_nodes = launch(L, dev, sync, dtype, logits, bias, ids, fin, nodes, block, st, max_new, ngram,
                                                          fbos, feos, scores, slack, what)
    assert got_ids[:, st + 1].tolist() == toks, (what, st, got_ids[:, st + 1].tolist(), toks)
    keep = torch.ones(ids.shape[1], dtype=torch.bool); keep[st + 1] = False
    assert torch.equal(got_ids[:, keep], ids[:, keep]), f"{what}: ids outside the written column changed"
    assert torch.equal(got_fin, fin_r) and got_step == st + 1, what
    assert got_nodes.tolist() == nodes_r.tolist(), (what, got_nodes.tolist(), nodes_r.tolist())
    worst = 0.0
    if scores:
        for b in range(ids.shape[0]):
            got = float(got_lp[b])
            if lps[b] is None:
                continue
            if lps[b] == 0.0:
                assert got == 0.0, (what, st, b, got)
            else:
                err = abs(got - lps[b])
                print(f"{what} step {st} row {b}: logp {got:.6f} vs {lps[b]:.6f}: {err:.3e} (bound {bounds[b]:.3e})")
                assert err <= bounds[b], f"{what} step {st} row {b}: {got} vs {lps[b]}: {err:.3e} > {bounds[b]:.3e}"
                worst = max(worst, err / bounds[b])
    return toks, nodes_r.tolist(), worst


# ---------------------------------------------------------------------------------------------- the test trie and its inputs
class Case:
    """long_greedy_inputs (B = 4, T = 130, 122 tokens of history, row 2 finished; rows 0 and 3 end in a 2-gram whose 40 followers
    the 3-gram rule bans) + one trie whose labels all start with BOS:
      BOS 10 c EOS   for 300 tokens c: the wide node (the strided loop over the edges wraps)
      BOS 11 500 EOS                  a node with one child, and a leaf behind the EOS
      BOS 12 {300, 400} EOS           two children that are given equal values
      BOS 13 {f0, f3, free} EOS       f0 / f3: a banned follower of row 0 / of row 3
      BOS 14 {two followers of row 0} EOS,  BOS 16 {two followers of row 3} EOS     every child banned in that row
      BOS 15 {600, V + 5} EOS         an edge token beyond the vocabulary
    Token LOUD (allowed nowhere) holds the raw maximum of every row."""

    def __init__(self, V, f16):
        self.V, self.f16 = V, f16
        ids, logits, bias, fin, xs, top, tdt = GC.base_inputs(V, f16)
        self.ids, self.bias, self.fin, self.xs, self.top, self.tdt = ids, bias, fin, xs, top, tdt
        special = {0, 1, 2, V - 1, 64, 65, LOUD, 300, 400, 500, 600} | set(range(10, 17))
        used = set(xs[0]) | set(xs[3]) | special
        self.wide = [t for t in range(200, V) if t not in used][:300]
        assert len(self.wide) == 300
        pick = lambda row: [t for t in xs[row] if t not in special and t not in xs[3 - row]]
        self.f0, self.f3 = pick(0)[-1], pick(3)[-1]
        self.all0, self.all3 = pick(0)[:2], pick(3)[:2]
        self.free = next(t for t in range(700, V) if t not in used and t not in self.wide)
        labels = [[BOS, 10, c, EOS] for c in self.wide] + [[BOS, 11, 500, EOS], [BOS, 12, 300, EOS], [BOS, 12, 400, EOS]]
        labels += [[BOS, 13, t, EOS] for t in (self.f0, self.f3, self.free)]
        labels += [[BOS, 14, t, EOS] for t in self.all0] + [[BOS, 16, t, EOS] for t in self.all3]
        labels += [[BOS, 15, 600, EOS], [BOS, 15, V + 5, EOS]]
        self.vocab = vocabulary(labels)
        self.block = self.vocab.pack()
        self.node = lambda *path: self.vocab.walk([BOS, *path])
        bias[300] = bias[400] = 0.25
        for row in range(GB):
            GC._set(logits, bias, row, LOUD, top + 5.0)
        self.logits = logits

    def set(self, row, tok, value):
        GC._set(self.logits, self.bias, row, tok, value)

    def inputs(self):
        return self.ids, self.logits.to(self.tdt).contiguous(), self.bias, self.fin


def check_wide_node(L, dev, V, f16, scores, sync=lambda: None):
    """300 children: the maximum is the last child in row 0, the first in row 1, child 270 (a second trip of the strided loop) in row 3"""
    c = Case(V, f16)
    c.set(0, c.wide[-1], c.top + 1.0); c.set(1, c.wide[0], c.top + 1.0); c.set(3, c.wide[270], c.top + 1.0)
    w = c.node(10)
    toks, nodes, worst = run_case(L, dev, sync, f16, scores, c.inputs(), [w, w, w, w], c.block, what="wide node")
    assert toks == [c.wide[-1], c.wide[0], PAD, c.wide[270]] and nodes[2] == w and min(nodes[0], nodes[1], nodes[3]) > 0
    return worst


def check_single_child_and_ties(L, dev, V, f16, scores, sync=lambda: None):
    """row 0 at a node with one child: that child, logp exactly 0.0; rows 1 and 3 at the node with children 300 and 400: equal
    values in row 1 (the lower id wins), 400 larger in row 3"""
    c = Case(V, f16)
    c.set(1, 300, 2.5); c.set(1, 400, 2.5); c.set(3, 300, 1.0); c.set(3, 400, 2.0)
    inputs = c.inputs()
    x = inputs[1].float() + c.bias
    assert float(x[1, 300]) == float(x[1, 400])
    s, e = c.node(11), c.node(12)
    toks, nodes, worst = run_case(L, dev, sync, f16, scores, inputs, [s, e, s, e], c.block, what="single child / tie")
    assert toks == [500, 300, PAD, 400] and nodes == [c.node(11, 500), c.node(12, 300), s, c.node(12, 400)]
    return worst


def check_ngram_ban(L, dev, V, f16, scores, sync=lambda: None):
    """a child removed by the ban: at BOS 13 row 0 loses f0 (its largest child) and row 3 loses f3, row 1 (no ban) keeps f0; then
    every child removed: row 0 at BOS 14 and row 3 at BOS 16 emit id 0 and leave the trie, row 1 at BOS 14 picks a child"""
    c = Case(V, f16)
    for row in (0, 1, 3):
        c.set(row, c.f0, c.top + 2.0); c.set(row, c.f3, c.top + 1.5); c.set(row, c.free, c.top - 3.0)
    c.set(0, c.f3, c.top - 4.0)                                      # row 0: behind `free` once f0 is gone
    n13, n14, n16 = c.node(13), c.node(14), c.node(16)
    toks, nodes, w0 = run_case(L, dev, sync, f16, scores, c.inputs(), [n13, n13, n13, n13], c.block, what="ngram: one child banned")
    assert toks == [c.free, c.f0, PAD, c.f0], (toks, c.f0, c.f3, c.free)
    toks, nodes, w1 = run_case(L, dev, sync, f16, scores, c.inputs(), [n14, n14, n14, n16], c.block, what="ngram: every child banned")
    assert toks[0] == 0 and toks[3] == 0 and toks[1] in c.all0 and nodes[0] == -1 and nodes[3] == -1 and nodes[1] > 0
    return max(w0, w1)


def check_leaf_and_outside(L, dev, V, f16, scores, sync=lambda: None):
    """a leaf, node -1, a node number beyond the trie: id 0, node -1; the finished row (at -1) emits pad and keeps its node"""
    c = Case(V, f16)
    leaf = c.node(11, 500, EOS)
    assert leaf > 0 and not c.vocab.children(leaf)
    toks, nodes, _ = run_case(L, dev, sync, f16, scores, c.inputs(), [leaf, -1, -1, c.vocab.n_nodes + 7], c.block, what="leaf / outside")
    assert toks == [0, 0, PAD, 0] and nodes == [-1, -1, -1, -1]
    toks, nodes, _ = run_case(L, dev, sync, f16, scores, c.inputs(), [leaf, -1, leaf, 1 << 30], c.block, what="finished at a leaf")
    assert toks == [0, 0, PAD, 0] and nodes == [-1, -1, leaf, -1]


def check_forced_positions(L, dev, V, f16, scores, sync=lambda: None):
    """step 0: the forced BOS moves a row from the root to the node behind BOS, and a row at a node without a BOS edge out of the
    trie; step max_new - 1: the forced EOS finishes every row, the node follows the EOS edge where there is one; logp exactly 0.0"""
    c = Case(V, f16)
    one = c.node(11)
    toks, nodes, _ = run_case(L, dev, sync, f16, scores, c.inputs(), [0, 0, 0, one], c.block, st=0, what="forced BOS")
    assert toks == [BOS, BOS, PAD, BOS] and nodes == [c.node(), c.node(), 0, -1]
    last = c.node(11, 500)
    toks, nodes, _ = run_case(L, dev, sync, f16, scores, c.inputs(), [last, c.node(10), last, c.node(12)], c.block, st=GMAX_NEW - 1,
                              what="forced EOS")
    assert toks == [EOS, EOS, PAD, EOS] and nodes == [c.node(11, 500, EOS), -1, last, -1]


def check_edge_token_beyond_vocabulary(L, dev, V, f16, scores, sync=lambda: None):
    """children {600, V + 5}: V + 5 is no entry of the row (in rows 0..2 it is entry 5 of the NEXT row, which holds that row's
    maximum) and is skipped: 600, logp exactly 0.0.  The trie block is followed by poison words that count into i12, as the words
    behind a block in a plan's buffer do."""
    c = Case(V, f16)
    n = c.node(15)
    assert sorted(edges_of(c.block, n)) == [600, V + 5]
    toks, nodes, worst = run_case(L, dev, sync, f16, scores, c.inputs(), [n, n, n, n], c.block, slack=POISON_WORDS, what="edge token >= V")
    assert toks == [600, 600, PAD, 600]
    return worst


def check_short_block(L, dev, V, sync=lambda: None):
    """a block whose header claims more than i12 holds, an i12 below the header, and a header with impossible counts: OMNI_E_ARG
    from omni_op_launch (a host-side argument check; nothing is launched, nothing written); the full size is accepted"""
    c = Case(V, False)
    ids, logits, bias, fin = c.inputs()
    d = {"logits": logits.to(dev), "bias": bias.to(dev), "ids": ids.to(dev), "fin": fin.to(dev), "node": torch.zeros(GB, dtype=torch.int32).to(dev),
         "step": torch.tensor([GSTEP], dtype=torch.int32).to(dev), "trie": c.block.to(dev)}
    lying = c.block.clone()
    lying[0] = 0
    d["lying"] = lying.to(dev)
    sync()
    ptrs = {k: v.data_ptr() for k, v in d.items()}
    seen = []
    full = c.block.numel() * 4
    for nbytes, trie in ((full - 4, "trie"), (full // 2, "trie"), (36, "trie"), (16, "trie"), (0, "trie"), (full, "lying")):
        op = vocab_op(L, L.F32, {**ptrs, "trie": ptrs[trie]}, GB, V, GT, GMAX_NEW, 3, BOS, EOS, nbytes)
        rc = L.lib().omni_op_launch(ctypes.byref(op), L._stream_ptr(None))
        assert rc == -1, (nbytes, trie, rc)                           # OMNI_E_ARG
        seen.append(L.lib().omni_last_error().decode())
    sync()
    assert torch.equal(d["ids"].cpu(), ids) and int(d["step"].cpu()) == GSTEP
    L.launch(vocab_op(L, L.F32, ptrs, GB, V, GT, GMAX_NEW, 3, BOS, EOS, full))
    sync()
    assert int(d["step"].cpu()) == GSTEP + 1
    return seen


# ---------------------------------------------------------------------------------------------- whole captioner vs transformers
N_CROPS, R, N_LABELS, VOCAB_SEED = GC.N_CROPS, GC.R, 64, 11
# The pixel seed: the first one from 403 upward at which the oracle's own smallest finite top-1 / top-2 gap of the CONSTRAINED scores
# is at least beam_checks.MARGIN (2e-4) on both checkpoints — below it the reference alone could not hold a cap of 0 excused rows.
# transformers 5.15 on the CPU, the vocabulary of `labels_for`: 403 itself holds it — the smallest finite gap is 9.76e-2 on the stock
# and on the EOS-prone checkpoint (the same first decision of the same row), and all 4 rows differ from the default output on both.
SEED = 403
MEASURED_GAP = {"stock": 9.756e-2, "eos_prone": 9.756e-2}
_ORACLE = {}


def labels_for(eos, seed=VOCAB_SEED):
    """64 seeded labels [BOS, 1..6 body tokens, eos] over a pool of 12 tokens: shared prefixes, >= 8 distinct first tokens, and a
    label whose body is a prefix of another's; body tokens may repeat (the 3-gram ban is live), dead ends are redrawn"""
    from omniparser_amd.florence import CaptionVocabulary
    g = torch.Generator().manual_seed(seed)
    pool = [t for t in (torch.randperm(40000, generator=g)[:14] + 100).tolist() if t not in (2, 13840)][:12]
    bodies = []
    while len(bodies) < N_LABELS:
        n = int(torch.randint(1, 7, (1,), generator=g))
        body = [pool[int(i)] for i in torch.randint(0, len(pool), (n,), generator=g)]
        if len(bodies) == 1:
            body = bodies[0][:1] if len(bodies[0]) > 1 else bodies[0] + [pool[0]]       # a body that is a prefix of another / extends it
        if body in bodies:
            continue
        try:
            CaptionVocabulary([[BOS] + b + [eos] for b in bodies + [body]]).check(51289, 10, eos, BOS, 2, 3, START)
        except ValueError:
            continue
        bodies.append(body)
    labels = [[BOS] + b + [eos] for b in bodies]
    assert len({b[0] for b in bodies}) >= 8
    assert any(a != b and b[:len(a)] == a for a in bodies for b in bodies)
    return labels


def max_new_for(labels):
    return max(len(lab) for lab in labels) + 2


def pixels(seed=None):
    return GC.pixels(SEED if seed is None else seed)


def hf_fn(vocab, pad):
    """transformers' prefix_allowed_tokens_fn of a vocabulary: the children of the node reached along sent[1:], [pad] for a prefix
    that has left the trie or has finished its label (transformers requires a non-empty list)"""
    def fn(batch_id, sent):
        return vocab.children(vocab.walk(sent[1:].tolist())) or [pad]
    return fn


def _hf(model, pix, max_new, **kw):
    from omniparser_amd.florence import PROMPT_IDS
    cfg = model.config
    n_img = (pix.shape[-1] // 32) ** 2 + 1
    inp = torch.tensor([[cfg.image_token_id] * n_img + PROMPT_IDS] * pix.shape[0])
    with torch.inference_mode():
        out = model.generate(input_ids=inp, pixel_values=pix, max_new_tokens=max_new, num_beams=1, do_sample=False,
                             output_scores=True, return_dict_in_generate=True, **kw)
        ts = model.compute_transition_scores(out.sequences, out.scores, normalize_logits=True)
    gaps = []
    for s in out.scores:
        top = s.double().topk(2, dim=-1).values
        g = top[:, 0] - top[:, 1]
        g[~torch.isfinite(g)] = float("inf")                  # a forced position or a single child is no decision
        gaps.append(g)
    return out.sequences, ts.double(), torch.stack(gaps, 1)


def oracle(eos_prone, constrained=True, seed=None):
    """transformers on the CPU, once per (checkpoint, constrained, seed): (sequences, transition scores, gaps)"""
    import beam_checks as BC
    seed = SEED if seed is None else seed
    key = (eos_prone, constrained, seed)
    if key not in _ORACLE:
        eos = BC.EOS_PRONE_TOKEN if eos_prone else 2
        labels = labels_for(eos)
        model = BC.oracle_model(0, eos_prone)
        try:
            kw = {"prefix_allowed_tokens_fn": hf_fn(vocabulary(labels), PAD)} if constrained else {}
            _ORACLE[key] = _hf(model, pixels(seed), max_new_for(labels), **kw)
        finally:
            model.generation_config.eos_token_id = 2
    return _ORACLE[key]


def smallest_gap(eos_prone, seed=None):
    gaps = oracle(eos_prone, True, seed)[2]
    return float(gaps[torch.isfinite(gaps)].min())


def captioner_vs_hf(eos_prone, device_pixels=False, cap=None, crops=False):
    """generate(vocabulary=..., output_scores=True) against transformers' generate(prefix_allowed_tokens_fn=...): no row excused;
    the largest |delta logp| is printed, then held to long_checks.TOL_LOGP_LONG.  Every row is start + one label + pad and
    label_index names it; the reference differs from its own default output in every row."""
    import beam_checks as BC
    eos = BC.EOS_PRONE_TOKEN if eos_prone else 2
    labels = labels_for(eos)
    max_new = max_new_for(labels)
    ref_seq, ref_ts, gaps = oracle(eos_prone)
    dflt = oracle(eos_prone, False)[0]
    cap = cap or GC.captioner(eos_prone)
    pix = pixels()
    out = cap.generate(pixel_values=pix.cuda() if device_pixels else pix, max_new_tokens=max_new, output_scores=True,
                       return_dict_in_generate=True, vocabulary=labels)
    worst, _ = SC.compare_with_hf(out.sequences, out.token_logprobs, ref_seq, ref_ts, gaps, eos, cap.w.pad, float("inf"), max_excused=0)
    finite = gaps[torch.isfinite(gaps)]
    changed = [b for b in range(N_CROPS) if GC.rows_changed(ref_seq[b:b + 1], dflt[b:b + 1], cap.w.pad)]
    print(f"vocabulary vs transformers: eos_prone={eos_prone} seed {SEED}: max |dlogp| = {worst:.3e}, smallest oracle gap "
          f"{float(finite.min()):.3e}, rows that differ from the default output {changed}, labels {out.label_index.tolist()}")
    assert float(finite.min()) >= BC.MARGIN, "the oracle's own gap is below the margin: choose another pixel seed"
    SC.compare_with_hf(out.sequences, out.token_logprobs, ref_seq, ref_ts, gaps, eos, cap.w.pad, LC.TOL_LOGP_LONG, max_excused=0)
    assert len(changed) == N_CROPS, "the reference's constrained output equals its default output in a row"
    check_rows_are_labels(out.sequences, out.label_index, labels, eos, cap.w.pad, cap.w.start)
    plain = cap.generate(pixel_values=pix.cuda() if device_pixels else pix, max_new_tokens=max_new, vocabulary=vocabulary(labels))
    assert torch.equal(plain, out.sequences), "the ids depend on output_scores"
    return worst


def check_rows_are_labels(seq, label_index, labels, eos, pad, start):
    distinct = list(dict.fromkeys(tuple(lab) for lab in labels))
    assert label_index.dtype == torch.long and tuple(label_index.shape) == (seq.shape[0],)
    for b, row in enumerate(seq.tolist()):
        k = int(label_index[b])
        assert 0 <= k < len(distinct), (b, k)
        lab = list(distinct[k])
        assert row[0] == start and row[1:1 + len(lab)] == lab and all(t == pad for t in row[1 + len(lab):]), (b, row, lab)


def check_caption_crops(cap, device_pixels=True, n_boxes=5):
    """caption_crops(vocabulary=...) on a frame = generate(vocabulary=...) on the pixels the crop op produced, ids and scores"""
    import gpu_checks as G
    from omniparser_amd.synth import synthetic_screenshot
    labels = labels_for(cap.w.eos)
    max_new = max_new_for(labels)
    frame = torch.from_numpy(synthetic_screenshot(5))
    frame = frame.cuda() if device_pixels else frame
    boxes = G.real_crop_boxes(5, n_boxes)
    cp = cap.plans(cap.bucket(len(boxes)), R, max_new)
    G._fill_rows(cap, cp, frame, boxes, list(range(len(boxes))))
    crop_px = cp.x_in.t[:len(boxes), :, :, :3].permute(0, 3, 1, 2).float().clone()
    want = cap.generate(pixel_values=crop_px, max_new_tokens=max_new, output_scores=True, return_dict_in_generate=True, vocabulary=labels)
    got = cap.caption_crops(frame, boxes, max_new_tokens=max_new, vocabulary=labels)
    got2, lp2 = cap.caption_crops(frame, boxes, max_new_tokens=max_new, vocabulary=vocabulary(labels), return_scores=True)
    assert torch.equal(got, want.sequences) and torch.equal(got2, got) and torch.equal(lp2, want.token_logprobs)
    check_rows_are_labels(got, want.label_index, labels, cap.w.eos, cap.w.pad, cap.w.start)


# ---------------------------------------------------------------------------------------------- plans and defaults
def check_plans_and_defaults(cap, device_pixels=False, full=True):
    """a default call, two vocabularies on ONE plan and graph, the default call again: bit-identical before and after, no `vocab`
    plan from a default call.  Starts from an empty plan cache (the captioner may have served other tests)."""
    L = GC.cap_lib()
    pix = pixels()
    px = pix.cuda() if device_pixels else pix
    eos = cap.w.eos
    v1 = labels_for(eos)
    v2 = [lab for lab in labels_for(eos, VOCAB_SEED + 1) if len(lab) <= max(len(x) for x in v1)]
    max_new = max_new_for(v1)
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    cap.clear_plans()
    has_vocab = lambda: [k for k in cap._plans if "vocab" in k]
    first = cap.generate(pixel_values=px, max_new_tokens=max_new)
    assert not has_vocab(), "a default call built a vocabulary plan"
    a = cap.generate(pixel_values=px, max_new_tokens=max_new, vocabulary=v1, return_dict_in_generate=True)
    assert len(has_vocab()) == 1
    plan = cap._plans[has_vocab()[0]]
    assert plan is cap.plans(cap.bucket(N_CROPS), R, max_new, vocab=True)
    kinds = [op.kind for op in plan.step_plan.ops]
    assert kinds[-1] == L.OP_GREEDY_VOCAB_STEP and L.OP_GREEDY_STEP not in kinds and L.OP_GREEDY_CTRL_STEP not in kinds
    dflt_plan = cap.plans(cap.bucket(N_CROPS), R, max_new)
    assert [op.kind for op in dflt_plan.step_plan.ops][-1] == L.OP_GREEDY_STEP and dflt_plan.trie is None and dflt_plan.node is None
    nbytes = cap.plan_cache_bytes()
    b = cap.generate(pixel_values=px, max_new_tokens=max_new, vocabulary=v2, return_dict_in_generate=True)
    assert len(has_vocab()) == 1 and cap._plans[has_vocab()[0]] is plan and cap.plan_cache_bytes() == nbytes
    check_rows_are_labels(a.sequences, a.label_index, v1, eos, cap.w.pad, cap.w.start)
    check_rows_are_labels(b.sequences, b.label_index, v2, eos, cap.w.pad, cap.w.start)
    assert GC.rows_changed(a.sequences, first, cap.w.pad) == N_CROPS, "the vocabulary changed nothing"
    again = cap.generate(pixel_values=px, max_new_tokens=max_new)
    assert torch.equal(again, first), "a vocabulary leaked into the next default call"
    if not full:                                                      # the emulated twin stops here: every call is an emulated encode
        return first, a, b
    a2 = cap.generate(pixel_values=px, max_new_tokens=max_new, vocabulary=v1)
    assert torch.equal(a2, a.sequences), "a vocabulary depends on the one that ran before it"
    return first, a, b


# ---------------------------------------------------------------------------------------------- host side
def check_packed_block():
    """the packed block of a known vocabulary, word for word, against include/omni_amd.h"""
    from omniparser_amd.florence import vocab_trie_words
    v = vocabulary([[0, 7, 2], [0, 5, 9, 2], [0, 5, 2], [0, 7, 2], [0, 5, 9, 2]])
    assert v.labels == ((0, 7, 2), (0, 5, 9, 2), (0, 5, 2)) and v.longest == 4
    # nodes in insertion order: 0 root, 1 [0], 2 [0 7], 3 [0 7 2], 4 [0 5], 5 [0 5 9], 6 [0 5 9 2], 7 [0 5 2]
    w = v.pack()
    assert w.dtype == torch.int32 and w.numel() == vocab_trie_words(8) == 8 + 9 + 14
    assert w[:8].tolist() == [8, 7, 4, 0, 0, 0, 0, 0]
    assert w[8:17].tolist() == [0, 1, 3, 4, 4, 6, 7, 7, 7]                      # first
    assert w[17:24].tolist() == [0, 5, 7, 2, 2, 9, 2]                            # edge_tok, ascending within a node
    assert w[24:31].tolist() == [1, 4, 2, 3, 7, 5, 6]                            # edge_dst
    assert [v.label_of(n) for n in range(8)] == [-1, -1, -1, 0, -1, -1, 1, 2] and v.label_of(99) == -1
    assert v.walk([0, 5, 9]) == 5 and v.walk([0, 6]) == -1 and v.children(4) == [2, 9] and v.children(3) == []
    assert v.label_index([0, 5, 2, 1, 1], 2) == 2 and v.label_index([0, 5, 9, 1], 2) == -1 and v.label_index([0, 9, 2], 2) == -1
    assert vocab_trie_words() == 8 + 65537 + 2 * 65535

"""Checks shared by the CPU (emulation) and GPU tests of OMNI_OP_VISUAL_MATCH and of the calls around it (Florence2Captioner.embed /
embed_crops / match / caption_crops(return_embeddings=True), util.utils.embed_elements / match_elements / track_elements,
ScreenParser.embed / match / track, Omniparser.find_similar).

Kernel bounds, all a priori:
  mode 0   |y - y_f64| <= 4 x 2^-23 per component and |norm - norm_f64| <= 4 x 2^-23, against the f64 result of the same stored inputs.
           An ABSOLUTE bound on the norm means something only while the norm's own f32 spacing is below it, i.e. for norms below 2, so the
           rows of that case are drawn with sigma = D^-1/2 (norm ~ 1).  A second case holds rows at sigma = 1 — the scale
           image_proj_norm leaves, norm ~ 28 — where the components keep the absolute bound (they are below 1) and the norm is held to
           the same four units RELATIVE to itself (4 x 2^-23 x norm): the sum of squares has 1 + D / 256 + 6 roundings per lane path,
           the square root halves their relative sum and adds half a unit.
  mode 1+2 |s - s_f64| <= D x 2^-24 x sum |q_i g_i|, which holds for any summation order of f32 products and sums; indices equal the
           f64 ranking (ties: the lower gallery index), no position excused: MATCH_SEED is chosen so that the f64 reference itself
           has no two neighbouring scores closer than twice that bound among the ranks that are compared (`reference_gaps`)."""
import ctypes

import torch

import caption_f64 as CF

ULP1 = 2.0 ** -23
TOL_EMBED = 4 * ULP1
D_MODEL = 768
MATCH_SEED = 0            # see `find_seed`; `reference_gaps` re-asserts it in every test that relies on it
E_ARG = -1


# ---------------------------------------------------------------------------------------------- mode 0
def embed_inputs(n=3, n_img=5, D=D_MODEL, sigma=None, f16=False, seed=0):
    """[n, n_img x D] in the source dtype: seeded Gaussian rows, the LAST crop's row 0 all zero (its other rows are not)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, n_img * D, generator=g) * (D ** -0.5 if sigma is None else sigma)
    x[n - 1, :D] = 0.0
    return x.to(torch.float16 if f16 else torch.float32)


def launch_embed(L, dev, sync, x, n_img, D, what="embed"):
    from omniparser_amd.florence import embed_op
    n = x.shape[0]
    ar = CF.Arena()
    ar.add("x", x.dtype, n, n_img * D, data=((0, x),))
    ar.add("y", torch.float32, n, D, out=((0, D),))
    ar.add("norm", torch.float32, 1, n, out=((0, n),))
    ar.build(dev)
    y = torch.empty(0)
    op = embed_op(L.F16 if x.dtype == torch.float16 else L.F32, ar.ptr("x"), n_img * D, y, y, n, D)
    op.p[4], op.p[5] = ar.ptr("y"), ar.ptr("norm")
    L.launch(op)
    sync()
    ar.fetch(what)
    return ar.get("y", 0, D), ar.get("norm", 0, n).view(-1)


def check_embed(L, dev, f16, sigma=None, sync=lambda: None, n=3, n_img=5, D=D_MODEL):
    x = embed_inputs(n, n_img, D, sigma, f16)
    y, norm = launch_embed(L, dev, sync, x, n_img, D)
    x0 = x[:, :D].double()
    ref_n = x0.pow(2).sum(1).sqrt()
    ref_y = torch.where(ref_n[:, None] > 0, x0 / ref_n[:, None].clamp_min(1e-300), torch.zeros_like(x0))
    ey = float((y.double() - ref_y).abs().max())
    en = (norm.double() - ref_n).abs()
    tol_n = TOL_EMBED * (ref_n.clamp_min(1.0) if sigma is not None else torch.ones_like(ref_n))
    print(f"embed f16={f16} sigma={sigma}: max |dy| = {ey / ULP1:.2f} ulp-of-1, norms {ref_n.tolist()}, |dnorm| = {(en / ULP1).tolist()} ulp-of-1")
    assert torch.isfinite(y).all() and torch.isfinite(norm).all()
    assert ey <= TOL_EMBED, ey
    assert bool((en <= tol_n).all()), (en.tolist(), tol_n.tolist())
    assert float(ref_n[n - 1]) == 0.0 and float(norm[n - 1]) == 0.0 and not bool(y[n - 1].any()), "the zero row is not exactly zero"
    if sigma is None:
        assert float(ref_n[:n - 1].max()) < 2.0, "the absolute norm bound needs norms below 2"
    return ey, float(en.max())


# ---------------------------------------------------------------------------------------------- modes 1 + 2
def unit_rows(rows, D, g):
    x = torch.randn(rows, D, generator=g, dtype=torch.float64)
    return (x / x.norm(dim=1, keepdim=True)).float()


def match_inputs(m=3, n=70, D=D_MODEL, seed=MATCH_SEED, ties=False):
    """unit queries and gallery; half of the gallery are look-alikes of a query (the query plus noise of its own size, renormalised),
    so the top ranks hold close scores of both kinds.  ties: gallery rows 5, 40 and 69 ARE query 0."""
    g = torch.Generator().manual_seed(seed)
    Q = unit_rows(m, D, g)
    G = unit_rows(n, D, g)
    for j in range(0, n, 2):
        mix = Q[j % m].double() + unit_rows(1, D, g)[0].double() * (0.5 + 0.1 * (j % 7))
        G[j] = (mix / mix.norm()).float()
    if ties:
        for j in (5, 40, 69):
            G[j] = Q[0]
    return Q, G


def reference(Q, G, k):
    """(f64 scores [m, n], bound [m, n], ranking idx [m, min(k, n)] — descending f64 score, the lower index first among equals)"""
    D = Q.shape[1]
    s = Q.double() @ G.double().T
    # identical gallery rows are exact ties; a BLAS may sum column j and column j' in different orders, so one of them speaks for all
    first = {}
    for j in range(G.shape[0]):
        j0 = first.setdefault(G[j].numpy().tobytes(), j)
        s[:, j] = s[:, j0]
    bound = D * 2.0 ** -24 * (Q.double().abs() @ G.double().abs().T)
    order = torch.sort(s, dim=1, descending=True, stable=True).indices
    return s, bound, order[:, :min(k, G.shape[0])]


def reference_gaps(Q, G, k):
    """positions the f64 reference ITSELF cannot rank: neighbours among ranks 0..min(k, n) whose f64 scores differ by less than twice
    the bound, identical gallery rows (an exact tie, ranked by index) aside.  [(query, rank)]"""
    s, bound, _ = reference(Q, G, k)
    n = G.shape[0]
    order = torch.sort(s, dim=1, descending=True, stable=True).indices
    bad = []
    for q in range(Q.shape[0]):
        for r in range(min(k, n - 1)):
            a, b = int(order[q, r]), int(order[q, r + 1])
            if torch.equal(G[a], G[b]):
                continue
            if float(s[q, a] - s[q, b]) < 2 * float(max(bound[q, a], bound[q, b])):
                bad.append((q, r))
    return bad


def find_seed(first=0, tries=64, k=8):
    """the first seed from `first` up at which neither the main case nor the tie case has a position the f64 reference cannot rank
    (run on the CPU when MATCH_SEED is chosen; seed 0 holds it)"""
    for seed in range(first, first + tries):
        if not any(reference_gaps(*match_inputs(m, n, D, seed=seed, ties=ties), kk) for m, n, D, kk, ties in SEEDED_CASES):
            return seed
    raise AssertionError("no seed")


# every (m, n, D, k, ties) the checks below draw with MATCH_SEED
SEEDED_CASES = ((3, 70, D_MODEL, 8, False), (3, 70, D_MODEL, 8, True), (3, 5, D_MODEL, 8, False), (9, 70, D_MODEL, 8, False),
                (3, 70, 100, 8, False), (2, 9, 2048, 8, False), (3, 600, 64, 4, False))


def launch_match(L, dev, sync, Q, G, k, split_len=0, what="match"):
    """modes 1 and 2, one launch each, every operand in one guard-banded arena.  Returns (idx i32 [m, k], score f32 [m, k], splits)."""
    from omniparser_amd.florence import match_geometry, match_ops
    (m, D), n = Q.shape, G.shape[0]
    groups, length, splits, nbytes = match_geometry(m, n, D, k, split_len)
    assert groups == (m + 7) // 8 and splits == (n + length - 1) // length and nbytes == m * splits * k * 8
    ar = CF.Arena()
    ar.add("q", torch.float32, m, D, data=((0, Q),))
    ar.add("g", torch.float32, n, D, data=((0, G),))
    ar.add("part", torch.int32, 1, nbytes // 4, scratch=True)
    full = n >= k                                      # else idx legitimately holds -1, the arena's "unwritten" pattern
    ar.add("idx", torch.int32, m, k, **({"out": ((0, k),)} if full else {"scratch": True}))
    ar.add("score", torch.float32, m, k, out=((0, k),))
    ar.build(dev)
    one, two = match_ops(ar.ptr("q"), ar.ptr("g"), ar.ptr("part"), ar.ptr("idx"), ar.ptr("score"), m, n, D, k, split_len, nbytes)
    L.launch(one)
    L.launch(two)
    sync()
    ar.fetch(what)
    return ar.get("idx", 0, k), ar.get("score", 0, k), splits


def check_against_reference(Q, G, k, idx, score, what):
    s, bound, want = reference(Q, G, k)
    kk = want.shape[1]
    assert idx[:, :kk].tolist() == want.tolist(), (what, idx[:, :kk].tolist(), want.tolist())
    err = (score[:, :kk].double() - s.gather(1, want)).abs()
    frac = float((err / bound.gather(1, want)).max())
    print(f"{what}: worst score error {frac:.3f} of the bound")
    assert frac <= 1.0, (what, frac)
    assert bool((idx[:, kk:] == -1).all()) and bool((score[:, kk:] == float("-inf")).all()), f"{what}: positions behind min(k, n)"
    return frac


def check_match(L, dev, k, sync=lambda: None, ties=False, m=3, n=70, D=D_MODEL, forced=32, forced_splits=3):
    """the default split and a forced split length: each against the f64 reference (no position excused), and torch.equal to each
    other in idx and score"""
    Q, G = match_inputs(m, n, D, ties=ties)
    assert reference_gaps(Q, G, k) == [], "the f64 reference cannot rank a compared position: choose another MATCH_SEED (find_seed)"
    i0, s0, n0 = launch_match(L, dev, sync, Q, G, k, 0, "default split")
    i1, s1, n1 = launch_match(L, dev, sync, Q, G, k, forced, f"split length {forced}")
    assert n0 == 1 and n1 == forced_splits, (n0, n1)
    worst = max(check_against_reference(Q, G, k, i0, s0, f"m={m} n={n} D={D} k={k} default split"),
                check_against_reference(Q, G, k, i1, s1, f"m={m} n={n} D={D} k={k} split length {forced}"))
    assert torch.equal(i0, i1) and torch.equal(s0.view(torch.int32), s1.view(torch.int32)), "the split changed idx or the bits of a score"
    if ties:
        assert i0[0, :min(k, 3)].tolist() == [5, 40, 69][:min(k, 3)] and i1[0, :min(k, 3)].tolist() == [5, 40, 69][:min(k, 3)]
    return worst


def check_short_gallery(L, dev, sync=lambda: None):
    """n = 5, k = 8: five ranked positions, then three times -1 / -inf"""
    Q, G = match_inputs(3, 5, D_MODEL)
    assert reference_gaps(Q, G, 8) == []
    idx, score, _ = launch_match(L, dev, sync, Q, G, 8, 0, "n = 5")
    check_against_reference(Q, G, 8, idx, score, "n = 5, k = 8")
    assert idx[:, 5:].tolist() == [[-1] * 3] * 3 and bool((score[:, 5:] == float("-inf")).all())
    i2, s2, n2 = launch_match(L, dev, sync, Q, G, 8, 2, "n = 5, split length 2")
    assert n2 == 3 and torch.equal(idx, i2) and torch.equal(s2.view(torch.int32), score.view(torch.int32))


def check_two_groups(L, dev, sync=lambda: None):
    """m = 9: two query groups, the second one holds one query; a query has the same bits whatever its place in a group"""
    Q, G = match_inputs(9, 70, D_MODEL)
    assert reference_gaps(Q, G, 8) == []
    idx, score, _ = launch_match(L, dev, sync, Q, G, 8, 0, "m = 9")
    check_against_reference(Q, G, 8, idx, score, "m = 9")
    i2, s2, _ = launch_match(L, dev, sync, Q, G, 8, 32, "m = 9, split length 32")
    assert torch.equal(idx, i2) and torch.equal(s2.view(torch.int32), score.view(torch.int32))
    alone_i, alone_s, _ = launch_match(L, dev, sync, Q[8:9], G, 8, 0, "the ninth query alone")
    moved_i, moved_s, _ = launch_match(L, dev, sync, Q[[3, 8, 0]], G, 8, 0, "queries 3, 8, 0")
    assert torch.equal(alone_i[0], idx[8]) and torch.equal(alone_s[0].view(torch.int32), score[8].view(torch.int32))
    assert torch.equal(moved_i, idx[[3, 8, 0]]) and torch.equal(moved_s.view(torch.int32), score[[3, 8, 0]].view(torch.int32))


def check_odd_width(L, dev, sync=lambda: None):
    """D = 100: no multiple of the wave's 256-float stride (25 of 64 lanes load); D = 2048: the query group is read through the
    caches instead of LDS; n = 600 at D = 64: the launcher's own choice is two slices"""
    from omniparser_amd.florence import match_geometry
    for m, n, D, forced, splits in ((3, 70, 100, 32, 3), (2, 9, 2048, 4, 3)):
        Q, G = match_inputs(m, n, D)
        assert reference_gaps(Q, G, 8) == [], (D, reference_gaps(Q, G, 8))
        idx, score, _ = launch_match(L, dev, sync, Q, G, 8, 0, f"D = {D}")
        check_against_reference(Q, G, 8, idx, score, f"D = {D}")
        i2, s2, n2 = launch_match(L, dev, sync, Q, G, 8, forced, f"D = {D}, split length {forced}")
        assert n2 == splits and torch.equal(idx, i2) and torch.equal(s2.view(torch.int32), score.view(torch.int32))
    assert match_geometry(3, 600, 64, 8)[1:3] == (300, 2)
    Q, G = match_inputs(3, 600, 64)
    assert reference_gaps(Q, G, 4) == []
    idx, score, splits = launch_match(L, dev, sync, Q, G, 4, 0, "n = 600")
    check_against_reference(Q, G, 4, idx, score, "n = 600, two slices by default")
    i2, s2, _ = launch_match(L, dev, sync, Q, G, 4, 600, "n = 600, one slice")
    assert splits == 2 and torch.equal(idx, i2) and torch.equal(s2.view(torch.int32), score.view(torch.int32))


def check_argument_errors(L, dev, sync=lambda: None):
    """k = 9, D = 6, n = 0, a null gallery, a partials buffer one element short: OMNI_E_ARG from omni_op_launch, idx / score / partials
    untouched; the same operands with good arguments are accepted"""
    from omniparser_amd.florence import match_geometry, match_ops
    m, n, D, k = 3, 70, D_MODEL, 8
    Q, G = match_inputs(m, n, D)
    nbytes = match_geometry(m, n, D, k)[3]
    d = {"q": Q.to(dev), "g": G.to(dev), "part": torch.full((nbytes // 4,), 0x5A5A5A5A, dtype=torch.int32).to(dev),
         "idx": torch.full((m * k + 8,), -7, dtype=torch.int32).to(dev), "score": torch.full((m * k + 8,), -7.0).to(dev)}
    sync()
    p = {name: t.data_ptr() for name, t in d.items()}
    seen = []
    for what, kw in (("k = 9", dict(k=9)), ("D = 6", dict(D=6)), ("n = 0", dict(n=0)), ("null gallery", dict(g=None)),
                     ("partials one element short", dict(nbytes=nbytes - 8))):
        a = dict(m=m, n=n, D=D, k=k, g=p["g"], nbytes=nbytes)
        a.update(kw)
        for op in match_ops(p["q"], a["g"], p["part"], p["idx"], p["score"], a["m"], a["n"], a["D"], a["k"], 0, a["nbytes"]):
            if what == "null gallery" and op.i[0] == 2:
                continue                                   # the merge does not read the gallery
            rc = L.lib().omni_op_launch(ctypes.byref(op), L._stream_ptr(None))
            assert rc == E_ARG, (what, op.i[0], rc)
            seen.append((what, L.lib().omni_last_error().decode()))
    sync()
    assert bool((d["idx"].cpu() == -7).all()) and bool((d["score"].cpu() == -7.0).all()) and bool((d["part"].cpu() == 0x5A5A5A5A).all())
    for op in match_ops(p["q"], p["g"], p["part"], p["idx"], p["score"], m, n, D, k, 0, nbytes):
        L.launch(op)
    sync()
    assert d["idx"].cpu()[:m * k].view(m, k).tolist() == reference(Q, G, k)[2].tolist()
    assert bool((d["idx"].cpu()[m * k:] == -7).all()) and bool((d["score"].cpu()[m * k:] == -7.0).all())
    # mode 0 refuses the same kinds of argument
    from omniparser_amd.florence import embed_op
    x = torch.zeros(2, 16).to(dev)
    y, nm = torch.full((2, 8), -7.0).to(dev), torch.full((2,), -7.0).to(dev)
    for n_, ld, D_ in ((0, 16, 8), (2, 16, 6), (2, 4, 8), (2, 16, 4100)):
        rc = L.lib().omni_op_launch(ctypes.byref(embed_op(L.F32, x.data_ptr(), ld, y, nm, n_, D_)), L._stream_ptr(None))
        assert rc == E_ARG, (n_, ld, D_, rc)
    rc = L.lib().omni_op_launch(ctypes.byref(embed_op(L.F32, None, 16, y, nm, 2, 8)), L._stream_ptr(None))
    assert rc == E_ARG
    sync()
    assert bool((y.cpu() == -7.0).all()) and bool((nm.cpu() == -7.0).all())
    return seen


# ---------------------------------------------------------------------------------------------- captioner
N_CROPS, R_SMALL = 4, 64
EMBED_SEEDS = (403, 404, 405, 406)       # pixel seeds of the comparisons with transformers (gen_ctrl_checks.pixels)
TOL_EMBED_F32 = 1e-4                      # gpu_checks.rel_err bound the project asserts for img_feat at this size (test_models_emu_cpu.py)
# f16 plans: gpu_checks.rel_err of embed(pixel_values) against the f64 reference, measured on the MI355X over EMBED_SEEDS
# (profiles/visual_match_f16_vs_f64.txt); the bound is twice the worst of them, the margin because four seeds are a handful
MEASURED_F16 = (2.3988e-03, 2.1142e-03, 2.2985e-03, 1.8956e-03)
TOL_EMBED_F16 = 2 * max(MEASURED_F16)     # 4.80e-3; f32 plans measured 1.2e-6 .. 1.6e-6 on the same seeds
_REF, _CAPS = {}, {}


def f64_embeddings(seed, n=N_CROPS, R=R_SMALL):
    """transformers on the CPU in f64, once per seed: get_image_features(pix.double()).pooler_output[:, 0], L2-normalised"""
    import gen_ctrl_checks as GC
    from tools.make_weights import shared_random_captioner
    key = (seed, n, R)
    if key not in _REF:
        pix = GC.pixels(seed) if (n, R) == (GC.N_CROPS, GC.R) else torch.randn(n, 3, R, R, generator=torch.Generator().manual_seed(seed))
        model = shared_random_captioner(0)
        with torch.inference_mode():
            m64 = model.model.double()
            try:
                row0 = m64.get_image_features(pix.double()).pooler_output[:, 0].clone()
            finally:
                model.model.float()
        _REF[key] = (pix, row0 / row0.norm(dim=1, keepdim=True))
    return _REF[key]


def captioner(precision="f32", R=R_SMALL):
    """f32 at 64x64: the captioner the generation-control and vocabulary tests share; else one per (precision, resolution)"""
    import gen_ctrl_checks as GC
    from omniparser_amd.florence import Florence2Captioner
    from tools.make_weights import ensure_caption_checkpoint
    if (precision, R) == ("f32", GC.R):
        return GC.captioner(False)
    if (precision, R) not in _CAPS:
        _CAPS[(precision, R)] = Florence2Captioner(ensure_caption_checkpoint(0), "cuda", precision=precision, resolution=R)
    return _CAPS[(precision, R)]


def embed_vs_f64(cap, seed, device_pixels=False):
    """gpu_checks.rel_err of cap.embed(pixels of `seed`) against the f64 reference; unit length within f32 rounding"""
    import gpu_checks as G
    pix, ref = f64_embeddings(seed)
    emb = cap.embed(_dev(pix) if device_pixels else pix)
    assert emb.dtype == torch.float32 and tuple(emb.shape) == (pix.shape[0], cap.w.d_model)
    got = emb.cpu().double()
    assert float((got.norm(dim=1) - 1).abs().max()) < 1e-6
    e = G.rel_err(got, ref)
    print(f"embed vs transformers f64: seed {seed}, plan dtype {'f32' if cap.dtype == 0 else 'f16'}: rel_err {e:.3e}")
    return e


def _sync():
    if torch.cuda.is_available():
        torch.cuda.synchronize()


def _dev(t):
    """onto the device the product runs on: the GPU, or the host under the emulation"""
    import gpu_checks as G
    return t.to(G.DEV)


DECODER_KINDS = ("OP_ASSEMBLE", "OP_ATTN_DECODE", "OP_EMBED_STEP", "OP_GREEDY_STEP", "OP_BEAM_STEP", "OP_GREEDY_CTRL_STEP",
                 "OP_GREEDY_VOCAB_STEP")


def check_embed_plan(cap, L, R=R_SMALL, n=N_CROPS, max_new=20, device_pixels=False, seed=EMBED_SEEDS[0]):
    """the embed plan holds no encoder / decoder op and ends in mode 0; its ops in front of that are the caption plan's own first ops,
    slot for slot; its result is torch.equal to mode 0 launched on img_feat of the full caption plan after a generate on the same pixels"""
    from omniparser_amd.florence import embed_op
    pix = torch.randn(n, 3, R, R, generator=torch.Generator().manual_seed(seed))
    px = _dev(pix) if device_pixels else pix
    _sync()
    cap.clear_plans()
    emb = cap.embed(px)
    keys = [k for k in cap._plans if "embed" in k]
    assert len(cap._plans) == 1 and len(keys) == 1, list(cap._plans)
    plan = cap._plans[keys[0]]
    assert plan is cap.embed_plans(cap.bucket(n), R) and plan.step_plan is None and plan.cross_kv == []
    kinds = [op.kind for op in plan.encode_plan.ops]
    banned = {getattr(L, name) for name in DECODER_KINDS}
    assert not banned & set(kinds), sorted(banned & set(kinds))
    # OMNI_OP_ATTN_ROWS is also the kind of DaViT's window attention (i12 = 1); the BART encoder's self-attention is its sequence form
    rows_attn = [op.i[12] for op in plan.encode_plan.ops if op.kind == L.OP_ATTN_ROWS]
    assert rows_attn and all(form == 1 for form in rows_attn), rows_attn
    last = plan.encode_plan.ops[-1]
    assert last.kind == L.OP_VISUAL_MATCH and last.i[0] == 0 and kinds.count(L.OP_VISUAL_MATCH) == 1
    cap.generate(pixel_values=px, max_new_tokens=max_new)
    full = cap.plans(cap.bucket(n), R, max_new)
    assert L.OP_VISUAL_MATCH not in [op.kind for op in full.encode_plan.ops] and L.OP_ASSEMBLE in [op.kind for op in full.encode_plan.ops]
    assert 0 in [op.i[12] for op in full.encode_plan.ops if op.kind == L.OP_ATTN_ROWS], "the caption plan's encoder has no sequence-form attention"
    head = full.encode_plan.ops[:len(kinds) - 1]
    assert [(a.kind, a.dtype, list(a.i), list(a.f)) for a in head] == [(b.kind, b.dtype, list(b.i), list(b.f)) for b in plan.encode_plan.ops[:-1]]
    D = cap.w.d_model
    out = torch.empty((n, D), dtype=torch.float32, device=emb.device)
    norm = torch.empty((n,), dtype=torch.float32, device=emb.device)
    _sync()
    L.launch(embed_op(cap.dtype, full.img_feat.ptr, full.n_img * D, out, norm, n, D))
    _sync()
    assert torch.equal(emb, out), float((emb - out).abs().max())
    assert bool((norm > 0).all())
    return emb


class PooledPixels:
    """a stand-in embedder for the host tests of the public surface (an emulated encode per call would take minutes): the crop,
    average-pooled to 16 x 16 x 3 = 768 values, centred and L2-normalised — a pure function of the crop's pixels, like the real one.
    `match` is the real one: OMNI_OP_VISUAL_MATCH on the emulation."""

    def __init__(self):
        from types import SimpleNamespace
        self.device, self.w = torch.device("cpu"), SimpleNamespace(d_model=768)

    def embed_crops(self, image_u8, boxes_px, batch_size=128):
        rows = []
        for x0, y0, x1, y1 in boxes_px:
            crop = image_u8[y0:y1, x0:x1].permute(2, 0, 1).double()[None]
            v = torch.nn.functional.adaptive_avg_pool2d(crop, 16).flatten()
            v = v - v.mean()
            rows.append((v / v.norm().clamp_min(1e-30)).float())
        return torch.stack(rows) if rows else torch.zeros((0, 768))

    def match(self, queries, gallery, top_k=1):
        from omniparser_amd.florence import match_topk
        return match_topk(queries, gallery, top_k)


def check_entry_points(cap, R=R_SMALL, n_boxes=3, max_new=20, beams=True, lean=False):
    """caption_crops(return_embeddings=True): ids torch.equal to the call without the flag, embeddings torch.equal to embed_crops on
    the same boxes (also under beam search: img_feat does not depend on the decoding mode); embed_crops equals embed on the crops'
    pixel values; return_embeddings builds no embed plan"""
    import gpu_checks as G
    from omniparser_amd.synth import synthetic_screenshot
    frame = _dev(torch.from_numpy(synthetic_screenshot(5)))
    boxes = G.real_crop_boxes(5, n_boxes)
    _sync()
    cap.clear_plans()
    plain = cap.caption_crops(frame, boxes, max_new_tokens=max_new)
    ids, emb = cap.caption_crops(frame, boxes, max_new_tokens=max_new, return_embeddings=True)
    assert torch.equal(ids, plain) and not [k for k in cap._plans if "embed" in k]
    via_crops = cap.embed_crops(frame, boxes)
    assert emb.dtype == torch.float32 and tuple(emb.shape) == (n_boxes, cap.w.d_model)
    assert torch.equal(emb, via_crops)
    assert len(cap._plans) == 2 and len([k for k in cap._plans if "embed" in k]) == 1, list(cap._plans)
    if not lean:                          # (the emulated twin stops short: every call is an emulated encode)
        ids2, lp2, emb_s = cap.caption_crops(frame, boxes, max_new_tokens=max_new, return_scores=True, return_embeddings=True)
        assert torch.equal(ids2, plain) and lp2.shape[0] == n_boxes and torch.equal(emb_s, via_crops)
    cp = cap.plans(cap.bucket(n_boxes), R, max_new)
    G._fill_rows(cap, cp, frame, boxes, list(range(n_boxes)))
    _sync()
    crop_px = cp.x_in.t[:n_boxes, :, :, :3].permute(0, 3, 1, 2).float().clone()
    assert torch.equal(cap.embed(crop_px), via_crops)
    if beams:
        ids_b, emb_b = cap.caption_crops(frame, boxes, max_new_tokens=max_new, num_beams=3, return_embeddings=True)
        assert torch.equal(emb_b, via_crops) and torch.equal(ids_b, cap.caption_crops(frame, boxes, max_new_tokens=max_new, num_beams=3))
    if lean:
        return via_crops
    none_ids, none_emb = cap.caption_crops(frame, [], return_embeddings=True)
    assert none_ids.shape[0] == 0 and tuple(none_emb.shape) == (0, cap.w.d_model) and tuple(cap.embed_crops(frame, []).shape) == (0, cap.w.d_model)
    return via_crops


def check_unchanged_defaults(cap, max_new=20, n_boxes=3, device_pixels=False):
    """generate and caption_crops with defaults: the same plan keys and the same ids before and after the captioner has embedded, and
    beside the one embed plan no key that was not there before"""
    import gen_ctrl_checks as GC
    import gpu_checks as G
    from omniparser_amd.synth import synthetic_screenshot
    pix = GC.pixels()
    px = _dev(pix) if device_pixels else pix
    frame = _dev(torch.from_numpy(synthetic_screenshot(5)))
    boxes = G.real_crop_boxes(5, n_boxes)
    _sync()
    cap.clear_plans()
    first = (cap.generate(pixel_values=px, max_new_tokens=max_new), cap.caption_crops(frame, boxes, max_new_tokens=max_new))
    never = set(cap._plans)
    assert not [k for k in never if "embed" in k]
    cap.embed(px)
    cap.embed_crops(frame, boxes)
    cap.caption_crops(frame, boxes, max_new_tokens=max_new, return_embeddings=True)
    again = (cap.generate(pixel_values=px, max_new_tokens=max_new), cap.caption_crops(frame, boxes, max_new_tokens=max_new))
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    assert {k for k in cap._plans if "embed" not in k} == never and len(set(cap._plans) - never) == 1
    _sync()
    cap.clear_plans()
    cap.generate(pixel_values=px, max_new_tokens=max_new)
    cap.caption_crops(frame, boxes, max_new_tokens=max_new)
    assert set(cap._plans) == never


# ---------------------------------------------------------------------------------------------- public surface
BOXES = [[0.1, 0.1, 0.2, 0.2], [0.3, 0.3, 0.5, 0.4], [0.6, 0.2, 0.8, 0.5]]       # the three boxes of the vocabulary test
SELF_SCORE, SAME_SCORE = 1 - 1e-5, 1e-6


def elements_of(boxes=BOXES):
    return [{"type": "icon", "bbox": list(b), "interactivity": True, "content": None} for b in boxes]


def check_public_surface(cap, proc=None):
    """self-match, min_score / top_k, ScreenParser.embed / match / track, tracking across a rolled frame and against an unrelated one"""
    import numpy as np
    from PIL import Image
    from omniparser_amd.pipeline import ScreenParser
    from omniparser_amd.synth import synthetic_screenshot
    from omniparser_amd.util import utils as U
    cmp_ = {"model": cap, "processor": proc}
    arr = synthetic_screenshot(5)
    H, W = arr.shape[:2]
    els = elements_of() + [{"type": "icon", "bbox": [0.5, 0.5, 0.5, 0.6], "content": None}]          # the last crop is empty: skipped
    px = U.crop_boxes_px(BOXES, W, H)
    index, emb = U.embed_elements(arr, els, cmp_)
    assert index == [0, 1, 2] and tuple(emb.shape) == (3, cap.w.d_model) and emb.dtype == torch.float32
    assert torch.equal(emb, cap.embed_crops(_dev(torch.from_numpy(arr)), px))
    # ---- self-match: the frame's own crops as exemplar images (numpy and PIL)
    crops = [np.ascontiguousarray(arr[y0:y1, x0:x1]) for x0, y0, x1, y1 in px]
    exemplars = [crops[0], Image.fromarray(crops[1]), crops[2]]
    lists = U.match_elements(arr, els, cmp_, exemplars, top_k=3)
    assert len(lists) == 3 and all(len(r) == 3 for r in lists)
    for e, r in enumerate(lists):
        own = [x for x in r if x["index"] == e]
        print(f"exemplar {e}: {[(x['index'], round(x['score'], 7)) for x in r]}")
        assert own and own[0]["score"] >= SELF_SCORE and abs(own[0]["score"] - r[0]["score"]) <= SAME_SCORE, (e, r)
        assert all(r[k]["score"] >= r[k + 1]["score"] for k in range(2))
    by_tensor = U.match_elements(arr, els, cmp_, emb, top_k=3)
    assert [[x["index"] for x in r] for r in by_tensor] == [[x["index"] for x in r] for r in lists]
    # ---- top_k and min_score cut the lists
    top2 = U.match_elements(arr, els, cmp_, exemplars, top_k=2)
    assert top2 == [r[:2] for r in lists]
    cut = max(r[1]["score"] for r in lists)
    if cut < SELF_SCORE:
        strict = U.match_elements(arr, els, cmp_, exemplars, top_k=3, min_score=(cut + SELF_SCORE) / 2)
        assert strict == [[x for x in r if x["score"] >= (cut + SELF_SCORE) / 2] for r in lists] and all(len(r) >= 1 for r in strict)
    assert U.match_elements(arr, els, cmp_, exemplars, top_k=3, min_score=2.0) == [[], [], []]
    assert U.match_elements(arr, [], cmp_, exemplars, top_k=3) == [[], [], []]
    for bad in (0, 9, True, 2.0):
        try:
            U.match_elements(arr, els, cmp_, exemplars, top_k=bad)
        except ValueError:
            continue
        raise AssertionError(f"top_k={bad!r} was accepted")
    # ---- tracking: the frame rolled by (dx, dy), the boxes moved with it: byte-identical crops
    dx, dy = 37, 21
    rolled = np.roll(arr, (dy, dx), axis=(0, 1))
    moved = [[(x0 + dx + 0.5) / W, (y0 + dy + 0.5) / H, (x1 + dx + 0.5) / W, (y1 + dy + 0.5) / H] for x0, y0, x1, y1 in px]
    here = [[(x0 + 0.5) / W, (y0 + 0.5) / H, (x1 + 0.5) / W, (y1 + 0.5) / H] for x0, y0, x1, y1 in px]
    px_m = U.crop_boxes_px(moved, W, H)
    assert U.crop_boxes_px(here, W, H) == px and px_m == [[x0 + dx, y0 + dy, x1 + dx, y1 + dy] for x0, y0, x1, y1 in px]
    assert all(np.array_equal(rolled[b[1]:b[3], b[0]:b[2]], arr[a[1]:a[3], a[0]:a[2]]) for a, b in zip(px, px_m))
    prev, cur = U.embed_elements(arr, elements_of(here), cmp_), U.embed_elements(rolled, elements_of(moved), cmp_)
    assert torch.equal(prev[1], cur[1]) and torch.equal(prev[1], emb)
    pairs = U.track_elements(prev, cur)
    sim = (prev[1].cpu().double() @ cur[1].cpu().double().T)
    print(f"track: {pairs}; similarities {sim.tolist()}")
    assert [p[0] for p in pairs] == [0, 1, 2] and sorted(p[1] for p in pairs) == [0, 1, 2]
    for i, j, s in pairs:
        assert s >= SELF_SCORE and (j == i or abs(float(sim[i, j]) - float(sim[i, i])) <= SAME_SCORE), (i, j, s)
    other = np.random.default_rng(7).integers(0, 256, size=arr.shape, dtype=np.uint8)
    far = U.embed_elements(other, elements_of(here), cmp_)
    print(f"unrelated frame: similarities {(prev[1].cpu().double() @ far[1].cpu().double().T).tolist()}")
    assert U.track_elements(prev, far, min_score=0.999) == []
    assert U.track_elements(prev, ([], far[1][:0])) == [] and U.track_elements(([], emb[:0]), cur) == []
    # ---- ScreenParser: frames already on the device
    sp = ScreenParser(None, cap, processor=proc)
    f0, f1 = _dev(torch.from_numpy(arr)), _dev(torch.from_numpy(rolled))
    i_sp, e_sp = sp.embed(f0, els)
    assert i_sp == index and torch.equal(e_sp, emb)
    assert sp.match(f0, els, exemplars, top_k=3) == lists
    assert sp.track(f0, elements_of(here), f1, elements_of(moved)) == pairs
    return lists, pairs


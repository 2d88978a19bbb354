"""Wv folded into channel attention's per-image projection (Florence2Captioner.fold_chan_v) on the host emulation of the kernels
(tests/emu): the checks of tests/chan_vfold_checks.py, which tests/test_gpu_v_chan_vfold.py runs on the MI355X."""


def test_bias_table_chain_bound_and_scale_product(emu):
    import chan_vfold_checks as C
    assert set(C.check_bias_table_and_scale()) == {128, 256, 512}


def test_fold_gemm_vs_f64_and_repacked_bits(emu):
    import chan_vfold_checks as C
    assert len(C.check_fold_gemm()) == 12


def test_gemm_with_per_image_bias(emu):
    import chan_vfold_checks as C
    assert C.check_per_image_bias()["worst_rel_err"] < 2e-6


def test_channel_block_tail_three_forms_vs_f64(emu):
    import chan_vfold_checks as C
    assert len(C.check_block_tail()) == 3


def test_switch_off_is_the_parent_op_list_and_on_drops_the_v_launch():
    """768x768 plans built on the CPU (no kernel runs): with fold_chan_v off no op carries a new slot (OMNI_OP_CHAN_ATTN i11, OMNI_OP_CONV
    i29, the fold GEMM's i26 > 0 with i27 = 0 outside the scores epilogue) and the folded blocks are q|k, v, chan_attn, projection; with it
    on every folded block is q|k, chan_attn (i11 = 1), fold GEMM, re-pack (OMNI_OP_SPLIT_CONVERT i6 = 1), projection on the block's LayerNorm output with a
    per-image bias — no OMNI_OP_CONV writes format B into a qkv slice — and the algorithmic FLOPs of the encode plan are the same."""
    import caption_checks as CC
    import caption_f64 as CF
    from omniparser_amd import _lib as L
    from omniparser_amd import florence as FL
    from tools.make_weights import ensure_caption_checkpoint
    d = ensure_caption_checkpoint(0)
    assert FL.Florence2Captioner.fold_chan_v is True
    plans = {}
    cap, cp = CC.build_cpu_plans(d, CF.B2, 768)
    plans[True] = (list(cp.encode_plan.ops), cp.encode_flops, list(cp.fold_stages))
    cap.fold_chan_v = False                                   # the same stand-in captioner (and weight cache) with the switch off
    cp_off = FL._CaptionPlans(cap, CF.B2, 768, 20)
    plans[False] = (list(cp_off.encode_plan.ops), cp_off.encode_flops, list(cp_off.fold_stages))
    ops, flops, stages = plans[False]
    assert stages == [0, 1, 2]
    fold_gemm = lambda op: op.kind == L.OP_CONV and op.i[20] == 2 and op.i[26] > 0 and op.i[27] == 0 and op.i[28] == 0   # noqa: E731
    assert not any(op.i[29] for op in ops if op.kind == L.OP_CONV) and not any(op.i[11] for op in ops if op.kind == L.OP_CHAN_ATTN)
    assert not any(op.i[6] for op in ops if op.kind == L.OP_SPLIT_CONVERT)
    assert not any(fold_gemm(op) for op in ops)
    folded = [j for j, op in enumerate(ops) if op.kind == L.OP_CHAN_ATTN and op.i[8] == 1]
    assert len(folded) == 11
    for j in folded:
        assert ops[j - 2].i[28] == 1 and ops[j - 1].i[21] == 1 and ops[j + 1].i[26] == ops[j].i[1] and ops[j + 1].i[5] == 2 * ops[j].i[3]
    ops, flops_on, stages = plans[True]
    assert stages == [0, 1, 2] and flops_on == flops
    first = [j for j, op in enumerate(ops) if op.kind == L.OP_CHAN_ATTN and op.i[11] == 1]
    assert len(first) == 11 and sum(1 for op in ops if fold_gemm(op)) == 11
    for j in first:
        C, N = ops[j].i[3], ops[j].i[1]
        assert ops[j - 1].kind == L.OP_CONV and ops[j - 1].i[28] == 1
        assert fold_gemm(ops[j + 1]) and ops[j + 1].i[26] == C and ops[j + 1].i[3] == C and ops[j + 1].i[12] == C and not ops[j + 1].p[2]
        assert ops[j + 2].kind == L.OP_SPLIT_CONVERT and ops[j + 2].i[6] == 1 and ops[j + 2].i[3] == C and ops[j].i[8] == 1 and not ops[j].p[4]
        proj = ops[j + 3]
        assert proj.kind == L.OP_CONV and proj.i[29] == 1 and proj.i[26] == N and proj.i[5] == 0 and proj.i[4] == C and proj.p[0] == ops[j - 1].p[0]
    # nothing writes format B into a slice of a wider buffer in stages 0-2 (the v slice of qkv): the only such launch was the v launch
    assert not any(op.kind == L.OP_CONV and op.i[21] == 1 and op.i[13] == 3 * op.i[12] for op in ops)

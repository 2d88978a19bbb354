"""Folded channel attention on the host emulation of the kernels (tests/emu): the per-image LDS-DMA GEMM, the softmax + fold + pack
kernels and a channel block's tail both ways — the checks of tests/chan_fold_checks.py, which tests/test_gpu_r_chan_fold.py runs on
the MI355X."""


def test_gemm_with_per_image_weights_vs_f64(emu):
    import chan_fold_checks as C
    r = C.check_gemm_per_image()
    assert r["worst_rel_err"] < 2e-6 and all(r["bitwise_same_matrix"].values())


def test_fold_kernels_chain_bound_and_packed_bits(emu):
    import chan_fold_checks as C
    r = C.check_fold()
    assert set(r) == {128, 256}


def test_channel_block_tail_folded_and_unfolded_vs_f64(emu):
    import chan_fold_checks as C
    r = C.check_composition()
    assert len(r) == 2

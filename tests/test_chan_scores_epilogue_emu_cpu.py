"""Scores epilogue of the LDS-DMA GEMM on the host emulation of the kernels (tests/emu): the checks of tests/chan_scores_epi_checks.py,
which tests/test_gpu_u_chan_scores_epilogue.py runs on the MI355X."""


def test_scores_epilogue_bitwise_vs_standalone_scores(emu):
    import chan_scores_epi_checks as C
    r = C.check_scores_bitwise()
    assert len(r) == 8 and all(r.values())


def test_scores_epilogue_writes_no_y_and_stays_inside_ws(emu):
    import chan_scores_epi_checks as C
    assert C.check_y_not_written()


def test_scores_epilogue_argument_errors(emu):
    import chan_scores_epi_checks as C
    assert len(C.check_argument_errors()) == 7


def test_softmax_sums_partials_in_ascending_chunk_order(emu):
    import chan_scores_epi_checks as C
    assert set(C.check_softmax_order()) == {1, 2, 9, 144}


def test_tokens_per_partial_is_the_op_at_that_chunk(emu):
    import chan_scores_epi_checks as C
    assert C.check_partial_tokens_bitwise()


def test_tokens_per_partial_vs_f64(emu):
    """caption_f64.EMU_TIER's channel-attention shapes up to C = 512, with i5 = 1024, i10 = 256"""
    import chan_scores_epi_checks as C
    assert len(C.check_partial_tokens_f64(shapes=((2500, 4), (300, 8), (150, 16)))) == 12

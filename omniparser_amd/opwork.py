"""Algorithmic work of one plan op (`omni_op_t`): FLOPs, bytes, a shape key and the kernel family that executes it.

"Algorithmic" = every operand read once and every result written once (weights included) — the traffic a perfectly cached execution
of the op list needs; FLOPs are 2 x MAC for GEMMs / attention.  `bench.py::roofline` divides these by the HIP-event time of the
launches (`omni_plan_profile`) for its `achieved` figure and its `per_kernel` list; `tools/plan_table.py` and
`tools/caption_profile.py` print tables from the same functions, so the bench line and the committed tables cannot disagree.
Slot meanings: include/omni_amd.h."""

NAMES = {1: "conv_igemm/conv_split", 2: "avgpool2", 3: "maxpool", 4: "resize_nearest", 5: "letterbox", 6: "detect_decode", 7: "nms",
         8: "dwconv3", 9: "layernorm", 10: "attn_rows (window / MHA)", 11: "chan_attn", 12: "proj_prep", 13: "assemble", 14: "embed_step",
         15: "attn_decode", 16: "greedy_step", 17: "crop_resize", 18: "dwconv3_ln", 19: "split_convert", 20: "hand_off", 21: "overlay",
         22: "png_pack", 23: "png_deflate", 24: "mlp_fused", 26: "greedy_ctrl_step", 28: "visual_match", 29: "region_ocr"}

MFMA_KINDS = (1, 24, 10)          # priced against the dense f16 MFMA peak; everything else against HBM


def op_work(op, esz=4):
    """(flops, algorithmic bytes) of one op."""
    i = op.i
    k = op.kind
    if k == 1:
        M, N, K = i[0] * i[10] * i[11], i[12], i[6] * i[7] * i[3]
        if i[25]:                                   # row-patch mode: algorithmic K = k x k taps x 4 stored channels (the op's 32 k holds zero weights)
            K = i[6] * i[6] * i[4]
            return 2 * M * N * K, esz * (i[0] * i[1] * i[2] * i[4] + N * K + M * N)
        if i[20] == 2 and i[28] == 1:               # scores epilogue: no y, one 4 KB partial per 256-row chunk and 64-column group
            return 2 * M * N * K + 2 * M * N * 16, esz * (M * K + N * K + (M // 256) * (N // 64) * 1024)
        nw = M // i[26] if (i[20] == 2 and i[26] > 0) else 1          # per-image weights: one matrix per image
        if i[20] == 2 and i[26] > 0 and i[27] == 0:  # the fold GEMM W''_b = W'_b . Wv: not work of the network (its 2 M N K MACs run, but the
            return 0, esz * (M * K + N * K + M * N)  # count keeps the v layer instead, below), operands read and written once
        if i[20] == 2 and i[29] == 1:                # projection with Wv folded in: carries the v layer's algorithmic work too (K = N = C)
            return 4 * M * N * K, esz * (i[0] * i[1] * i[2] * i[3] + nw * N * K + nw * N + M * N * (2 if op.p[3] else 1))
        return 2 * M * N * K, esz * (i[0] * i[1] * i[2] * i[3] + nw * N * K + M * N * (2 if op.p[3] else 1))
    if k == 24:                                     # fc1 + GELU + fc2 + residual: h in, residual in, y out, both weight matrices
        rows, C, hid = i[0] * max(i[1], 1), i[3], i[12]
        return 4 * rows * C * hid, esz * (3 * rows * C + 2 * C * hid)
    if k == 19 and i[6] == 1:                       # re-pack of W'' = W' . Wv: f32 matrices in, format B out
        return 0, esz * 2 * i[0] * i[3] * i[3]
    if k in (2, 3, 4):
        return 0, esz * (i[0] * i[1] * i[2] * i[3] + i[0] * max(i[10], 1) * max(i[11], 1) * i[3])
    if k in (8, 18):
        n = i[0] * i[1] * i[2] * i[3]
        return 18 * n, esz * n * (2 if k == 8 else 3)
    if k == 9:
        n = i[0] * max(i[1], 1) * i[3]
        return 8 * n, esz * 2 * n
    if k == 10:
        heads, nq, nk, groups, D = i[8], i[9], i[10], i[11], i[15]
        return 4 * groups * heads * nq * nk * D, esz * groups * (nq + 2 * nk + nq) * heads * D
    if k == 11:
        B, N, C = i[0], i[1], i[3]
        if i[8] == 1 and i[9] == 1:                 # fold mode behind the scores epilogue: reads the partials instead of q and k
            ct = i[10] or i[5]                      # tokens per partial
            chunks = (N + ct - 1) // ct
            return 2 * B * C * C * 32, esz * (B * (C // 32) * chunks * 1024 + C * C + B * C * C)
        if i[8] == 1:                               # fold mode: scores over q and k, then W'_b = Wp . blockdiag(A) written once per image
            return 2 * B * N * C * 32 + 2 * B * C * C * 32, esz * (B * N * C * 2 + C * C + B * C * C)
        return 4 * B * N * C * 32, esz * B * N * C * 4
    if k == 15:
        B, heads, nk = i[10], i[6], (i[7] if i[7] > 0 else i[8])
        return 4 * B * heads * nk * 64, esz * B * nk * i[9] * 2
    if k in (16, 26):
        return 0, esz * i[0] * i[1]
    if k == 28:                                     # i0: 0 = embed (row 0 of every crop in, unit vector + norm out), 1 = partial top-k, 2 = merge
        if i[0] == 0:
            n, D = i[1], i[3]
            return 3 * n * D, n * D * (esz + 4) + 4 * n
        m, n, D, kk = i[1], i[2], i[3], i[4]
        ln = i[5] if i[5] > 0 else None             # (the launcher's split: one partial list per query and split; unknown here = 1 split)
        splits = (n + ln - 1) // ln if ln else 1
        if i[0] == 1:                               # queries and gallery once (a perfectly cached execution), the partials out
            return 2 * m * n * D, 4 * (m + n) * D + 8 * m * splits * kk
        return 0, 8 * m * splits * kk + 8 * m * kk
    if k == 29:                                     # i0: 0 = tile cut (u8 window in, normalised pixels out), 1 = region parse, 3 = box parse,
        if i[0] == 0:                               # 5 = polygon parse, 6 = mask raster
            n, R, ldo = i[1], i[4], i[13]
            return 2 * 3 * n * R * R, n * R * R * (3 + ldo * esz)
        if i[0] == 5:                               # as the parses, plus the vertex slots: a record and a sum per polygon slot, 8 bytes per vertex
            n, T, P, V = i[1], i[2], i[3], i[9]
            return 0, n * (4 * T + (4 * (T - 1) if op.p[2] else 0) + 68 * P + 8 * V + 16 + 24)
        if i[0] == 6:                               # records, rows, vertices and origins in (once: the blocks of a row share them in cache),
            n, T, I, R = i[1], i[2], i[3], i[7]     # mask words and counts out; no flops: the edge tests are 64-bit integer work
            return 0, n * (64 * (T // 2) + 8 * ((T - 1) // 2) + 16 + 24 + I * R * (4 * ((R + 31) // 32) + 4))
        n, T, M = i[1], i[2], i[3]                  # ids and log-probabilities in, records, sums and row counters out (class table: cached)
        slot = 72 if i[0] == 3 else 68              # a record of 16 ints and one sum (boxes: two)
        return 0, n * (4 * T + (4 * (T - 1) if op.p[2] else 0) + slot * M + 16 + 24)
    return 0, 0


def op_shape(op):
    """(rows, channels out, K or a variant tag): the key launches are grouped by."""
    i, k = op.i, op.kind
    if k in (1, 19):
        return (i[0] * max(i[10], 1) * max(i[11], 1) if k == 1 else i[0] * max(i[1], 1), i[12] if k == 1 else i[3], i[6] * i[7] * i[3] if k == 1 else 0)
    if k == 24:
        return (i[0] * max(i[1], 1), i[3], i[12])
    if k in (8, 18):
        return (i[0] * i[1] * i[2], i[3], 0)
    if k == 9:
        return (i[0] * max(i[1], 1), i[3], i[6])
    if k == 10:
        return (i[11] * i[9], i[8] * i[15], i[12])
    if k == 11:
        return (i[0] * i[1], i[3], (2 if i[9] == 1 else 1) if i[8] == 1 else 0)
    if k == 15:
        return (i[10], i[9], i[7] if i[7] > 0 else i[8])
    if k == 28:                                     # embed: (crops, D, 0); match: (queries, D, gallery rows)
        return (i[1], i[3], 0 if i[0] == 0 else i[2])
    if k == 29:                                     # cut: (tiles, R, 0); parse, boxes and polygons: (rows, T, 0); masks: (rows, R, instance slots)
        if i[0] == 6:
            return (i[1], i[7], i[3])
        return (i[1], i[4] if i[0] == 0 else i[2], 0)
    return (i[0], i[3], 0)


def op_kernel(op):
    """the kernel family a launch of this op runs (kind 1 is served by three kernels, chosen by the planner: slot i20)."""
    if op.kind == 1:
        if op.i[20] == 2 and op.i[28] == 1:
            return "gemm_dma (scores epilogue)"
        if op.i[20] == 2 and op.i[26] > 0 and op.i[27] == 0:
            return "gemm_dma (fold W' . Wv)"
        if op.i[20] == 2 and op.i[26] > 0:
            return "gemm_dma (per-image weights + bias)" if op.i[29] == 1 else "gemm_dma (per-image weights)"
        return "gemm_dma" if op.i[20] == 2 else ("conv_split" if op.i[20] else "conv_igemm")
    if op.kind == 19 and op.i[6] == 1:
        return "split_convert (re-pack W'')"
    if op.kind == 11 and op.i[8] == 1:
        return "chan_attn (fold)" if op.i[9] == 1 else "chan_attn (scores + fold)"
    if op.kind == 28:
        return ("visual_match (embed)", "visual_match (partial top-k)", "visual_match (merge)")[op.i[0]] if 0 <= op.i[0] <= 2 else "visual_match"
    if op.kind == 29:
        return {0: "region_ocr (tile cut)", 1: "region_ocr (parse)", 3: "region_ocr (boxes)", 5: "region_ocr (polygons)",
                6: "region_ocr (masks)"}.get(op.i[0], "region_ocr")
    return NAMES.get(op.kind, str(op.kind))

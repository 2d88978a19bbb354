"""Checks shared by the CPU (emulation) and GPU tests of OMNI_OP_REGION_OCR and of the calls around it
(Florence2Captioner.read_regions, util.utils.read_text_regions / parse_ocr_regions / FlorenceOCR, Omniparser's "florence" provider).

Everything here is exact; there is no tolerance but one:
  mode 0   bit-equal to FlorenceProcessor(images=tile, do_resize=False) on the Pillow crop of the same window, pasted on a white
           canvas where the frame is smaller than the tile; the f16 case is that f32 result rounded to f16 once.
  mode 1   records, row counters and log-probability sums bit-equal to `twin_parse`, a literal restatement of the op's semantics
           (include/omni_amd.h) that shares no code with the kernel; for rows without a HARD token, texts and quads equal to
           transformers' Florence2PostProcessor (decode_with_spans + parse_ocr_from_text_and_spans) on the same ids; for rows with one,
           util.utils.parse_ocr_regions equals that oracle.
  confidence (GPU, captioner) the mean log-probability per region within the project's per-token tolerance of 1.38e-4
           (profiles/long_decode_tolerance.json) of transformers' compute_transition_scores over the same tokens.

The oracle's tokenizer: tests/golden/tokenizer_synth/tokenizer.json (400 byte-level BPE tokens; 31 = '<' and 202 = newline are HARD)
plus <loc_0>..<loc_999> added at ids 400..1399."""
import ctypes
import json
import shutil
from pathlib import Path

import numpy as np
import torch

import caption_f64 as CF

E_ARG = -1
GOLDEN_TOK = Path(__file__).resolve().parent / "golden" / "tokenizer_synth" / "tokenizer.json"
LOC0, N_TEXT = 400, 400
START, BOS, PAD, EOS = 2, 0, 1, 2
TOK_LT, TOK_NL = 31, 202
STRIP, TEXT, HARD = 1000, 1001, 1002
INF = 2 ** 31 - 1


# ---------------------------------------------------------------------------------------------- tokenizer, class table, oracle
def write_tokenizer(dst_dir, n_loc=1000, first=LOC0, shuffle=False):
    """tokenizer.json = the synthetic fixture + `n_loc` added tokens <loc_i> at ids first.. (shuffle: <loc_0> and <loc_1> swapped)"""
    dst = Path(dst_dir)
    dst.mkdir(parents=True, exist_ok=True)
    d = json.loads(GOLDEN_TOK.read_text())
    assert len(d["model"]["vocab"]) == N_TEXT == first
    names = [f"<loc_{i}>" for i in range(n_loc)]
    if shuffle:
        names[0], names[1] = names[1], names[0]
    d["added_tokens"] += [{"id": first + i, "content": t, "single_word": False, "lstrip": False, "rstrip": False, "normalized": False,
                           "special": False} for i, t in enumerate(names)]
    (dst / "tokenizer.json").write_text(json.dumps(d))
    return dst


_ORACLE = {}


def oracle(tmp_dir):
    """(FlorenceProcessor with the location tokens, transformers' Florence2PostProcessor over the same tokenizer file)"""
    if "v" not in _ORACLE:
        from transformers import PreTrainedTokenizerFast
        from transformers.models.florence2.processing_florence2 import Florence2PostProcessor
        from omniparser_amd.util import utils as U
        d = write_tokenizer(Path(tmp_dir) / "tok_loc")
        tok = PreTrainedTokenizerFast(tokenizer_file=str(d / "tokenizer.json"), bos_token="<s>", eos_token="</s>", pad_token="<pad>", unk_token="<unk>")
        _ORACLE["v"] = (U.FlorenceProcessor(d, image_token_id=1400, special_ids=(BOS, PAD, EOS, 3)), Florence2PostProcessor(None, tok))
    return _ORACLE["v"]


def oracle_regions(post, row, size):
    """transformers on one row (start token, generated ids ...; cut in front of the first EOS): [(text, quad)]"""
    end = next((j for j in range(1, len(row)) if row[j] == EOS), len(row))
    text, _ = post.decode_with_spans([int(t) for t in row[1:end]])
    return [(r["text"], [int(v) for v in r["quad_box"]]) for r in post.parse_ocr_from_text_and_spans(text, None, (size, size))]


def check_dequantize(R):
    """the integer form ((2 bin + 1) R) // 2000 equals Florence2PostProcessor.dequantize(...).int() for all 1000 bins"""
    from transformers.models.florence2.processing_florence2 import Florence2PostProcessor
    from omniparser_amd.util import utils as U
    post = Florence2PostProcessor.__new__(Florence2PostProcessor)
    post.quantize_bins = (1000, 1000)
    bins = torch.arange(1000)
    ref = post.dequantize(torch.stack([bins, bins], dim=1), size=(R, R))
    mine = torch.tensor([U.dequantize_bin(int(b), R) for b in bins], dtype=ref.dtype)
    assert torch.equal(ref[:, 0], mine) and torch.equal(ref[:, 1], mine), R


# ---------------------------------------------------------------------------------------------- mode 1: the literal twin
def twin_parse(ids, table, logp, cells, T, R, eos=EOS):
    """OMNI_OP_REGION_OCR mode 1 as include/omni_amd.h words it, on the host: ids [n, >= T] ints, table u16 numpy, logp f32 numpy
    [n, >= T - 1] or None, cells [n][6] -> (records i32 [n, M, 16], sums f32 [n, M], rows i32 [n, 4])"""
    n, M = len(ids), (T - 1) // 9
    rec, sums, rows = np.zeros((n, M, 16), np.int32), np.zeros((n, M), np.float32), np.zeros((n, 4), np.int32)
    for r in range(n):
        row = [int(t) for t in ids[r][:T]]
        end = next((j for j in range(1, T) if row[j] == eos), T)
        cls = [min(int(table[t]), HARD) if 0 <= t < len(table) else HARD for t in row[:end]]
        kept_cols = [j for j in range(1, end) if cls[j] != STRIP]
        is_loc = [cls[j] < 1000 for j in kept_cols]
        p = k = kept = 0
        while True:
            e = next((e for e in range(p + 1, len(kept_cols) - 7) if all(is_loc[e:e + 8])), None)
            if e is None:
                break
            cols = kept_cols[p:e + 8]
            total = np.float32(0.0)
            if logp is not None:
                for j in cols:
                    total = np.float32(total + np.float32(logp[r][j - 1]))
            quad = [((2 * cls[j] + 1) * R) // 2000 + cells[r][q & 1] for q, j in enumerate(kept_cols[e:e + 8])]
            cx, cy = min(quad[0::2]) + max(quad[0::2]), min(quad[1::2]) + max(quad[1::2])
            c = cells[r]
            own = c[2] <= cx and (c[3] == INF or cx < c[3]) and c[4] <= cy and (c[5] == INF or cy < c[5])
            rec[r, k, :13] = [r, kept_cols[p], kept_cols[e - 1] + 1, *quad, len(cols), int(own)]
            sums[r, k] = total
            kept += int(own)
            k += 1
            p = e + 8
        rows[r] = [k, kept, int(any(c == HARD for c in cls[1:])) | (2 if end == T else 0), 0]
    return rec, sums, rows


def region_text(row, rec, table, texts):
    """the text of a device record: the rendered non-STRIP tokens of its content columns, stripped"""
    return "".join(texts[t] for t in row[rec[1]:rec[2]] if table[t] != STRIP).strip()


# ---------------------------------------------------------------------------------------------- mode 1: rows
def loc(*bins):
    return [LOC0 + b for b in bins]


QUAD_A, QUAD_B = loc(10, 20, 500, 20, 500, 300, 10, 300), loc(0, 999, 999, 0, 1, 2, 3, 4)
A, B, C, SP = 36, 37, 38, 224          # 'A', 'B', 'C' and the byte-level space token (asserted in `parse_rows`)


def gen_cases(T):
    """{name: (generated tokens without the EOS, has an EOS)} — every case of the issue's list that fits a row of T tokens; a row
    is START + generated + [EOS] + garbage"""
    room = T - 2                          # generated tokens in front of an EOS
    cases = {
        "no_region": ([BOS, A, B, C], True),
        "eight_locs_no_content": ([BOS] + QUAD_A, True) if room >= 9 else ([BOS] + QUAD_A[:7], True),
        "one_token_and_quad_whole_row": ([A] + QUAD_A, T != 10),                      # at T = 10 it IS the row: no EOS fits
    }
    if room >= 10:
        cases["nine_locs"] = ([BOS] + loc(7) + QUAD_A, True)
        cases["whitespace_content"] = ([BOS, SP] + QUAD_B, True)
        cases["hard_lt"] = ([BOS, A, TOK_LT] + QUAD_A[:7], True)
    if room >= 17:
        cases["sixteen_locs"] = ([BOS] + QUAD_A + QUAD_B, True)
        cases["strips_inside"] = ([BOS, A, PAD, B] + QUAD_A[:2] + [BOS] + QUAD_A[2:7] + [PAD] + QUAD_A[7:], True)
        cases["id_beyond_table"] = ([BOS, A, 5000] + QUAD_A + [-3], True)
        cases["truncated_region_at_the_end"] = ([BOS] + [A] * (T - 1 - 9) + QUAD_B, False)
    if room >= 24:
        cases["seventeen_locs"] = ([BOS] + QUAD_A + QUAD_B + loc(5), True)
        cases["two_regions_back_to_back"] = ([BOS, A, B] + QUAD_A + [C] + QUAD_B, True)
        cases["hard_newline"] = ([BOS, A, TOK_NL, B] + QUAD_A + [C, A] + QUAD_B, True)
        cases["hard_lt_in_content"] = ([BOS, A, TOK_LT, B] + QUAD_A + [C] + QUAD_B, True)
        cases["no_eos_no_region"] = ([BOS] + [A, B, C] * ((T - 2) // 3) + [A] * ((T - 2) % 3), False)
    if T >= 1025:
        cases["every_slot"] = (([A] + QUAD_A) * ((T - 1) // 9) + QUAD_B[:(T - 1) % 9], False)      # M regions, more than 64 lanes
    for name, (g, eos) in cases.items():
        assert len(g) + (2 if eos else 1) <= T and (eos or len(g) == T - 1), (name, T, len(g))
    return cases


def parse_rows(T, n, seed=0):
    """n rows of T ids (numpy i32) and their log-probabilities f32 [n, T - 1], cycling through `gen_cases` from an offset that
    depends on T; behind a row's EOS: garbage ids (location tokens and EOS among them) and NaN log-probabilities"""
    cases = gen_cases(T)
    names = list(cases)
    rng = np.random.default_rng(1000 * T + n + seed)
    ids = np.zeros((n, T), np.int32)
    logp = np.full((n, T - 1), np.nan, np.float32)
    picked = []
    for r in range(n):
        name = names[(r + T) % len(names)] if n > 1 else names[(T // 9) % len(names)]
        g, eos = cases[name]
        row = [START] + g + ([EOS] if eos else [])
        used = len(row)
        junk = rng.choice(np.array(QUAD_A + QUAD_B + [EOS, A, 70000, -1, TOK_NL], dtype=np.int64), size=T - used)
        ids[r] = row + junk.tolist()
        logp[r, :used - 1] = -rng.random(used - 1, dtype=np.float32) * 3
        picked.append(name)
    return ids, logp, picked


def grid_cells(origins, R):
    from omniparser_amd.florence import ocr_cells
    return ocr_cells(origins, R)


def launch_parse(L, dev, sync, ids, table, logp, cells, T, R, pad_ids=2, pad_logp=3, what="region parse", slots=None):
    """one launch, every operand in one guard-banded arena; ids and logp rows are wider than their data (the padding holds 0xFF
    bytes: id -1, NaN).  -> (records [n, M, 16], sums [n, M], rows [n, 4]) as numpy"""
    from omniparser_amd.florence import region_parse_op
    n, M = ids.shape[0], (T - 1) // 9
    ar = CF.Arena()
    ar.add("ids", torch.int32, n, T + pad_ids, data=((0, torch.from_numpy(ids)),))
    ar.add("table", torch.int16, 1, len(table), data=((0, torch.from_numpy(table.astype(np.int16))[None]),))
    if logp is not None:
        ar.add("logp", torch.float32, n, T - 1 + pad_logp, data=((0, torch.from_numpy(logp)),))
    ar.add("cells", torch.int32, n, 6, data=((0, torch.tensor(cells, dtype=torch.int32)),))
    ar.add("rec", torch.int32, n * M, 16, out=((0, 16),))
    ar.add("sums", torch.float32, 1, n * M, out=((0, n * M),))
    ar.add("rows", torch.int32, n, 4, out=((0, 4),))
    ar.build(dev)
    op = region_parse_op(ar.ptr("ids"), ar.ptr("table"), ar.ptr("logp") if logp is not None else None, ar.ptr("cells"), ar.ptr("rec"),
                         ar.ptr("sums"), ar.ptr("rows"), n, T, len(table), R, EOS, ld_ids=T + pad_ids, ld_logp=T - 1 + pad_logp, slots=slots)
    L.launch(op)
    sync()
    ar.fetch(what)
    return (ar.get("rec", 0, 16).numpy().reshape(n, M, 16), ar.get("sums", 0, n * M).numpy().reshape(n, M), ar.get("rows", 0, 4).numpy())


def check_parse(L, dev, tmp_dir, T, n, R=64, sync=lambda: None, with_logp=True):
    """one launch of n synthetic rows of T tokens: bit-equal to the twin; texts and quads equal to transformers where no HARD token
    occurs, the host fallback equal to transformers where one does"""
    from omniparser_amd.util import utils as U
    proc, post = oracle(tmp_dir)
    table, texts = proc.loc_class_table()
    assert texts[SP] == " " and table[SP] == TEXT and table[TOK_LT] == HARD and table[TOK_NL] == HARD and table[A] == TEXT
    assert table[LOC0] == 0 and table[LOC0 + 999] == 999 and table[BOS] == table[PAD] == table[EOS] == STRIP and len(table) == 1400
    ids, logp, names = parse_rows(T, n)
    if not with_logp:
        logp = None
    origins = [(13 * (r % 3), 7 * (r % 2)) for r in range(n)]
    cells = [[ox, oy, -2 ** 31, INF, -2 ** 31, INF] for ox, oy in origins]
    rec, sums, rows = launch_parse(L, dev, sync, ids, table, logp, cells, T, R)
    t_rec, t_sums, t_rows = twin_parse(ids, table, logp, cells, T, R)
    assert np.array_equal(rows, t_rows), (names, rows.tolist(), t_rows.tolist())
    assert np.array_equal(rec, t_rec), names
    assert np.array_equal(sums.view(np.int32), t_sums.view(np.int32)), names
    assert not np.isnan(sums).any()
    seen = {"regions": 0, "hard": 0, "truncated": 0}
    for r, name in enumerate(names):
        row = ids[r].tolist()
        found, _kept, flags = (int(v) for v in rows[r, :3])
        seen["regions"] += found
        seen["hard"] += flags & 1
        seen["truncated"] += (flags >> 1) & 1
        if "beyond_table" in name:                          # transformers cannot render an id its tokenizer does not know
            assert flags & 1
            continue
        ox, oy = origins[r]
        want = oracle_regions(post, row, R)
        if flags & 1:
            got = [(g["text"], g["quad"]) for g in U.parse_ocr_regions(row, proc, (R, R))]
        else:
            got = [(region_text(row, rec[r, k], table, texts), [int(v) - (oy if q & 1 else ox) for q, v in enumerate(rec[r, k, 3:11])])
                   for k in range(found)]
        assert got == want, (name, got, want)
        assert ("hard" in name) == bool(flags & 1), name
    return names, seen


def check_expected_counts(L, dev, tmp_dir, sync=lambda: None):
    """the rows of the issue's list give what it says they give (one launch, T = 65, every case once)"""
    proc, _ = oracle(tmp_dir)
    table, texts = proc.loc_class_table()
    T, R = 65, 64
    cases = gen_cases(T)
    names = list(cases)
    ids = np.full((len(names), T), PAD, np.int32)
    for r, name in enumerate(names):
        g, eos = cases[name]
        row = [START] + g + ([EOS] if eos else [])
        ids[r, :len(row)] = row
    cells = [[0, 0, -2 ** 31, INF, -2 ** 31, INF]] * len(names)
    rec, _sums, rows = launch_parse(L, dev, sync, ids, table, None, cells, T, R)
    got = {name: (int(rows[r, 0]), int(rows[r, 2])) for r, name in enumerate(names)}
    want = {"no_region": (0, 0), "eight_locs_no_content": (0, 0), "one_token_and_quad_whole_row": (1, 0), "nine_locs": (1, 0),
            "whitespace_content": (1, 0), "hard_lt": (0, 1), "sixteen_locs": (1, 0), "strips_inside": (1, 0), "id_beyond_table": (1, 1),
            "truncated_region_at_the_end": (1, 2), "seventeen_locs": (1, 0), "two_regions_back_to_back": (2, 0), "hard_newline": (2, 1),
            "hard_lt_in_content": (2, 1), "no_eos_no_region": (0, 2)}
    assert got == want, got
    r = names.index("nine_locs")                            # the stray location token is the content
    assert rec[r, 0, 1:3].tolist() == [2, 3] and rec[r, 0, 11] == 9 and region_text(ids[r].tolist(), rec[r, 0], table, texts) == "<loc_7>"
    r = names.index("strips_inside")                        # content A <pad> B: columns 2..4, 2 + 8 tokens counted
    assert rec[r, 0, 1:3].tolist() == [2, 5] and rec[r, 0, 11] == 10
    r = names.index("whitespace_content")
    assert region_text(ids[r].tolist(), rec[r, 0], table, texts) == "" and rec[r, 0, 12] == 1
    assert not np.any(_sums)                                # no log-probabilities given


def check_ownership(L, dev, tmp_dir, sync=lambda: None):
    """a 3 x 2 grid of 64 x 64 tiles over 150 x 100 pixels (origins x 0, 43, 86 and y 0, 36): the x boundaries, doubled, are
    0 + 43 + 64 = 107 and 43 + 86 + 64 = 193, the y boundary 0 + 36 + 64 = 100.  Every tile reads the same three regions; their
    doubled centres in frame pixels decide.  A centre exactly ON a boundary belongs to the cell that starts there."""
    from omniparser_amd.pipeline import ScreenParser
    proc, _ = oracle(tmp_dir)
    table, _texts = proc.loc_class_table()
    R, T = 64, 65
    origins = ScreenParser.tile_origins(150, 100, R, R, 16)[0]
    assert origins == [(0, 0), (43, 0), (86, 0), (0, 36), (43, 36), (86, 36)]
    cells = grid_cells(origins, R)
    assert cells[0] == [0, 0, -2 ** 31, 107, -2 ** 31, 100] and cells[4] == [43, 36, 107, 193, 100, INF] and cells[2][2:4] == [193, INF]

    def quad_bins(x0, y0, x1, y1):        # bins whose de-quantised corners are exactly these tile pixels at R = 64
        def b(v):
            k = next(k for k in range(1000) if ((2 * k + 1) * R) // 2000 == v)
            return k
        return loc(b(x0), b(y0), b(x1), b(y0), b(x1), b(y1), b(x0), b(y1))
    # tile pixels (x0, y0, x1, y1): centre doubled = x0 + x1 (+ 2 origin).  In tile 1 (origin 43): 10 + 11 + 86 = 107, ON the boundary
    regs = [quad_bins(10, 5, 11, 9), quad_bins(10, 5, 10, 9), quad_bins(40, 30, 50, 34)]
    row = [START, BOS] + [A] + regs[0] + [B] + regs[1] + [C] + regs[2] + [EOS]
    ids = np.full((len(origins), T), PAD, np.int32)
    ids[:, :len(row)] = row
    rec, _sums, rows = launch_parse(L, dev, sync, ids, table, None, cells, T, R)
    t_rec, _t, t_rows = twin_parse(ids, table, None, cells, T, R)
    assert np.array_equal(rec, t_rec) and np.array_equal(rows, t_rows)
    kept = [[int(rec[r, k, 12]) for k in range(3)] for r in range(len(origins))]
    # tile 0: centres 21, 20 < 107 and 2 * 7 = 14 < 100: kept; 90 < 107 and 64 < 100: kept
    # tile 1: 107 == boundary: belongs to tile 1's cell (kept); 106 < 107: tile 0's (dropped); 90 + 86 = 176 in [107, 193): kept
    # tile 2 (origin 86): 193 == boundary of cell 2: kept; 192: dropped; 262: kept
    # tiles 3..5 (origin y 36): y centres 14 + 72 = 86 < 100: dropped; 64 + 72 = 136 >= 100: by x as above
    assert kept == [[1, 1, 1], [1, 0, 1], [1, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, 1]], kept
    assert rows[:, 0].tolist() == [3] * 6 and rows[:, 1].tolist() == [3, 2, 2, 1, 1, 1]
    # the y boundary exactly: a box whose doubled y centre is 100 in frame pixels — tile 0: 50 + 50; tile 3: 14 + 14 + 72
    row0 = [START, BOS, A] + quad_bins(5, 50, 9, 50) + [EOS]
    row3 = [START, BOS, A] + quad_bins(5, 14, 9, 14) + [EOS]
    ids2 = np.full((2, T), PAD, np.int32)
    ids2[0, :len(row0)], ids2[1, :len(row3)] = row0, row3
    rec2, _s, _r = launch_parse(L, dev, sync, ids2, table, None, [cells[0], cells[3]], T, R)
    assert rec2[0, 0, 4] + rec2[0, 0, 8] == 100 == rec2[1, 0, 4] + rec2[1, 0, 8] and [int(rec2[0, 0, 12]), int(rec2[1, 0, 12])] == [0, 1]


def check_parse_errors(L, dev, tmp_dir, sync=lambda: None):
    """M != (T - 1) // 9, T < 2, NULL ids / class table / records, table_len < 1, a stride below T: OMNI_E_ARG, outputs untouched"""
    from omniparser_amd.florence import region_parse_op
    proc, _ = oracle(tmp_dir)
    table, _ = proc.loc_class_table()
    T, n, R = 19, 3, 64
    M = (T - 1) // 9
    ids, logp, _ = parse_rows(T, n)
    d = {"ids": torch.from_numpy(ids).to(dev), "table": torch.from_numpy(table.astype(np.int16)).to(dev), "logp": torch.from_numpy(logp).to(dev),
         "cells": torch.tensor([[0, 0, -2 ** 31, INF, -2 ** 31, INF]] * n, dtype=torch.int32).to(dev),
         "rec": torch.full((n * M * 16,), -7, dtype=torch.int32).to(dev), "sums": torch.full((n * M,), -7.0).to(dev),
         "rows": torch.full((n * 4,), -7, dtype=torch.int32).to(dev)}
    sync()
    p = {k: t.data_ptr() for k, t in d.items()}
    seen = []
    for what, kw in (("M too large", dict(slots=M + 1)), ("M too small", dict(slots=M - 1)), ("T = 1", dict(T=1, slots=0)), ("T = 0", dict(T=0, slots=0)),
                     ("T beyond the limit", dict(T=2050, slots=227)), ("null ids", dict(ids=None)), ("null table", dict(table=None)),
                     ("null records", dict(rec=None)), ("null cells", dict(cells=None)), ("table_len = 0", dict(table_len=0)),
                     ("ids stride below T", dict(ld_ids=T - 1)), ("logp stride below T - 1", dict(ld_logp=T - 2)), ("n = 0", dict(n=0)),
                     ("R = 0", dict(R=0)), ("mode 2", dict(mode=2))):
        a = dict(p, n=n, T=T, table_len=len(table), R=R, ld_ids=0, ld_logp=0, slots=None, mode=1)
        a.update(kw)
        op = region_parse_op(a["ids"], a["table"], a["logp"], a["cells"], a["rec"], a["sums"], a["rows"], a["n"], a["T"], a["table_len"], a["R"],
                             EOS, ld_ids=a["ld_ids"], ld_logp=a["ld_logp"], slots=a["slots"])
        op.i[0] = a["mode"]
        rc = L.lib().omni_op_launch(ctypes.byref(op), L._stream_ptr(None))
        assert rc == E_ARG, (what, rc)
        seen.append((what, L.lib().omni_last_error().decode()))
    sync()
    assert all(bool((d[k].cpu() == -7).all()) for k in ("rec", "sums", "rows"))
    L.launch(region_parse_op(p["ids"], p["table"], p["logp"], p["cells"], p["rec"], p["sums"], p["rows"], n, T, len(table), R, EOS))
    sync()
    t_rec, t_sums, t_rows = twin_parse(ids, table, logp, d["cells"].cpu().tolist(), T, R)
    assert np.array_equal(d["rec"].cpu().numpy().reshape(n, M, 16), t_rec) and np.array_equal(d["rows"].cpu().numpy().reshape(n, 4), t_rows)
    assert np.array_equal(d["sums"].cpu().numpy().reshape(n, M).view(np.int32), t_sums.view(np.int32))
    return seen


# ---------------------------------------------------------------------------------------------- mode 0
CUT_FRAMES = {"six_tiles": (150, 100, 16), "one_tile": (64, 64, 16), "narrower_than_a_tile": (40, 150, 16)}     # W, H, overlap


def frame(W, H, seed=0):
    return np.random.default_rng(seed + 31 * W + H).integers(0, 256, (H, W, 3), dtype=np.uint8)


def host_tiles(img, origins, R):
    """FlorenceProcessor(images=tile, do_resize=False) on the Pillow crop of every window, pasted on a white R x R canvas: f32
    [n, 3, R, R]"""
    from PIL import Image
    from omniparser_amd.util import utils as U
    proc = U.FlorenceProcessor(None)
    pil = Image.fromarray(img)
    H, W = img.shape[:2]
    tiles = []
    for x, y in origins:
        canvas = Image.new("RGB", (R, R), (255, 255, 255))
        canvas.paste(pil.crop((x, y, min(x + R, W), min(y + R, H))), (0, 0))
        tiles.append(canvas)
    return proc(images=tiles, do_resize=False)["pixel_values"]


def launch_cut(L, dev, sync, img, origins, R, f16, ldo, what="tile cut"):
    from omniparser_amd.florence import tile_cut_op
    n = len(origins)
    H, W = img.shape[:2]
    dt = torch.float16 if f16 else torch.float32
    ar = CF.Arena()
    ar.add("img", torch.uint8, 1, H * W * 3, data=((0, torch.from_numpy(img).reshape(1, -1)),))
    ar.add("origins", torch.int32, n, 2, data=((0, torch.tensor(origins, dtype=torch.int32)),))
    ar.add("lut", torch.float32, 1, 256, data=((0, torch.from_numpy((np.arange(256).astype(np.float64) * (1 / 255)).astype(np.float32))[None]),))
    ar.add("y", dt, n * R * R, ldo, out=((0, ldo),))
    ar.build(dev)
    L.launch(tile_cut_op(L.F16 if f16 else L.F32, ar.ptr("img"), ar.ptr("origins"), ar.ptr("y"), ar.ptr("lut"), n, H, W, R, ldo))
    sync()
    ar.fetch(what)
    return ar.get("y", 0, ldo).view(n, R, R, ldo)


def check_cut(L, dev, name, f16, R=64, sync=lambda: None):
    from omniparser_amd.pipeline import ScreenParser
    W, H, overlap = CUT_FRAMES[name]
    img = frame(W, H)
    origins = ScreenParser.tile_origins(W, H, R, R, overlap)[0]
    if name == "six_tiles":
        assert len(origins) == 6 and origins[-1] == (W - R, H - R) and (W * 3) % 4 != 0       # the last tile ends at the frame's last pixel
    if name == "one_tile":
        assert origins == [(0, 0)]
    if name == "narrower_than_a_tile":
        assert len(origins) == 3 and W < R
    ldo = 8 if f16 else 4
    y = launch_cut(L, dev, sync, img, origins, R, f16, ldo)
    ref = host_tiles(img, origins, R).permute(0, 2, 3, 1).contiguous()
    if f16:
        ref = ref.to(torch.float16)
    bits = torch.int16 if f16 else torch.int32
    assert torch.equal(y[..., :3].contiguous().view(bits), ref.view(bits)), name
    assert not bool(y[..., 3:].any()), "padding channels are not zero"
    return len(origins)


def check_cut_errors(L, dev, sync=lambda: None):
    from omniparser_amd.florence import tile_cut_op
    img = torch.from_numpy(frame(20, 10)).to(dev)
    org = torch.zeros((2, 2), dtype=torch.int32).to(dev)
    lut = torch.zeros(256).to(dev)
    y = torch.full((2 * 8 * 8 * 4,), -7.0).to(dev)
    sync()
    good = dict(img=img.data_ptr(), org=org.data_ptr(), y=y.data_ptr(), lut=lut.data_ptr(), n=2, H=10, W=20, R=8, ldo=4)
    seen = []
    for what, kw in (("n = 0", dict(n=0)), ("R = 0", dict(R=0)), ("H = 0", dict(H=0)), ("pitch 2", dict(ldo=2)), ("null frame", dict(img=None)),
                     ("null origins", dict(org=None)), ("null output", dict(y=None)), ("null table", dict(lut=None))):
        a = dict(good)
        a.update(kw)
        op = tile_cut_op(L.F32, a["img"], a["org"], a["y"], a["lut"], a["n"], a["H"], a["W"], a["R"], a["ldo"])
        rc = L.lib().omni_op_launch(ctypes.byref(op), L._stream_ptr(None))
        assert rc == E_ARG, (what, rc)
        seen.append((what, L.lib().omni_last_error().decode()))
    sync()
    assert bool((y.cpu() == -7.0).all())
    return seen


# ---------------------------------------------------------------------------------------------- captioner against transformers
OCR_FRAME = (150, 100, 16)             # W, H, overlap: 6 tiles at R = 64
OCR_MAX_NEW = 64
OCR_TEXT_IDS = tuple(range(36, 76))    # the text tokens generation may pick besides the 1000 location tokens ('A' .. and 14 merges)
OCR_SEED = 0                           # see `ocr_reference` for what the oracle gives at it
TOL_LOGP = 1.38e-4                     # profiles/long_decode_tolerance.json: per token, hence for a mean over tokens


def ocr_suppress(vocab, keep=()):
    """suppress_tokens that leave only the location ids, OCR_TEXT_IDS and `keep` (bos, eos, forced tokens: they cannot be suppressed)"""
    allowed = set(range(LOC0, LOC0 + 1000)) | set(OCR_TEXT_IDS) | {int(k) for k in keep}
    return [t for t in range(vocab) if t not in allowed]


def ocr_reference(tmp_dir, eos_prone, seed=OCR_SEED, R=64, frame_whl=OCR_FRAME, max_new=OCR_MAX_NEW, restrict=True):
    """transformers on the CPU for the tiles of the seeded frame: (frame u8, origins, pixel_values of the host-cut tiles, prompt row,
    suppress list or None, sequences, margins, per-token log-probabilities [n, T - 1], per tile the post-processor's [(text, quad)])

    What THE ORACLE ALONE gives at OCR_SEED = 0 with OCR_TEXT_IDS = 36..75 (transformers on the CPU, chosen and recorded before any
    device run; `check_read_regions` asserts it again):
      stock checkpoint     6 regions in each of the 6 tiles, 35 of the 36 with a stray location token in their content (the allowed
                           set is 96 % location tokens), every row 64 tokens long, smallest top-1 / top-2 margin 3.4e-4
      EOS-prone checkpoint the EOS token (13840) beats every allowed token at the first free step in every tile: 6 tiles, no region,
                           3 columns per row — the early exit after the first poll
    One run with regions in some tiles AND a tile without any was not found: the stand-in's answer barely depends on the pixels
    (seeds 0..39 x eight windows of 40 text ids with the EOS-prone checkpoint, seeds 0..5 with the stock one, min_new_tokens 10..30:
    every tile of a frame ends at the same length), so the two halves of that condition are asserted on the two checkpoints."""
    import beam_checks as BC
    import prompt_checks as P
    from omniparser_amd.pipeline import ScreenParser
    proc, post = oracle(tmp_dir)
    W, H, overlap = frame_whl
    img = frame(W, H, seed)
    origins = ScreenParser.tile_origins(W, H, R, R, overlap)[0]
    pix = host_tiles(img, origins, R)
    row = proc.prompt_ids("<OCR_WITH_REGION>")
    model = BC.oracle_model(0, eos_prone)
    try:
        eos = model.generation_config.eos_token_id
        suppress = ocr_suppress(model.config.get_text_config().vocab_size, keep=(BOS, EOS, eos)) if restrict else None
        kw = {"suppress_tokens": suppress} if restrict else {}
        ids, mask = P.hf_inputs(model, R, [row] * len(origins))
        with torch.inference_mode():
            out = model.generate(input_ids=ids, attention_mask=mask, pixel_values=pix, max_new_tokens=max_new, num_beams=1, do_sample=False,
                                 output_scores=True, return_dict_in_generate=True, **kw)
            ts = model.compute_transition_scores(out.sequences, out.scores, normalize_logits=True)
        seq = out.sequences
        margins = [float("inf")] * seq.shape[0]
        for t, sc in enumerate(out.scores):
            if t == 0 or t == max_new - 1:
                continue
            top2 = sc.float().topk(2, dim=1).values
            for b in range(seq.shape[0]):
                if not (seq[b, 1:t + 1] == eos).any():
                    margins[b] = min(margins[b], float(top2[b, 0] - top2[b, 1]))
    finally:
        model.generation_config.eos_token_id = 2
    regions = []
    for b in range(seq.shape[0]):
        r = seq[b].tolist()
        end = next((j for j in range(1, len(r)) if r[j] == eos), len(r))
        known = [t for t in r[1:end] if 0 <= t < 1400]          # (an id the synthetic tokenizer does not know cannot be rendered)
        text, _ = post.decode_with_spans(known)
        regions.append([(g["text"], [int(v) for v in g["quad_box"]]) for g in post.parse_ocr_from_text_and_spans(text, None, (R, R))]
                       if len(known) == end - 1 else None)
    return dict(img=img, origins=origins, pix=pix, row=row, suppress=suppress, seq=seq, margins=margins, logp=ts.float(), regions=regions, eos=eos)


def record_columns(row, rec, table):
    """the columns a device record counts: the non-STRIP tokens of its content and its eight location tokens"""
    cols = [j for j in range(int(rec[1]), int(rec[2])) if table[row[j]] != STRIP]
    j, locs = int(rec[2]), 0
    while locs < 8:
        if table[row[j]] != STRIP:
            cols.append(j)
            locs += 1
        j += 1
    assert len(cols) == int(rec[11])
    return cols


def caption_dir_with_tokenizer(tmp_dir, eos_prone=False):
    """the stand-in caption checkpoint (or its EOS-prone twin) with the location-token tokenizer next to it"""
    import beam_checks as BC
    from tools.make_weights import ensure_caption_checkpoint
    src = BC.eos_prone_checkpoint(0) if eos_prone else ensure_caption_checkpoint(0)
    dst = Path(tmp_dir) / ("ckpt_eos" if eos_prone else "ckpt")
    if not (dst / "tokenizer.json").exists():
        dst.mkdir(parents=True, exist_ok=True)
        for f in ("model.safetensors", "config.json", "generation_config.json"):
            (dst / f).symlink_to((src / f).resolve())
        shutil.copy(write_tokenizer(Path(tmp_dir) / "tok_for_ckpt") / "tokenizer.json", dst / "tokenizer.json")
    return dst


def check_read_regions(tmp_dir, eos_prone, log=None):
    """Florence2Captioner.read_regions at R = 64 on the 150 x 100 frame, 64 new tokens, generation restricted to the location tokens
    and OCR_TEXT_IDS: ids = generate() on the host-cut tiles row for row, token-exact against transformers on the CPU (margins
    asserted first), regions = the post-processor on transformers' sequences, mean log-probabilities within TOL_LOGP"""
    import prompt_checks as P
    from omniparser_amd.florence import Florence2Captioner
    from omniparser_amd.util import utils as U
    ref = ocr_reference(tmp_dir, eos_prone)
    W, H, overlap = OCR_FRAME
    R, n = 64, len(ref["origins"])
    per = [len(r) for r in ref["regions"]]
    if eos_prone:                                           # the EOS token beats every allowed token at once: no tile has a region
        assert per == [0] * n, per
    else:
        stray = sum(1 for r in ref["regions"] for text, _ in r if "<loc_" in text)
        assert sum(per) >= 4 and sum(1 for p in per if p) >= 2 and stray >= 1, (per, stray)
    finite = [m for m in ref["margins"] if m != float("inf")]
    if finite:
        P.assert_margins(finite, f"region ocr eos_prone={eos_prone}")
    ckpt = caption_dir_with_tokenizer(tmp_dir, eos_prone)
    cap = Florence2Captioner(ckpt, "cuda", precision="f32", resolution=R)
    proc = U.FlorenceProcessor(ckpt, image_token_id=cap.w.cfg.get("image_token_id", 51289), special_ids=(cap.w.bos, cap.w.pad, cap.w.eos, 3))
    table, texts = proc.loc_class_table()
    gen = {"suppress_tokens": ref["suppress"]}
    out = cap.read_regions(torch.from_numpy(ref["img"]).cuda(), max_new_tokens=OCR_MAX_NEW, overlap=overlap, prompt_ids=ref["row"],
                           class_table=table, controls=gen)
    assert out.origins == ref["origins"] and tuple(out.ids.shape) == (n, OCR_MAX_NEW + 1)
    n_img = (R // 32) ** 2 + 1
    inp = torch.tensor([[proc.image_token_id] * n_img + ref["row"]] * n)
    g = cap.generate(input_ids=inp, pixel_values=ref["pix"], max_new_tokens=OCR_MAX_NEW, output_scores=True, return_dict_in_generate=True, **gen)
    worst = 0.0
    for b in range(n):
        mine = P._trim(out.ids[b])
        assert mine == P._trim(g.sequences[b]), (b, mine, g.sequences[b].tolist())
        assert mine == P._trim(ref["seq"][b]), (b, mine, ref["seq"][b].tolist())
        row = out.ids[b].tolist()
        found, _kept, flags = (int(v) for v in out.rows[b, :3])
        assert flags == 0 or (flags == 2 and ref["eos"] not in row[1:]), (b, flags)
        ox, oy = out.origins[b]
        got = [(region_text(row, out.records[b, k], table, texts), [int(v) - (oy if q & 1 else ox) for q, v in enumerate(out.records[b, k, 3:11])])
               for k in range(found)]
        assert got == ref["regions"][b], (b, got, ref["regions"][b])
        for k in range(found):
            cols = record_columns(row, out.records[b, k], table)
            want = float(sum(float(ref["logp"][b, j - 1]) for j in cols)) / len(cols)
            have = float(out.sums[b, k]) / int(out.records[b, k, 11])
            worst = max(worst, abs(want - have))
    line = f"read_regions eos_prone={eos_prone}: regions per tile {per}, steps {cap.last_steps}, max |d mean logp| = {worst:.3e} (bound {TOL_LOGP:.2e})"
    print(line)
    if log is not None:
        log.append(line)
    assert worst <= TOL_LOGP, worst
    return cap, proc, ref, out


def check_read_regions_768():
    """R = 768, a 900 x 800 frame (4 tiles at overlap 128), 16 new tokens, no tokenizer-dependent part: the plan's input after the tile
    cut is bit-equal to the processor on the Pillow crops, and the ids equal generate() on those"""
    from omniparser_amd.florence import Florence2Captioner, PROMPT_IDS
    from omniparser_amd.pipeline import ScreenParser
    from tools.make_weights import ensure_caption_checkpoint
    R, max_new = 768, 16
    img = frame(900, 800)
    origins = ScreenParser.tile_origins(900, 800, R, R, 128)[0]
    assert origins == [(0, 0), (132, 0), (0, 32), (132, 32)]
    pix = host_tiles(img, origins, R)
    cap = Florence2Captioner(ensure_caption_checkpoint(0), "cuda", precision="f32", resolution=R)
    table = np.full((1400,), TEXT, np.uint16)
    out = cap.read_regions(torch.from_numpy(img).cuda(), max_new_tokens=max_new, overlap=128, prompt_ids=list(PROMPT_IDS), class_table=table)
    cp = cap.plans(cap.bucket(4), R, max_new, scores=True)      # the default prompt's plan: what read_regions just ran on
    x = cp.x_in.t[:4, :, :, :3].float().cpu()
    assert torch.equal(x.view(torch.int32), pix.permute(0, 2, 3, 1).contiguous().view(torch.int32)), "the plan's input is not the processor's"
    g = cap.generate(pixel_values=pix, max_new_tokens=max_new, output_scores=True, return_dict_in_generate=True)
    import prompt_checks as P
    for b in range(4):
        assert P._trim(out.ids[b]) == P._trim(g.sequences[b]), b
    return out


# ---------------------------------------------------------------------------------------------- the host surface
class StandInReader:
    """A stand-in for Florence2Captioner on the host emulation: `read_regions` with the captioner's argument checks, tile grid and
    both modes of the real op (launched on the emulated device), but the DECODE between them is a lookup — tile k answers with a
    canned row chosen by k (an emulated encode + 64-step decode per tile takes minutes).  The real captioner: the MI355X twin."""

    def __init__(self, L, R=64, eos=EOS):
        from types import SimpleNamespace
        self.L, self.resolution, self.device = L, R, torch.device("cpu")
        self.w = SimpleNamespace(eos=eos, pad=PAD)
        self.calls = []

    def canned(self, k, T):
        rows = [[BOS, A, B] + QUAD_A + [C] + QUAD_B,        # two regions
                [BOS, SP] + QUAD_B,                         # whitespace only: dropped by read_text_regions
                [BOS, A, TOK_NL, B] + QUAD_A,               # a newline: re-parsed on the host
                [BOS, C, C] + loc(100, 100, 900, 100, 900, 900, 100, 900),
                [BOS, A, B, C]]                             # nothing
        g = rows[k % len(rows)]
        return ([START] + g + [EOS] + [PAD] * T)[:T]

    def read_regions(self, image_u8, max_new_tokens=1024, overlap=128, prompt_ids=None, class_table=None, controls=None):
        from types import SimpleNamespace
        from omniparser_amd import florence as FL
        from omniparser_amd.pipeline import ScreenParser
        R = self.resolution
        if prompt_ids is None or class_table is None:
            raise ValueError("read_regions needs prompt_ids and class_table")
        table = FL.check_class_table(class_table)
        if isinstance(overlap, bool) or not isinstance(overlap, int) or not 0 <= overlap < R:
            raise ValueError(f"overlap must be an integer in 0..{R - 1}")
        if isinstance(max_new_tokens, bool) or not isinstance(max_new_tokens, int) or not 1 <= max_new_tokens <= 1024:
            raise ValueError("max_new_tokens must be an integer in 1..1024")
        self.calls.append(dict(max_new_tokens=max_new_tokens, overlap=overlap, controls=controls))
        H, W = image_u8.shape[:2]
        origins = ScreenParser.tile_origins(W, H, R, R, overlap)[0]
        n, T = len(origins), max_new_tokens + 1
        M = FL.ocr_slots(T)
        org = torch.tensor(origins, dtype=torch.int32)
        lut = torch.from_numpy((np.arange(256).astype(np.float64) * (1 / 255)).astype(np.float32))
        x = torch.empty((n, R, R, 4), dtype=torch.float32)
        img = image_u8.contiguous()
        self.L.launch(FL.tile_cut_op(self.L.F32, img.data_ptr(), org.data_ptr(), x.data_ptr(), lut.data_ptr(), n, H, W, R, 4))
        self.tiles = x
        ids = torch.tensor([self.canned(k, T) for k in range(n)], dtype=torch.int32)
        logp = -torch.rand((n, T), generator=torch.Generator().manual_seed(n))
        cells = torch.tensor(FL.ocr_cells(origins, R), dtype=torch.int32)
        rec, sums, rows = torch.zeros((n, max(M, 1), 16), dtype=torch.int32), torch.zeros((n, max(M, 1))), torch.zeros((n, 4), dtype=torch.int32)
        self.L.launch(FL.region_parse_op(ids.data_ptr(), table.data_ptr(), logp.data_ptr() + 4, cells.data_ptr(), rec.data_ptr(), sums.data_ptr(),
                                         rows.data_ptr(), n, T, table.numel(), R, self.w.eos, ld_ids=T, ld_logp=T))
        return SimpleNamespace(origins=origins, records=rec[:, :M], sums=sums[:, :M], rows=rows, ids=ids.long(), logp=logp[:, 1:])


def check_read_text_regions(cmp_, img, kw, expect_some=True):
    """read_text_regions against the reader's own raw output: tile-major order, only kept regions with text, confidence =
    exp(sum / count), quads and boxes in frame pixels; FlorenceOCR.readtext behind set_ocr_engine / check_ocr_box gives the same
    boxes after get_xywh / get_xyxy; FlorenceOCR(image) is the ocr_provider contract"""
    import math
    from PIL import Image
    from omniparser_amd.util import utils as U
    model, proc = cmp_["model"], cmp_["processor"]
    table, texts = proc.loc_class_table()
    regions, stats = U.read_text_regions(img, cmp_, return_stats=True, **kw)
    assert regions == U.read_text_regions(Image.fromarray(img), cmp_, **kw)
    raw = model.read_regions(torch.from_numpy(img).to(model.device), max_new_tokens=kw.get("max_new_tokens", 1024), overlap=kw.get("overlap", 128),
                             prompt_ids=proc.prompt_ids("<OCR_WITH_REGION>"), class_table=table, controls=kw.get("generation"))
    assert len(stats) == len(raw.origins) and [s["fallback"] for s in stats] == [bool(int(f) & 1) for f in raw.rows[:, 2]]
    assert [s["truncated"] for s in stats] == [bool(int(f) & 2) for f in raw.rows[:, 2]]
    want = []
    for r in range(len(raw.origins)):
        if int(raw.rows[r, 2]) & 1:
            continue
        assert stats[r]["found"] == int(raw.rows[r, 0]) and stats[r]["kept"] == int(raw.rows[r, 1])
        row = raw.ids[r].tolist()
        for k in range(int(raw.rows[r, 0])):
            rec = raw.records[r, k].tolist()
            text = region_text(row, rec, table, texts)
            if rec[12] and text:
                want.append((r, text, rec[3:11], math.exp(float(raw.sums[r, k]) / rec[11])))
    got = [(g["tile"], g["text"], [v for xy in g["quad"] for v in xy], g["confidence"]) for g in regions if not stats[g["tile"]]["fallback"]]
    assert got == want, (got, want)
    assert [g["tile"] for g in regions] == sorted(g["tile"] for g in regions)
    for g in regions:
        xs, ys = [p[0] for p in g["quad"]], [p[1] for p in g["quad"]]
        assert g["bbox"] == [min(xs), min(ys), max(xs), max(ys)] and 0.0 < g["confidence"] <= 1.0 and g["text"] == g["text"].strip() != ""
    if expect_some:
        assert regions
    strict = U.read_text_regions(img, cmp_, min_confidence=0.999999, **kw)
    assert all(g["confidence"] >= 0.999999 for g in strict) and len(strict) <= len(regions)
    # behind the existing OCR front-end
    ocr = U.FlorenceOCR(cmp_, **kw)
    saved = dict(U._OCR_ENGINES)
    try:
        U.set_ocr_engine(easyocr_reader=ocr)
        (t1, b1), _ = U.check_ocr_box(Image.fromarray(img), display_img=False, output_bb_format="xyxy", easyocr_args={"text_threshold": 0.8, "paragraph": False})
        (t2, b2), _ = U.check_ocr_box(Image.fromarray(img), display_img=False, output_bb_format="xywh")
    finally:
        U._OCR_ENGINES.update(saved)
    assert t1 == t2 == [g["text"] for g in regions]
    assert b1 == [U.get_xyxy(g["quad"]) for g in regions] and b2 == [U.get_xywh(g["quad"]) for g in regions]
    tx, bx = ocr(Image.fromarray(img))
    assert tx == t1 and bx == [g["bbox"] for g in regions]
    assert [(q, t, c) for q, t, c in ocr.readtext(img, text_threshold=0.9)] == [(g["quad"], g["text"], g["confidence"]) for g in regions]
    return regions, stats

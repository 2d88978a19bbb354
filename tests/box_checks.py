"""Checks shared by the CPU (emulation) and GPU tests of OMNI_OP_REGION_OCR mode 3 (box answers) and of the calls around it
(Florence2Captioner.locate_regions / decode_tiles, util.utils.locate / ground_elements / describe_regions / parse_box_answer,
FlorenceProcessor.task_prompt_ids / quantize_box).  Tokenizer, class table, frames and the transformers oracle: tests/region_checks.py.

Everything here is exact; there is no tolerance but one:
  mode 3   records, row counters and both log-probability sums bit-equal to `twin_boxes`, a literal restatement of the op's semantics
           (include/omni_amd.h) that shares no code with the kernel; for rows without a HARD token, labels and boxes equal to
           transformers' Florence2PostProcessor — parse_description_with_bboxes_from_text_and_spans and
           parse_phrase_grounding_from_text_and_spans for grammar 0, the former with allow_empty_phrase for grammar 1; for rows with
           one, util.utils.parse_box_answer equals those.
  confidence (GPU, captioner) the mean log-probability per box (phrase tokens + four location tokens) within the project's per-token
           tolerance of 1.38e-4 (profiles/long_decode_tolerance.json) of transformers' compute_transition_scores over the same tokens."""
import ctypes
import itertools

import numpy as np
import torch

import caption_f64 as CF
import region_checks as RC
from region_checks import A, B, BOS, C, E_ARG, EOS, HARD, INF, LOC0, PAD, SP, START, STRIP, TEXT, TOK_LT, TOK_NL, loc

BOX_A, BOX_B, BOX_C = loc(10, 20, 500, 300), loc(0, 999, 999, 0), loc(1, 2, 3, 4)
OVD, CPG = "<OPEN_VOCABULARY_DETECTION>", "<CAPTION_TO_PHRASE_GROUNDING>"


# ---------------------------------------------------------------------------------------------- the literal twin
def twin_boxes(ids, table, logp, cells, T, R, grammar, eos=EOS):
    """OMNI_OP_REGION_OCR mode 3 as include/omni_amd.h words it, on the host: ids [n, >= T] ints, table u16 numpy, logp f32 numpy
    [n, >= T - 1] or None, cells [n][6] -> (records i32 [n, M, 16], sums f32 [n, M, 2], rows i32 [n, 4])"""
    n, M = len(ids), (T - 1) // 4
    rec, sums, rows = np.zeros((n, M, 16), np.int32), np.zeros((n, M, 2), np.float32), np.zeros((n, 4), np.int32)

    def total(r, cols):
        t = np.float32(0.0)
        if logp is not None:
            for j in cols:
                t = np.float32(t + np.float32(logp[r][j - 1]))
        return t
    for r in range(n):
        row = [int(t) for t in ids[r][:T]]
        end = next((j for j in range(1, T) if row[j] == eos), T)
        cls = [min(int(table[t]), HARD) if 0 <= t < len(table) else HARD for t in row[:end]]
        cols = [j for j in range(1, end) if cls[j] != STRIP]           # original columns of the non-STRIP tokens
        runs = [(is_loc, [c for c in grp]) for is_loc, grp in itertools.groupby(cols, key=lambda j: cls[j] < 1000)]
        carry, text, found = None, [], []                               # found: (phrase columns, lead, the four columns of a box)
        phrases = 0
        for is_loc, run in runs:
            if not is_loc:
                text = run
                continue
            if grammar == 1:
                phrase, lead, locs = ([], 0, run) if len(run) >= 4 else (None, 0, [])
            else:
                start = carry if carry is not None else (text[0] if text else None)
                if start is not None and len(run) >= 4:
                    phrase, lead, locs, carry = [j for j in cols if start <= j < run[0]], int(carry is not None), run, None
                elif start is None and len(run) >= 5:
                    phrase, lead, locs, carry = run[:1], 1, run[1:], None
                else:
                    phrase, carry = None, run[-1]
            text = []
            if phrase is None:
                continue
            for q in range(len(locs) // 4):
                found.append((phrase, lead, locs[4 * q:4 * q + 4], phrases))
            phrases += 1
        kept = 0
        c = cells[r]
        for k, (phrase, lead, four, ordinal) in enumerate(found):
            x0, y0, x1, y1 = (((2 * cls[j] + 1) * R) // 2000 + c[q & 1] for q, j in enumerate(four))
            cx, cy = x0 + x1, y0 + y1
            own = c[2] <= cx and (c[3] == INF or cx < c[3]) and c[4] <= cy and (c[5] == INF or cy < c[5])
            c0, c1 = (phrase[0], phrase[-1] + 1) if phrase else (four[0], four[0])
            rec[r, k, :12] = [r, c0, c1, x0, y0, x1, y1, four[0], len(phrase), int(own), ordinal, lead]
            sums[r, k] = [total(r, phrase), total(r, four)]
            kept += int(own)
        rows[r] = [len(found), kept, int(any(v == HARD for v in cls[1:])) | (2 if end == T else 0), phrases]
    return rec, sums, rows


def box_label(row, rec, table, texts):
    """the label of a device record: the rendered non-STRIP tokens of its phrase columns (`lead`: the first without its first
    character), stripped, non-ASCII characters dropped"""
    toks = [texts[t] for t in row[rec[1]:rec[2]] if table[t] != STRIP]
    if rec[11] and toks:
        toks[0] = toks[0][1:]
    return "".join(toks).strip().encode("ascii", "ignore").decode("ascii")


def oracle_boxes(post, row, size, which, eos=EOS):
    """transformers on one row (start token, generated ids ...; cut in front of the first EOS): [(label, [x0, y0, x1, y1])] of
    `which` = "description" (parse_description_with_bboxes_from_text_and_spans), "bboxes" (the same, allow_empty_phrase) or
    "grounding" (parse_phrase_grounding_from_text_and_spans, one entry per box of an instance)"""
    end = next((j for j in range(1, len(row)) if row[j] == eos), len(row))
    text, _ = post.decode_with_spans([int(t) for t in row[1:end]])
    if which == "grounding":
        return [(g["cat_name"], [int(v) for v in b]) for g in post.parse_phrase_grounding_from_text_and_spans(text, (size, size)) for b in g["bbox"]]
    got = post.parse_description_with_bboxes_from_text_and_spans(text, (size, size), allow_empty_phrase=which == "bboxes")
    return [(g["cat_name"], [int(v) for v in g["bbox"]]) for g in got]


ORACLES = {0: ("description", "grounding"), 1: ("bboxes",)}


# ---------------------------------------------------------------------------------------------- rows
def gen_cases(T):
    """{name: (generated tokens without the EOS, has an EOS)} — every case of the issue's list that fits a row of T tokens; a row
    is START + generated + [EOS] + garbage"""
    room = T - 2                          # generated tokens in front of an EOS
    cases = {
        "eos_in_column_1": ([], True),
        "text_only": ([BOS, A, B], True),
        "three_locs_only": ([BOS] + BOX_A[:3], True),
        "text_4_whole_row": ([A] + BOX_A, T != 6),                                    # at T = 6 it IS the row: no EOS fits
        "five_leading_locs": (loc(7) + BOX_A, T != 6),                                # the two grammars give different bins
    }
    if room >= 8:
        cases["text_4"] = ([BOS, A, B] + BOX_A, True)
        cases["text_5"] = ([A] + BOX_A + loc(5), True)
        cases["text_6"] = ([A] + BOX_A + loc(5, 6), True)
        cases["text_7"] = ([A] + BOX_A + loc(5, 6, 7), True)
        cases["hard_lt"] = ([BOS, A, TOK_LT] + BOX_A, True)
        cases["four_locs_only"] = ([BOS] + BOX_B, True)
    if room >= 9:
        cases["text_8_one_phrase_two_boxes"] = ([A] + BOX_A + BOX_B, True)
    if room >= 17:
        cases["nine_leading_locs"] = (loc(7) + BOX_A + BOX_B, True)
        cases["text_3_text_4_lead_phrase"] = ([A] + BOX_A[:3] + [B] + BOX_B, True)
        cases["four_locs_text_4"] = (BOX_A + [B] + BOX_B, True)
        cases["strips_inside"] = ([BOS, A, PAD, B] + BOX_A[:2] + [BOS] + BOX_A[2:] + [PAD] + BOX_B, True)
        cases["id_beyond_table"] = ([BOS, A, 5000] + BOX_A + [-3], True)
        cases["two_phrases_three_boxes"] = ([A, B] + BOX_A + [C] + BOX_B + BOX_C, True)
        cases["whitespace_phrase"] = ([BOS, SP] + BOX_B, True)
        cases["hard_newline"] = ([A, TOK_NL, B] + BOX_A, True)
        cases["carry_twice"] = ([A] + BOX_A[:3] + [B] + BOX_B[:2] + [C] + BOX_C, True)
        cases["no_eos_text"] = ([BOS] + [A, B, C] * ((T - 2) // 3) + [A] * ((T - 2) % 3), False)
        cases["every_slot_in_grammar_1"] = ((BOX_A + BOX_B) * ((T - 1) // 8) + BOX_C[:(T - 1) % 8], False)      # T - 1 location tokens
    for name, (g, eos) in cases.items():
        assert len(g) + (2 if eos else 1) <= T and (eos or len(g) == T - 1), (name, T, len(g))
    return cases


def parse_rows(T, n, seed=0):
    """n rows of T ids (numpy i32) and their log-probabilities f32 [n, T - 1], cycling through `gen_cases` from an offset that
    depends on T; behind a row's EOS: garbage ids (location tokens and EOS among them) and NaN log-probabilities"""
    cases = gen_cases(T)
    names = list(cases)
    rng = np.random.default_rng(4000 * T + n + seed)
    ids = np.zeros((n, T), np.int32)
    logp = np.full((n, T - 1), np.nan, np.float32)
    picked = []
    for r in range(n):
        name = names[(r + T) % len(names)]
        g, eos = cases[name]
        row = [START] + g + ([EOS] if eos else [])
        used = len(row)
        junk = rng.choice(np.array(BOX_A + BOX_B + [EOS, A, 70000, -1, TOK_NL], dtype=np.int64), size=T - used)
        ids[r] = row + junk.tolist()
        logp[r, :used - 1] = -rng.random(used - 1, dtype=np.float32) * 3
        picked.append(name)
    return ids, logp, picked


RANDOM_T = 50                              # rows of 1..48 generated tokens + EOS


def random_rows(n, text_share, seed):
    """the issue's generator: n rows of 1..48 tokens, `text_share` of them text (RC.OCR_TEXT_IDS and the space), 3 % STRIP tokens, the
    rest uniform over the 1000 location tokens; no HARD token"""
    rng = np.random.default_rng(seed)
    text = np.array(list(RC.OCR_TEXT_IDS) + [SP])
    ids = np.full((n, RANDOM_T), PAD, np.int32)
    logp = np.full((n, RANDOM_T - 1), np.nan, np.float32)
    for r in range(n):
        m = int(rng.integers(1, 49))
        u = rng.random(m)
        row = np.where(u < 0.03, rng.choice([BOS, PAD], size=m), np.where(u < 0.03 + text_share, rng.choice(text, size=m), LOC0 + rng.integers(0, 1000, size=m)))
        ids[r, 0], ids[r, 1:1 + m], ids[r, 1 + m] = START, row, EOS
        logp[r, :m + 1] = -rng.random(m + 1, dtype=np.float32) * 3
    return ids, logp


# ---------------------------------------------------------------------------------------------- launches
def launch_boxes(L, dev, sync, ids, table, logp, cells, T, R, grammar, pad_ids=2, pad_logp=3, what="box parse", slots=None):
    """one launch, every operand in one guard-banded arena; ids and logp rows are wider than their data (the padding holds 0xFF
    bytes: id -1, NaN).  -> (records [n, M, 16], sums [n, M, 2], rows [n, 4]) as numpy"""
    from omniparser_amd.florence import box_parse_op
    n, M = ids.shape[0], (T - 1) // 4
    ar = CF.Arena()
    ar.add("ids", torch.int32, n, T + pad_ids, data=((0, torch.from_numpy(ids)),))
    ar.add("table", torch.int16, 1, len(table), data=((0, torch.from_numpy(table.astype(np.int16))[None]),))
    if logp is not None:
        ar.add("logp", torch.float32, n, T - 1 + pad_logp, data=((0, torch.from_numpy(logp)),))
    ar.add("cells", torch.int32, n, 6, data=((0, torch.tensor(cells, dtype=torch.int32)),))
    ar.add("rec", torch.int32, n * M, 16, out=((0, 16),))
    ar.add("sums", torch.float32, 1, n * M * 2, out=((0, n * M * 2),))
    ar.add("rows", torch.int32, n, 4, out=((0, 4),))
    ar.build(dev)
    op = box_parse_op(ar.ptr("ids"), ar.ptr("table"), ar.ptr("logp") if logp is not None else None, ar.ptr("cells"), ar.ptr("rec"),
                      ar.ptr("sums"), ar.ptr("rows"), n, T, len(table), R, EOS, grammar, ld_ids=T + pad_ids, ld_logp=T - 1 + pad_logp, slots=slots)
    L.launch(op)
    sync()
    ar.fetch(what)
    return (ar.get("rec", 0, 16).numpy().reshape(n, M, 16), ar.get("sums", 0, n * M * 2).numpy().reshape(n, M, 2), ar.get("rows", 0, 4).numpy())


def _class_table(tmp_dir):
    proc, post = RC.oracle(tmp_dir)
    table, texts = proc.loc_class_table()
    assert texts[SP] == " " and table[SP] == TEXT and table[TOK_LT] == HARD and table[TOK_NL] == HARD and all(table[t] == TEXT for t in RC.OCR_TEXT_IDS)
    assert table[LOC0] == 0 and table[LOC0 + 999] == 999 and table[BOS] == table[PAD] == table[EOS] == STRIP and len(table) == 1400
    return proc, post, table, texts


def _compare(L, dev, sync, tmp_dir, ids, logp, names, T, R, grammar, origins):
    """launch, then: bits of the twin; labels and boxes of transformers (rows without a HARD token) or the host fallback equal to
    transformers (rows with one).  -> (records, sums, rows)"""
    from omniparser_amd.util import utils as U
    proc, post, table, texts = _class_table(tmp_dir)
    n = ids.shape[0]
    cells = [[ox, oy, -2 ** 31, INF, -2 ** 31, INF] for ox, oy in origins]
    rec, sums, rows = launch_boxes(L, dev, sync, ids, table, logp, cells, T, R, grammar)
    t_rec, t_sums, t_rows = twin_boxes(ids, table, logp, cells, T, R, grammar)
    assert np.array_equal(rows, t_rows), (names, rows.tolist(), t_rows.tolist())
    assert np.array_equal(rec, t_rec), names
    assert np.array_equal(sums.view(np.int32), t_sums.view(np.int32)), names
    assert not np.isnan(sums).any()
    if logp is None:
        assert not np.any(sums)
    for r in range(n):
        row = ids[r].tolist()
        found, _kept, flags, phrases = (int(v) for v in rows[r])
        name = names[r] if names else f"random row {r}"
        if "beyond_table" in name:                          # transformers cannot render an id its tokenizer does not know
            assert flags & 1
            continue
        ox, oy = origins[r]
        if flags & 1:
            got = [(g["label"], g["bbox"]) for g in U.parse_box_answer(row, proc, (R, R), grammar)]
        else:
            got = [(box_label(row, rec[r, k], table, texts), [int(rec[r, k, 3]) - ox, int(rec[r, k, 4]) - oy, int(rec[r, k, 5]) - ox, int(rec[r, k, 6]) - oy])
                   for k in range(found)]
            assert phrases == len({int(rec[r, k, 10]) for k in range(found)})
        for which in ORACLES[grammar]:
            want = oracle_boxes(post, row, R, which)
            assert got == want, (name, grammar, which, got, want)
        if names:
            assert ("hard" in name) == bool(flags & 1), name
    return rec, sums, rows


def check_boxes(L, dev, tmp_dir, T, n, grammar, R=64, sync=lambda: None, with_logp=True):
    """one launch of n listed rows of T tokens"""
    ids, logp, names = parse_rows(T, n)
    origins = [(13 * (r % 3), 7 * (r % 2)) for r in range(n)]
    _compare(L, dev, sync, tmp_dir, ids, logp if with_logp else None, names, T, R, grammar, origins)
    return names


def check_random(L, dev, tmp_dir, grammar, text_share, n=400, R=64, sync=lambda: None):
    """one launch of n rows of the seeded random generator -> the number of boxes the oracle and the device agree on"""
    ids, logp = random_rows(n, text_share, seed=int(1000 * text_share) + grammar)
    _rec, _sums, rows = _compare(L, dev, sync, tmp_dir, ids, logp, None, RANDOM_T, R, grammar, [(0, 0)] * n)
    assert not rows[:, 2].any()                             # no HARD token, every row has its EOS
    return int(rows[:, 0].sum())


def check_expected(L, dev, tmp_dir, sync=lambda: None):
    """the rows of the issue's list give what it says they give (T = 65, every case once, both grammars): boxes, phrases, flags,
    and for the named ones the columns and bins"""
    _proc, _post, table, texts = _class_table(tmp_dir)
    T, R = 65, 64
    cases = gen_cases(T)
    names = list(cases)
    ids = np.full((len(names), T), PAD, np.int32)
    for r, name in enumerate(names):
        g, eos = cases[name]
        row = [START] + g + ([EOS] if eos else [])
        ids[r, :len(row)] = row
    cells = [[0, 0, -2 ** 31, INF, -2 ** 31, INF]] * len(names)
    out = {}
    for grammar in (0, 1):
        rec, sums, rows = launch_boxes(L, dev, sync, ids, table, None, cells, T, R, grammar)
        assert not np.any(sums)
        out[grammar] = rec
        got = {name: (int(rows[r, 0]), int(rows[r, 3]), int(rows[r, 2])) for r, name in enumerate(names)}
        M = (T - 1) // 4
        want0 = {"eos_in_column_1": (0, 0, 0), "text_only": (0, 0, 0), "three_locs_only": (0, 0, 0), "text_4_whole_row": (1, 1, 0),
                 "five_leading_locs": (1, 1, 0), "text_4": (1, 1, 0), "text_5": (1, 1, 0), "text_6": (1, 1, 0), "text_7": (1, 1, 0),
                 "hard_lt": (1, 1, 1), "four_locs_only": (0, 0, 0), "text_8_one_phrase_two_boxes": (2, 1, 0), "nine_leading_locs": (2, 1, 0),
                 "text_3_text_4_lead_phrase": (1, 1, 0), "four_locs_text_4": (1, 1, 0), "strips_inside": (2, 1, 0), "id_beyond_table": (1, 1, 1),
                 "two_phrases_three_boxes": (3, 2, 0), "whitespace_phrase": (1, 1, 0), "hard_newline": (1, 1, 1), "carry_twice": (1, 1, 0),
                 "no_eos_text": (0, 0, 2), "every_slot_in_grammar_1": (M - 1, 1, 2)}
        want1 = dict(want0, five_leading_locs=(1, 1, 0), four_locs_only=(1, 1, 0), nine_leading_locs=(2, 1, 0), text_3_text_4_lead_phrase=(1, 1, 0),
                     four_locs_text_4=(2, 2, 0), carry_twice=(1, 1, 0), every_slot_in_grammar_1=(M, 1, 2))
        assert got == (want0, want1)[grammar], (grammar, got)
    r0, r1 = out[0], out[1]
    px = lambda *b: [((2 * k + 1) * R) // 2000 for k in b]                                                          # noqa: E731
    r = names.index("five_leading_locs")                    # grammar 0: <loc_7> is the phrase, the box is BOX_A; grammar 1: 7, 10, 20, 500
    assert r0[r, 0, 1:3].tolist() == [1, 2] and r0[r, 0, 11] == 1 and r0[r, 0, 7] == 2 and r0[r, 0, 3:7].tolist() == px(10, 20, 500, 300)
    assert box_label(ids[r].tolist(), r0[r, 0], table, texts) == "loc_7>"
    assert r1[r, 0, 1:3].tolist() == [1, 1] and r1[r, 0, 7] == 1 and r1[r, 0, 3:7].tolist() == px(7, 10, 20, 500) and r1[r, 0, 8] == 0
    r = names.index("nine_leading_locs")
    assert r0[r, 1, 3:7].tolist() == px(0, 999, 999, 0) and r1[r, 1, 3:7].tolist() == px(300, 0, 999, 999)
    r = names.index("text_8_one_phrase_two_boxes")          # two boxes, one phrase ordinal
    assert r0[r, :2, 10].tolist() == [0, 0] and r0[r, :2, 7].tolist() == [2, 6] and r0[r, :2, 1].tolist() == [1, 1]
    r = names.index("text_3_text_4_lead_phrase")            # A l l l B BOX_B: the phrase starts at the third location token's column
    assert r0[r, 0, 1:3].tolist() == [4, 6] and r0[r, 0, 11] == 1 and r0[r, 0, 8] == 2 and box_label(ids[r].tolist(), r0[r, 0], table, texts) == "loc_500>B"
    r = names.index("four_locs_text_4")
    assert r0[r, 0, 1:3].tolist() == [4, 6] and r0[r, 0, 11] == 1 and r0[r, 0, 3:7].tolist() == px(0, 999, 999, 0)
    r = names.index("strips_inside")                        # <s> A <pad> B l l <s> l l <pad> BOX_B: phrase columns 2..4, two tokens
    assert r0[r, 0, 1:3].tolist() == [2, 5] and r0[r, 0, 8] == 2 and r0[r, :2, 7].tolist() == [5, 11] and r0[r, 0, 3:7].tolist() == px(10, 20, 500, 300)
    r = names.index("two_phrases_three_boxes")
    assert r0[r, :3, 10].tolist() == [0, 1, 1] and r0[r, :3, 1].tolist() == [1, 7, 7]
    r = names.index("carry_twice")                          # A l l l B l l C BOX_C: the phrase is the LAST left-over token + C
    assert r0[r, 0, 1:3].tolist() == [7, 9] and r0[r, 0, 11] == 1
    r = names.index("whitespace_phrase")
    assert box_label(ids[r].tolist(), r0[r, 0], table, texts) == "" and r0[r, 0, 8] == 1
    assert r0[names.index("text_4"), 0, 3:7].tolist() == px(10, 20, 500, 300) == [0, 1, 32, 19]


def check_ownership(L, dev, tmp_dir, sync=lambda: None):
    """RC.check_ownership's 3 x 2 grid (x boundaries, doubled, 107 and 193; y boundary 100), four boxes per tile — the fourth the first
    with x1 < x0: the centre is the same — and the y boundary exactly"""
    from omniparser_amd.pipeline import ScreenParser
    _proc, _post, table, _texts = _class_table(tmp_dir)
    R, T = 64, 65
    origins = ScreenParser.tile_origins(150, 100, R, R, 16)[0]
    cells = RC.grid_cells(origins, R)
    assert cells[0] == [0, 0, -2 ** 31, 107, -2 ** 31, 100] and cells[4] == [43, 36, 107, 193, 100, INF]

    def box(x0, y0, x1, y1):              # bins whose de-quantised corners are exactly these tile pixels at R = 64
        return loc(*[next(k for k in range(1000) if ((2 * k + 1) * R) // 2000 == v) for v in (x0, y0, x1, y1)])
    row = [START, BOS, A] + box(10, 5, 11, 9) + [B] + box(10, 5, 10, 9) + [C] + box(40, 30, 50, 34) + [A] + box(11, 5, 10, 9) + [EOS]
    ids = np.full((len(origins), T), PAD, np.int32)
    ids[:, :len(row)] = row
    for grammar in (0, 1):
        rec, _sums, rows = launch_boxes(L, dev, sync, ids, table, None, cells, T, R, grammar)
        t_rec, _t, t_rows = twin_boxes(ids, table, None, cells, T, R, grammar)
        assert np.array_equal(rec, t_rec) and np.array_equal(rows, t_rows)
        kept = [[int(rec[r, k, 9]) for k in range(4)] for r in range(len(origins))]
        # doubled centres in tile pixels: 21, 20, 90, 21 on x; 14, 14, 64, 14 on y (see RC.check_ownership for the arithmetic)
        assert kept == [[1, 1, 1, 1], [1, 0, 1, 1], [1, 0, 1, 1], [0, 0, 1, 0], [0, 0, 1, 0], [0, 0, 1, 0]], kept
        assert rows[:, 0].tolist() == [4] * 6 and rows[:, 1].tolist() == [4, 3, 3, 1, 1, 1]
        assert rec[1, 3, 3] > rec[1, 3, 5]                  # x1 < x0 reaches the record as it is
    row0 = [START, BOS, A] + box(5, 50, 9, 50) + [EOS]      # doubled y centre 100 in frame pixels: tile 0 50 + 50, tile 3 14 + 14 + 72
    row3 = [START, BOS, A] + box(5, 14, 9, 14) + [EOS]
    ids2 = np.full((2, T), PAD, np.int32)
    ids2[0, :len(row0)], ids2[1, :len(row3)] = row0, row3
    rec2, _s, _r = launch_boxes(L, dev, sync, ids2, table, None, [cells[0], cells[3]], T, R, 0)
    assert rec2[0, 0, 4] + rec2[0, 0, 6] == 100 == rec2[1, 0, 4] + rec2[1, 0, 6] and [int(rec2[0, 0, 9]), int(rec2[1, 0, 9])] == [0, 1]


def check_errors(L, dev, tmp_dir, sync=lambda: None):
    """mode 1's argument errors in mode 3, M != (T - 1) // 4 (mode 1's M among them), a grammar outside 0..1, mode 2 with mode-3
    arguments: OMNI_E_ARG, outputs untouched; then the good launch"""
    from omniparser_amd.florence import box_parse_op
    _proc, _post, table, _texts = _class_table(tmp_dir)
    T, n, R = 19, 3, 64
    M = (T - 1) // 4
    ids, logp, _ = parse_rows(T, n)
    d = {"ids": torch.from_numpy(ids).to(dev), "table": torch.from_numpy(table.astype(np.int16)).to(dev), "logp": torch.from_numpy(logp).to(dev),
         "cells": torch.tensor([[0, 0, -2 ** 31, INF, -2 ** 31, INF]] * n, dtype=torch.int32).to(dev),
         "rec": torch.full((n * M * 16,), -7, dtype=torch.int32).to(dev), "sums": torch.full((n * M * 2,), -7.0).to(dev),
         "rows": torch.full((n * 4,), -7, dtype=torch.int32).to(dev)}
    sync()
    p = {k: t.data_ptr() for k, t in d.items()}
    seen = []
    for what, kw in (("M too large", dict(slots=M + 1)), ("M too small", dict(slots=M - 1)), ("mode 1's M", dict(slots=(T - 1) // 9)),
                     ("T = 1", dict(T=1, slots=0)), ("T beyond the limit", dict(T=2050, slots=512)), ("null ids", dict(ids=None)),
                     ("null table", dict(table=None)), ("null records", dict(rec=None)), ("null sums", dict(sums=None)), ("null rows", dict(rows=None)),
                     ("null cells", dict(cells=None)), ("table_len = 0", dict(table_len=0)), ("ids stride below T", dict(ld_ids=T - 1)),
                     ("logp stride below T - 1", dict(ld_logp=T - 2)), ("n = 0", dict(n=0)), ("R = 0", dict(R=0)), ("grammar 2", dict(grammar=2)),
                     ("grammar -1", dict(grammar=-1)), ("mode 2", dict(mode=2)), ("mode 4", dict(mode=4))):
        a = dict(p, n=n, T=T, table_len=len(table), R=R, ld_ids=0, ld_logp=0, slots=None, mode=3, grammar=0)
        a.update(kw)
        op = box_parse_op(a["ids"], a["table"], a["logp"], a["cells"], a["rec"], a["sums"], a["rows"], a["n"], a["T"], a["table_len"], a["R"],
                          EOS, a["grammar"], ld_ids=a["ld_ids"], ld_logp=a["ld_logp"], slots=a["slots"])
        op.i[0] = a["mode"]
        rc = L.lib().omni_op_launch(ctypes.byref(op), L._stream_ptr(None))
        assert rc == E_ARG, (what, rc)
        seen.append((what, L.lib().omni_last_error().decode()))
    sync()
    assert all(bool((d[k].cpu() == -7).all()) for k in ("rec", "sums", "rows"))
    cells = d["cells"].cpu().tolist()
    for grammar in (0, 1):
        L.launch(box_parse_op(p["ids"], p["table"], p["logp"], p["cells"], p["rec"], p["sums"], p["rows"], n, T, len(table), R, EOS, grammar))
        sync()
        t_rec, t_sums, t_rows = twin_boxes(ids, table, logp, cells, T, R, grammar)
        assert np.array_equal(d["rec"].cpu().numpy().reshape(n, M, 16), t_rec) and np.array_equal(d["rows"].cpu().numpy().reshape(n, 4), t_rows)
        assert np.array_equal(d["sums"].cpu().numpy().reshape(n, M, 2).view(np.int32), t_sums.view(np.int32))
    return seen


# ---------------------------------------------------------------------------------------------- captioner against transformers
BOX_PHRASES = ("AB", "C D")            # two short phrases of <OPEN_VOCABULARY_DETECTION>: 2 prompts x 6 tiles = 12 rows
BOX_SEED = 1                           # see `box_reference` for what the oracle gives at it


def box_reference(tmp_dir, eos_prone, seed=BOX_SEED, R=64, frame_whl=RC.OCR_FRAME, max_new=RC.OCR_MAX_NEW):
    """transformers on the CPU for prompts x tiles of the seeded frame, prompt-major: dict(img, tiles, prompts, rows [(prompt, tile)],
    pix [rows, 3, R, R] of the host-cut tiles, suppress, seq, margins, logp [rows, T - 1], boxes: per row the post-processor's
    [(label, box)] of parse_description_with_bboxes_from_text_and_spans, eos)

    What THE ORACLE ALONE gives at BOX_SEED with BOX_PHRASES and generation restricted to the location tokens and RC.OCR_TEXT_IDS
    (transformers on the CPU, chosen and recorded before any device run; `check_locate_regions` asserts it again), seeds scanned from 0:
      seed 0, stock checkpoint   14 or 15 boxes in each of the 12 rows, but the smallest top-1 / top-2 margin is 9.1e-6, below
                                 gpu_checks.CAPTION_MARGIN: NOT used
      seed 1, stock checkpoint   boxes per row [14, 14, 14, 14, 15, 15, 15, 15, 15, 15, 15, 15]; 146 of the 174 boxes belong to a phrase
                                 with lead = 1 (the allowed set is 96 % location tokens, so most phrases start inside a left-over
                                 location token); 15 phrases carry two or more boxes; every row 64 tokens long; smallest margin 2.5e-4
      EOS-prone checkpoint       the EOS token beats every allowed token at the first free step: 12 rows, no box, 3 columns per row
                                 (one row 6) — the early exit after the first poll"""
    import beam_checks as BC
    import prompt_checks as P
    from omniparser_amd.pipeline import ScreenParser
    proc, post = RC.oracle(tmp_dir)
    W, H, overlap = frame_whl
    img = RC.frame(W, H, seed)
    tiles = ScreenParser.tile_origins(W, H, R, R, overlap)[0]
    tile_pix = RC.host_tiles(img, tiles, R)
    prompts = [proc.task_prompt_ids(OVD, text=q) for q in BOX_PHRASES]
    rows = [(p, t) for p in range(len(prompts)) for t in range(len(tiles))]
    pix = tile_pix[[t for _, t in rows]]
    ref = _generate(BC.oracle_model(0, eos_prone), pix, [prompts[p] for p, _ in rows], R, max_new)
    boxes = []
    for r in ref["seq"].tolist():
        end = next((j for j in range(1, len(r)) if r[j] == ref["eos"]), len(r))
        known = [t for t in r[:end] if 0 <= t < 1400]          # (an id the synthetic tokenizer does not know cannot be rendered)
        boxes.append(oracle_boxes(post, known, R, "description", eos=-1) if len(known) == end else None)
    return dict(ref, img=img, tiles=tiles, prompts=prompts, rows=rows, pix=pix, boxes=boxes)


def _generate(model, pix, prompt_rows, R, max_new):
    """greedy generate() of transformers with one prompt per row, restricted as RC.ocr_suppress restricts: dict(suppress, seq, margins,
    logp, eos)"""
    import prompt_checks as P
    try:
        eos = model.generation_config.eos_token_id
        suppress = RC.ocr_suppress(model.config.get_text_config().vocab_size, keep=(BOS, EOS, eos))
        ids, mask = P.hf_inputs(model, R, prompt_rows)
        with torch.inference_mode():
            out = model.generate(input_ids=ids, attention_mask=mask, pixel_values=pix, max_new_tokens=max_new, num_beams=1, do_sample=False,
                                 output_scores=True, return_dict_in_generate=True, suppress_tokens=suppress)
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
    return dict(suppress=suppress, seq=seq, margins=margins, logp=ts.float(), eos=eos)


def oracle_summary(ref, table, texts):
    """(boxes per row, phrases with lead = 1, phrases with two or more boxes) of a `box_reference`, from the oracle's own labels: a
    lead phrase is one whose label starts inside a location token ("loc_N>...")"""
    import re
    per = [len(b) for b in ref["boxes"]]
    lead = sum(1 for b in ref["boxes"] for label, _ in b if re.match(r"loc_\d+>", label))
    multi = 0
    for b in ref["boxes"]:
        multi += sum(1 for _label, grp in itertools.groupby(b, key=lambda g: g[0]) if len(list(grp)) >= 2)
    return per, lead, multi


def box_columns(row, rec, table):
    """the columns a device record counts: the non-STRIP tokens of its phrase and its four location tokens"""
    cols = [j for j in range(int(rec[1]), int(rec[2])) if table[row[j]] != STRIP]
    assert len(cols) == int(rec[8])
    j, locs = int(rec[7]), 0
    while locs < 4:
        if table[row[j]] != STRIP:
            cols.append(j)
            locs += 1
        j += 1
    return cols


def check_locate_regions(tmp_dir, eos_prone, log=None):
    """Florence2Captioner.locate_regions at R = 64 on the 150 x 100 frame, <OPEN_VOCABULARY_DETECTION> with BOX_PHRASES (12 rows), 64 new
    tokens, generation restricted to the location tokens and RC.OCR_TEXT_IDS: ids = generate() on the host-cut tiles row for row,
    token-exact against transformers on the CPU (margins asserted first), boxes and labels = the post-processor on transformers'
    sequences plus the tile's origin, mean log-probabilities within RC.TOL_LOGP"""
    import prompt_checks as P
    from omniparser_amd.florence import Florence2Captioner
    from omniparser_amd.util import utils as U
    ref = box_reference(tmp_dir, eos_prone)
    _W, _H, overlap = RC.OCR_FRAME
    R, n = 64, len(ref["rows"])
    assert n == 12
    ckpt = RC.caption_dir_with_tokenizer(tmp_dir, eos_prone)
    cap = Florence2Captioner(ckpt, "cuda", precision="f32", resolution=R)
    proc = U.FlorenceProcessor(ckpt, image_token_id=cap.w.cfg.get("image_token_id", 51289), special_ids=(cap.w.bos, cap.w.pad, cap.w.eos, 3))
    table, texts = proc.loc_class_table()
    per, lead, multi = oracle_summary(ref, table, texts)
    if eos_prone:                                           # the EOS token beats every allowed token at once: no row has a box
        assert per == [0] * n, per
    else:
        assert min(per) >= 1 and lead >= 1 and multi >= 1, (per, lead, multi)
    finite = [m for m in ref["margins"] if m != float("inf")]
    if finite:
        P.assert_margins(finite, f"box answers eos_prone={eos_prone}")
    gen = {"suppress_tokens": ref["suppress"]}
    out = cap.locate_regions(torch.from_numpy(ref["img"]).cuda(), ref["prompts"], table, 0, max_new_tokens=RC.OCR_MAX_NEW, overlap=overlap, controls=gen)
    assert out.origins == [ref["tiles"][t] for _, t in ref["rows"]] and tuple(out.ids.shape) == (n, RC.OCR_MAX_NEW + 1)
    assert list(zip(out.prompt_index, out.tile_index)) == ref["rows"]
    prompt_rows = [ref["prompts"][p] for p, _ in ref["rows"]]
    n_img = (R // 32) ** 2 + 1
    width = max(len(r) for r in prompt_rows)
    inp = torch.tensor([[proc.image_token_id] * n_img + r + [PAD] * (width - len(r)) for r in prompt_rows])
    mask = torch.tensor([[1] * (n_img + len(r)) + [0] * (width - len(r)) for r in prompt_rows])
    g = cap.generate(input_ids=inp, attention_mask=mask, pixel_values=ref["pix"], max_new_tokens=RC.OCR_MAX_NEW, output_scores=True,
                     return_dict_in_generate=True, **gen)
    worst, leads = 0.0, 0
    for b in range(n):
        mine = P._trim(out.ids[b])
        assert mine == P._trim(g.sequences[b]), (b, mine, g.sequences[b].tolist())
        assert mine == P._trim(ref["seq"][b]), (b, mine, ref["seq"][b].tolist())
        row = out.ids[b].tolist()
        found, _kept, flags, _phrases = (int(v) for v in out.rows[b])
        assert flags == 0 or (flags == 2 and ref["eos"] not in row[1:]), (b, flags)
        ox, oy = out.origins[b]
        got = [(box_label(row, out.records[b, k], table, texts), [int(out.records[b, k, 3]) - ox, int(out.records[b, k, 4]) - oy,
                                                                  int(out.records[b, k, 5]) - ox, int(out.records[b, k, 6]) - oy]) for k in range(found)]
        assert got == ref["boxes"][b], (b, got, ref["boxes"][b])
        for k in range(found):
            cols = box_columns(row, out.records[b, k], table)
            want = float(sum(float(ref["logp"][b, j - 1]) for j in cols)) / len(cols)
            have = (float(out.sums[b, k, 0]) + float(out.sums[b, k, 1])) / (int(out.records[b, k, 8]) + 4)
            worst = max(worst, abs(want - have))
            leads += int(out.records[b, k, 11])
    line = (f"locate_regions eos_prone={eos_prone}: boxes per row {per}, lead phrases {lead}, phrases with >= 2 boxes {multi}, steps {cap.last_steps}, "
            f"max |d mean logp| = {worst:.3e} (bound {RC.TOL_LOGP:.2e})")
    print(line)
    if log is not None:
        log.append(line)
    assert worst <= RC.TOL_LOGP, worst
    assert eos_prone or leads >= 1
    return cap, proc, ref, out


DESCRIBE_BOXES = ([5, 5, 40, 30], [100, 10, 140, 40], [60, 70, 90, 95])       # frame pixels of the 150 x 100 frame: tiles 0, 2 and 4
DESCRIBE_TILES = (0, 2, 4)


def describe_rows(proc, tiles, R, task="<REGION_TO_DESCRIPTION>", boxes=DESCRIBE_BOXES, owners=DESCRIBE_TILES):
    """(origins, prompt rows) `describe_regions` must hand to `decode_tiles` for DESCRIBE_BOXES: the owning tile's origin, the box
    clipped to that tile, quantised in tile coordinates"""
    origins, prompts = [], []
    for b, t in zip(boxes, owners):
        ox, oy = tiles[t]
        clip = lambda v: min(max(v, 0), R)                  # noqa: E731
        origins.append((ox, oy))
        prompts.append(proc.task_prompt_ids(task, region=[clip(b[0] - ox), clip(b[1] - oy), clip(b[2] - ox), clip(b[3] - oy)], size=(R, R)))
    return origins, prompts


def check_describe_regions(tmp_dir, max_new=16):
    """util.utils.describe_regions with three boxes in different tiles of the 150 x 100 frame at R = 64: the rows it decodes are
    `describe_rows`, their ids token-exact against transformers with the same prompt rows on the host-cut tiles, the texts
    batch_decode of those"""
    import os
    import beam_checks as BC
    import prompt_checks as P
    from omniparser_amd.pipeline import ScreenParser
    from omniparser_amd.util import utils as U
    W, H, overlap = RC.OCR_FRAME
    R = 64
    img = RC.frame(W, H)
    tiles = ScreenParser.tile_origins(W, H, R, R, overlap)[0]
    os.environ["OMNI_CAPTION_RES"] = "64"
    try:
        cmp_ = U.get_caption_model_processor("florence2", str(RC.caption_dir_with_tokenizer(tmp_dir)), "cuda")
    finally:
        os.environ.pop("OMNI_CAPTION_RES", None)
    model, proc = cmp_["model"], cmp_["processor"]
    origins, prompts = describe_rows(proc, tiles, R)
    assert len({tuple(p) for p in prompts}) == 3
    ref = _generate(BC.oracle_model(0, False), RC.host_tiles(img, origins, R), prompts, R, max_new)
    finite = [m for m in ref["margins"] if m != float("inf")]
    if finite:
        P.assert_margins(finite, "region prompts")
    gen = {"suppress_tokens": ref["suppress"]}
    calls = []
    real = model.decode_tiles

    def spy(image_u8, origins, prompts, max_new_tokens, controls=None):
        out = real(image_u8, origins, prompts, max_new_tokens, controls=controls)
        calls.append((list(origins), [list(p) for p in prompts], out))
        return out
    model.decode_tiles = spy
    try:
        texts = U.describe_regions(img, [list(b) for b in DESCRIBE_BOXES], cmp_, max_new_tokens=max_new, overlap=overlap, generation=gen)
    finally:
        del model.decode_tiles
    assert len(calls) == 1 and calls[0][0] == origins and calls[0][1] == prompts
    out = calls[0][2]
    for b in range(3):
        assert P._trim(out.ids[b]) == P._trim(ref["seq"][b]), (b, out.ids[b].tolist(), ref["seq"][b].tolist())
    assert texts == [t.strip() for t in proc.batch_decode(ref["seq"], skip_special_tokens=True)] and len(texts) == 3
    return texts


def check_locate_regions_768():
    """R = 768, a 900 x 800 frame (4 tiles at overlap 128), 16 new tokens, no tokenizer-dependent part: the ids equal generate() on
    the host-cut tiles, and the records are the twin's on those ids"""
    import prompt_checks as P
    from omniparser_amd.florence import Florence2Captioner, PROMPT_IDS, ocr_cells
    from omniparser_amd.pipeline import ScreenParser
    from tools.make_weights import ensure_caption_checkpoint
    R, max_new = 768, 16
    img = RC.frame(900, 800)
    origins = ScreenParser.tile_origins(900, 800, R, R, 128)[0]
    assert origins == [(0, 0), (132, 0), (0, 32), (132, 32)]
    pix = RC.host_tiles(img, origins, R)
    cap = Florence2Captioner(ensure_caption_checkpoint(0), "cuda", precision="f32", resolution=R)
    table = np.full((cap.w.vocab,), TEXT, np.uint16)
    table[1000:2000] = np.arange(1000)                      # a thousand ids of the stand-in's vocabulary count as location bins
    out = cap.locate_regions(torch.from_numpy(img).cuda(), [list(PROMPT_IDS)], table, 0, max_new_tokens=max_new, overlap=128)
    g = cap.generate(pixel_values=pix, max_new_tokens=max_new, output_scores=True, return_dict_in_generate=True)
    for b in range(4):
        assert P._trim(out.ids[b]) == P._trim(g.sequences[b]), b
    ids = out.ids.numpy().astype(np.int32)
    t_rec, t_sums, t_rows = twin_boxes(ids, table, out.logp.numpy(), ocr_cells(origins, R), max_new + 1, R, 0, eos=int(cap.w.eos))
    assert np.array_equal(out.records.numpy(), t_rec) and np.array_equal(out.rows.numpy(), t_rows)
    assert np.array_equal(out.sums.numpy().view(np.int32), t_sums.view(np.int32))
    return out


# ---------------------------------------------------------------------------------------------- the host surface
class StandInLocator(RC.StandInReader):
    """RC.StandInReader with `locate_regions` and `decode_tiles`: the captioner's argument checks, row layout, and both modes of the
    real op (launched on the emulated device), the DECODE between them a lookup — row k answers with a canned row chosen by k."""

    def canned_boxes(self, k, T, poly=None):
        rows = [[BOS, A, B] + BOX_A + BOX_B,                # one phrase, two boxes
                [A] + BOX_A[:3] + [B] + BOX_B,              # a lead phrase
                [BOS, A, TOK_NL, B] + BOX_A,                # a newline: re-parsed on the host
                [BOS, C, C] + loc(100, 100, 900, 900),
                [BOS, A, B, C],                             # nothing
                [BOS, A, TOK_LT] + (poly or [B]) + BOX_A]   # a "<": re-parsed (the label is B, not A<B); with `poly` the text holds <poly>
        g = rows[k % len(rows)]
        return ([START] + g + [EOS] + [PAD] * T)[:T]

    def _checks(self, image_u8, prompts, max_new_tokens):
        from omniparser_amd import florence as FL
        rows = [[int(t) for t in r] for r in (prompts or [])]
        if not rows:
            raise ValueError("no prompts")
        for r in rows:
            FL.text_capacity(len(r))
        if isinstance(max_new_tokens, bool) or not isinstance(max_new_tokens, int) or not 1 <= max_new_tokens <= 1024:
            raise ValueError("max_new_tokens must be an integer in 1..1024")
        return rows

    def _cut(self, image_u8, origins):
        from omniparser_amd import florence as FL
        R, n = self.resolution, len(origins)
        H, W = image_u8.shape[:2]
        org = torch.tensor(origins, dtype=torch.int32)
        lut = torch.from_numpy((np.arange(256).astype(np.float64) * (1 / 255)).astype(np.float32))
        x = torch.empty((n, R, R, 4), dtype=torch.float32)
        img = image_u8.contiguous()
        self.L.launch(FL.tile_cut_op(self.L.F32, img.data_ptr(), org.data_ptr(), x.data_ptr(), lut.data_ptr(), n, H, W, R, 4))
        self.tiles = x

    def locate_regions(self, image_u8, prompts, class_table, grammar, max_new_tokens=1024, overlap=128, controls=None):
        from types import SimpleNamespace
        from omniparser_amd import florence as FL
        from omniparser_amd.pipeline import ScreenParser
        R = self.resolution
        table = FL.check_class_table(class_table)
        if grammar not in (0, 1):
            raise ValueError("grammar")
        if isinstance(overlap, bool) or not isinstance(overlap, int) or not 0 <= overlap < R:
            raise ValueError(f"overlap must be an integer in 0..{R - 1}")
        prompts = self._checks(image_u8, prompts, max_new_tokens)
        self.calls.append(dict(prompts=prompts, grammar=grammar, max_new_tokens=max_new_tokens, overlap=overlap, controls=controls))
        H, W = image_u8.shape[:2]
        tiles = ScreenParser.tile_origins(W, H, R, R, overlap)[0]
        origins = list(tiles) * len(prompts)
        n, T = len(origins), max_new_tokens + 1
        M = FL.box_slots(T)
        self._cut(image_u8, origins)
        ids = torch.tensor([self.canned_boxes(k, T, getattr(self, "poly", None)) for k in range(n)], dtype=torch.int32)
        logp = -torch.rand((n, T), generator=torch.Generator().manual_seed(n))
        cells = torch.tensor(FL.ocr_cells(origins, R), dtype=torch.int32)
        rec, sums = torch.zeros((n, max(M, 1), 16), dtype=torch.int32), torch.zeros((n, max(M, 1), 2))
        rows = torch.zeros((n, 4), dtype=torch.int32)
        self.L.launch(FL.box_parse_op(ids.data_ptr(), table.data_ptr(), logp.data_ptr() + 4, cells.data_ptr(), rec.data_ptr(), sums.data_ptr(),
                                      rows.data_ptr(), n, T, table.numel(), R, self.w.eos, grammar, ld_ids=T, ld_logp=T))
        return SimpleNamespace(origins=origins, prompt_index=[p for p in range(len(prompts)) for _ in tiles],
                               tile_index=list(range(len(tiles))) * len(prompts), records=rec[:, :M], sums=sums[:, :M], rows=rows,
                               ids=ids.long(), logp=logp[:, 1:])

    def decode_tiles(self, image_u8, origins, prompts, max_new_tokens, controls=None):
        from types import SimpleNamespace
        prompts = self._checks(image_u8, prompts, max_new_tokens)
        if len(origins) != len(prompts):
            raise ValueError("origins and prompts of different lengths")
        self.calls.append(dict(origins=list(origins), prompts=prompts, max_new_tokens=max_new_tokens, controls=controls))
        self._cut(image_u8, list(origins))
        T = max_new_tokens + 1
        answers = [[BOS, A, B], [BOS, C, SP, A], [BOS, B]]
        ids = torch.tensor([([START] + answers[k % 3] + [EOS] + [PAD] * T)[:T] for k in range(len(origins))])
        return SimpleNamespace(ids=ids, logp=torch.zeros((len(origins), T - 1)))


def check_locate(cmp_, img, kw, task=OVD, text=BOX_PHRASES):
    """util.utils.locate against the locator's own raw output: prompt-major order, only kept boxes, confidence = exp((phrase sum +
    box sum) / (n_content + 4)), boxes in frame pixels; fallback rows equal `parse_box_answer` plus the origin"""
    import math
    from PIL import Image
    from omniparser_amd.florence import ocr_cells
    from omniparser_amd.util import utils as U
    model, proc = cmp_["model"], cmp_["processor"]
    table, texts = proc.loc_class_table()
    text = list(text) if text is not None else None
    boxes, stats = U.locate(img, cmp_, task=task, text=text, return_stats=True, **kw)
    assert boxes == U.locate(Image.fromarray(img), cmp_, task=task, text=text, **kw)
    queries = text if text is not None else [None]
    prompts = [proc.task_prompt_ids(task, text=q) if q is not None else proc.prompt_ids(task) for q in queries]
    grammar = 1 if task == "<REGION_PROPOSAL>" else 0
    assert model.calls[-1]["prompts"] == prompts and model.calls[-1]["grammar"] == grammar
    raw = model.locate_regions(torch.from_numpy(img), prompts, table, grammar, max_new_tokens=kw.get("max_new_tokens", 256), overlap=kw.get("overlap", 128),
                               controls=kw.get("generation"))
    R = model.resolution
    cells = ocr_cells(raw.origins, R)
    assert len(stats) == len(raw.origins) and [s["fallback"] for s in stats] == [bool(int(f) & 1) for f in raw.rows[:, 2]]
    want = []
    for r, (ox, oy) in enumerate(raw.origins):
        row = raw.ids[r].tolist()
        q, tile = queries[raw.prompt_index[r]], raw.tile_index[r]
        assert stats[r]["query"] == q and stats[r]["tile"] == tile
        if int(raw.rows[r, 2]) & 1:
            for g in U.parse_box_answer(row, proc, (R, R), grammar):
                box = [g["bbox"][0] + ox, g["bbox"][1] + oy, g["bbox"][2] + ox, g["bbox"][3] + oy]
                cols = g["phrase_columns"] + g["box_columns"]
                if U._owns(cells[r], box):
                    want.append((g["label"], q, box, math.exp(sum(float(raw.logp[r, j - 1]) for j in cols) / len(cols)), tile, g["phrase"]))
            continue
        assert stats[r]["found"] == int(raw.rows[r, 0]) and stats[r]["kept"] == int(raw.rows[r, 1]) and stats[r]["phrases"] == int(raw.rows[r, 3])
        for k in range(int(raw.rows[r, 0])):
            rec = raw.records[r, k].tolist()
            if rec[9]:
                conf = math.exp((float(raw.sums[r, k, 0]) + float(raw.sums[r, k, 1])) / (rec[8] + 4))
                want.append((box_label(row, rec, table, texts), q, rec[3:7], conf, tile, rec[10]))
    got = [(b["label"], b["query"], b["bbox"], b["confidence"], b["tile"], b["phrase"]) for b in boxes]
    assert got == want, (got, want)
    assert all(0.0 < b["confidence"] <= 1.0 for b in boxes)
    strict = U.locate(img, cmp_, task=task, text=text, min_confidence=0.999999, **kw)
    assert all(b["confidence"] >= 0.999999 for b in strict) and len(strict) <= len(boxes)
    return boxes, stats

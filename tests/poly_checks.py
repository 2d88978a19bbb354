"""Checks shared by the CPU (emulation) and GPU tests of OMNI_OP_REGION_OCR modes 5 (polygon parse) and 6 (mask raster) and of the
calls around them (FlorenceProcessor.poly_class_table / segment_prompt_ids, util.utils.parse_polygon_answer / raster_polygons / segment /
segment_elements, Florence2Captioner.segment_regions).  Base tokenizer, frames and cells: tests/region_checks.py.

Everything here is exact; there is no tolerance but one:
  mode 5   vertices, records, row counters and log-probability sums bit-equal to `twin_polys`, a literal restatement of the op's
           semantics that shares no code with the kernel (it applies transformers' three patterns to a string with one letter per
           token); for rows without a HARD token, instances and polygons equal to transformers' Florence2PostProcessor with
           parse_tasks = "polygons" taken through .int(); for rows with one, util.utils.parse_polygon_answer equals that.
  mode 6   mask words and per-row counts bit-equal to `twin_masks` (numpy, int64, the header's edge rule); rectangles and frame
           clipping give the pixels written down in the test; Pillow's ImageDraw.polygon agrees on every pixel farther than 1.5 px
           from every edge of five simple polygons.
  confidence (GPU, captioner) the mean log-probability per instance within the project's per-token tolerance of 1.38e-4
           (profiles/long_decode_tolerance.json) of transformers' compute_transition_scores over the same tokens.

The tokenizer: region_checks.write_tokenizer's (400 text tokens, <loc_0>..<loc_999> at 400..1399) plus <sep>, <poly>, </poly> at
1400..1402 — ids the seeded checkpoint's vocabulary covers."""
import ctypes
import json
import re
from pathlib import Path

import numpy as np
import torch

import caption_f64 as CF
import region_checks as RC
from region_checks import A, B, BOS, C, E_ARG, EOS, HARD, INF, LOC0, PAD, SP, START, STRIP, TEXT, TOK_LT, TOK_NL, loc

SEP, POLY, PEND = 1400, 1401, 1402                  # token ids
C_SEP, C_POLY, C_PEND = 1003, 1004, 1005            # their classes
IMAGE_TOKEN = 1403
NEG = -2 ** 31


# ---------------------------------------------------------------------------------------------- tokenizer, class table, oracle
def write_poly_tokenizer(dst_dir):
    """region_checks.write_tokenizer's tokenizer.json plus the three polygon tokens at ids 1400..1402"""
    dst = RC.write_tokenizer(dst_dir)
    d = json.loads((dst / "tokenizer.json").read_text())
    assert max(t["id"] for t in d["added_tokens"]) == SEP - 1
    d["added_tokens"] += [{"id": SEP + i, "content": t, "single_word": False, "lstrip": False, "rstrip": False, "normalized": False, "special": False}
                          for i, t in enumerate(("<sep>", "<poly>", "</poly>"))]
    (dst / "tokenizer.json").write_text(json.dumps(d))
    return dst


_ORACLE = {}


def oracle(tmp_dir):
    """(FlorenceProcessor over the polygon tokenizer, transformers' Florence2PostProcessor over the same file with the "polygons" task)"""
    if "v" not in _ORACLE:
        from transformers import PreTrainedTokenizerFast
        from transformers.models.florence2.processing_florence2 import Florence2PostProcessor
        from omniparser_amd.util import utils as U
        d = write_poly_tokenizer(Path(tmp_dir) / "tok_poly")
        tok = PreTrainedTokenizerFast(tokenizer_file=str(d / "tokenizer.json"), bos_token="<s>", eos_token="</s>", pad_token="<pad>", unk_token="<unk>")
        _ORACLE["v"] = (U.FlorenceProcessor(d, image_token_id=IMAGE_TOKEN, special_ids=(BOS, PAD, EOS, 3)), Florence2PostProcessor({"polygons": {}}, tok))
    return _ORACLE["v"]


def class_table(tmp_dir):
    proc, post = oracle(tmp_dir)
    table, texts = proc.poly_class_table()
    base, _ = proc.loc_class_table()
    assert (table[SEP], table[POLY], table[PEND]) == (C_SEP, C_POLY, C_PEND) and (base[SEP], base[POLY], base[PEND]) == (HARD, HARD, HARD)
    assert (texts[SEP], texts[POLY], texts[PEND]) == ("<sep>", "<poly>", "</poly>") and len(table) == 1403
    assert np.array_equal(np.delete(table, [SEP, POLY, PEND]), np.delete(base, [SEP, POLY, PEND]))
    assert table[LOC0] == 0 and table[LOC0 + 999] == 999 and table[BOS] == table[PAD] == table[EOS] == STRIP and table[TOK_LT] == HARD and table[A] == TEXT
    return proc, post, table, texts


def oracle_polys(post, row, size, eos=EOS):
    """transformers on one row (start token, generated ids ...; cut in front of the first EOS): per instance the list of its polygons,
    each [x0, y0, x1, y1, ...] through .int()"""
    end = next((j for j in range(1, len(row)) if row[j] == eos), len(row))
    seq = [int(t) for t in row[1:end]]
    if not seq:
        return []
    got = post(sequence=seq, parse_tasks="polygons", image_size=(size, size))["polygons"]    # (a leading <s> is skipped there and deleted anyway)
    return [[torch.tensor(p, dtype=torch.float32).int().tolist() for p in g["polygons"]] for g in got]


# ---------------------------------------------------------------------------------------------- mode 5: the literal twin
_LETTER = {STRIP: "", TEXT: "t", HARD: "h", C_SEP: "s", C_POLY: "p", C_PEND: "e"}


def twin_polys(ids, table, logp, cells, T, R, eos=EOS):
    """OMNI_OP_REGION_OCR mode 5 as include/omni_amd.h words it, on the host, with transformers' own patterns over a string that holds
    ONE LETTER PER non-STRIP TOKEN (l = location bin, s / p / e = <sep> / <poly> / </poly>, t / h = text / hard):
    -> (vertices i32 [n, V, 2], records i32 [n, P, 16], sums f32 [n, P], rows i32 [n, 4])"""
    n, P, V = len(ids), T // 2, (T - 1) // 2
    verts, rec = np.zeros((n, V, 2), np.int32), np.zeros((n, P, 16), np.int32)
    sums, rows = np.zeros((n, P), np.float32), np.zeros((n, 4), np.int32)
    for r in range(n):
        row = [int(t) for t in ids[r][:T]]
        end = next((j for j in range(1, T) if row[j] == eos), T)
        cls = [(int(table[t]) if int(table[t]) <= C_PEND else HARD) if 0 <= t < len(table) else HARD for t in row[:end]]
        cols = [j for j in range(1, end) if cls[j] != STRIP]
        text = "".join("l" if cls[j] < 1000 else _LETTER[cls[j]] for j in cols)
        c = cells[r]
        k = inst = nv = kept = 0
        for run, m in enumerate(re.finditer(r"[lspe]{4,}", text)):
            phrase = m.group()
            if not re.search(r"^(.*?)(?=l|p)", re.sub(r"^l", "", phrase, count=1)):
                continue
            if "p" in phrase and "e" in phrase:
                contents = [(m.start() + q.start(1), q.group(1)) for q in re.finditer(r"p(.*?)e", phrase)]
            else:
                contents = [(m.start(), phrase)]
            for at, content in contents:
                polys = [(at + q.start(1), len(q.group(1))) for q in re.finditer(r"(l+)(?:s|$)", content)]
                if not polys:
                    continue
                first, pts = k, []
                for ordinal, (s0, n_loc) in enumerate(polys):
                    used = cols[s0:s0 + n_loc - n_loc % 2]
                    xy = [((2 * cls[j] + 1) * R) // 2000 + c[q & 1] for q, j in enumerate(used)]
                    total = np.float32(0.0)
                    if logp is not None:
                        for j in used:
                            total = np.float32(total + np.float32(logp[r][j - 1]))
                    verts[r, nv:nv + len(xy) // 2] = np.array(xy, np.int64).reshape(-1, 2)
                    rec[r, k, :10] = [r, inst, ordinal, nv, len(xy) // 2, cols[s0], cols[s0 + n_loc - 1] + 1, n_loc, 0, run]
                    sums[r, k] = total
                    pts += xy
                    nv += len(xy) // 2
                    k += 1
                if pts:
                    box = [min(pts[0::2]), min(pts[1::2]), max(pts[0::2]), max(pts[1::2])]
                    cx, cy = box[0] + box[2], box[1] + box[3]
                    own = c[2] <= cx and (c[3] == INF or cx < c[3]) and c[4] <= cy and (c[5] == INF or cy < c[5])
                    rec[r, first:k, 8] = int(own)
                    rec[r, first:k, 10:14] = box
                    kept += int(own)
                inst += 1
        rows[r] = [k, inst, int(any(v == HARD for v in cls[1:])) | (2 if end == T else 0), kept]
    return verts, rec, sums, rows


def device_polys(rec, verts, found, origin):
    """a row's device records as the oracle's nesting, in tile pixels: per instance the list of its polygons [x0, y0, x1, y1, ...]"""
    out = []
    for k in range(found):
        if rec[k, 2] == 0:
            out.append([])
        v0, nv = int(rec[k, 3]), int(rec[k, 4])
        out[-1].append([int(v) - origin[q & 1] for q, v in enumerate(verts[v0:v0 + nv].reshape(-1).tolist())])
    return out


# ---------------------------------------------------------------------------------------------- mode 5: rows
L2, L3, L4, L6, L7 = loc(10, 20), loc(1, 2, 3), loc(100, 900, 900, 100), loc(100, 100, 900, 150, 500, 800), loc(5, 6, 7, 8, 9, 10, 11)
#                        case -> (instances, polygons, flags): what the issue's list says the row gives
WANT = {"six_plain_bins": (1, 1, 0), "two_polygons_one_instance": (1, 2, 0), "two_poly_instances": (2, 2, 0), "bins_then_poly_pair": (1, 1, 0),
        "poly_inside_poly": (1, 1, 0), "three_bins": (0, 0, 0), "text_six_text_four": (2, 2, 0), "loc_sep_sep_sep": (0, 0, 0),
        "end_four_poly": (0, 0, 0), "loc_sep_three": (1, 2, 0), "strips_between_bins": (1, 1, 0), "eos_mid_run": (1, 1, 0),
        "id_beyond_table": (1, 1, 1), "hard_lt": (1, 1, 1), "hard_newline": (2, 3, 1), "eos_in_column_1": (0, 0, 0), "text_only": (0, 0, 0)}


def gen_cases(T):
    """{name: (generated tokens without the EOS, has an EOS)} — every case of the issue's list that fits a row of T tokens; a row
    is START + generated + [EOS] + garbage"""
    cases = {
        "eos_in_column_1": ([], True),
        "text_only": ([A, B][:max(T - 2, 0)], True),
        "three_bins": (L3[:T - 2], True) if T > 3 else (L3[:2], False),
        "loc_sep_sep_sep": (loc(5) + [SEP] * 3, True),
        "end_four_poly": ([PEND] + L4 + [POLY], True),
        "six_plain_bins": (L6, True),
        "loc_sep_three": (loc(7) + [SEP] + L3, True),
        "eos_mid_run": (L4 + [EOS] + L2, True),               # the run ends at the EOS with four bins: two vertices
        "bins_then_poly_pair": ([BOS] + L2 + [POLY] + L6 + [PEND], True),
        "poly_inside_poly": ([POLY] + L6 + [POLY] + L4 + [PEND], True),
        "two_polygons_one_instance": (L6 + [SEP] + loc(1, 2, 3, 4, 5, 6), True),
        "text_six_text_four": ([BOS, A] + L6 + [B, C] + L4, True),
        "hard_lt": ([A, TOK_LT] + L6, True),
        "strips_between_bins": ([BOS] + L6[:1] + [PAD] + L6[1:3] + [BOS, PAD] + L6[3:], True),
        "id_beyond_table": ([A, 5000] + L6 + [-3], True),
        "two_poly_instances": ([POLY] + L6 + [PEND, POLY] + L7 + [PEND], True),
        "hard_newline": (L6 + [TOK_NL] + L4 + [SEP] + L2, True),
    }
    cases = {k: v for k, v in cases.items() if len(v[0]) + (2 if v[1] else 1) <= T}
    if T >= 5:
        cases["every_polygon_slot"] = ((loc(3) + [SEP]) * ((T - 1) // 2) + loc(4) * ((T - 1) % 2), False)     # T / 2 polygons of one bin
        cases["every_vertex_slot"] = (loc(*[(37 * q) % 1000 for q in range(T - 1)]), False)                   # one polygon of (T - 1) / 2 vertices
    for name, (g, eos) in cases.items():
        assert len(g) + (2 if eos else 1) <= T and (eos or len(g) == T - 1), (name, T, len(g))
    return cases


def parse_rows(T, n, seed=0):
    """n rows of T ids (numpy i32) and their log-probabilities f32 [n, T - 1], cycling through `gen_cases` from an offset that
    depends on T; behind a row's EOS: garbage ids (structure tokens and EOS among them) and NaN log-probabilities"""
    cases = gen_cases(T)
    names = list(cases)
    rng = np.random.default_rng(7000 * T + n + seed)
    ids = np.zeros((n, T), np.int32)
    logp = np.full((n, T - 1), np.nan, np.float32)
    picked = []
    for r in range(n):
        name = names[(r + T) % len(names)]
        g, eos = cases[name]
        row = [START] + g + ([EOS] if eos else [])
        used = row.index(EOS, 1) + 1 if EOS in row[1:] else len(row)
        junk = rng.choice(np.array(L6 + [SEP, POLY, PEND, EOS, A, 70000, -1, TOK_NL], dtype=np.int64), size=T - len(row))
        ids[r] = row + junk.tolist()
        logp[r, :used - 1] = -rng.random(used - 1, dtype=np.float32) * 3
        picked.append(name)
    return ids, logp, picked


RANDOM_T = 50                              # rows of 1..48 generated tokens + EOS


def random_rows(n, text_share, seed):
    """n rows of 1..48 tokens over the seven classes: `text_share` of them text, 3 % STRIP, 0.15 % HARD (`<`), 6 % each of <sep>, <poly>
    and </poly>, the rest uniform over the 1000 location tokens"""
    rng = np.random.default_rng(seed)
    text = np.array(list(RC.OCR_TEXT_IDS) + [SP])
    ids = np.full((n, RANDOM_T), PAD, np.int32)
    logp = np.full((n, RANDOM_T - 1), np.nan, np.float32)
    for r in range(n):
        m = int(rng.integers(1, 49))
        u = rng.random(m)
        edges = np.cumsum([0.03, 0.0015, text_share, 0.06, 0.06, 0.06])
        picks = [rng.choice([BOS, PAD], size=m), np.full(m, TOK_LT), rng.choice(text, size=m), np.full(m, SEP), np.full(m, POLY), np.full(m, PEND)]
        row = LOC0 + rng.integers(0, 1000, size=m)
        for e, p in reversed(list(zip(edges, picks))):
            row = np.where(u < e, p, row)
        ids[r, 0], ids[r, 1:1 + m], ids[r, 1 + m] = START, row, EOS
        logp[r, :m + 1] = -rng.random(m + 1, dtype=np.float32) * 3
    return ids, logp


def random_rows_condition(tmp_dir, text_share, n=400):
    """the generator's condition, on the CPU oracle alone: more than 100 rows yield a polygon of at least 3 vertices, at most 10 % are HARD"""
    _proc, post, table, _texts = class_table(tmp_dir)
    ids, _ = random_rows(n, text_share, seed=int(1000 * text_share) + 5)
    hard = sum(1 for r in ids if TOK_LT in r.tolist())
    good = sum(1 for r in ids if TOK_LT not in r.tolist() and any(len(p) >= 6 for g in oracle_polys(post, r.tolist(), 64) for p in g))
    assert good > 100 and hard <= n // 10, (text_share, good, hard)
    return good, hard


# ---------------------------------------------------------------------------------------------- launches
def launch_polys(L, dev, sync, ids, table, logp, cells, T, R, pad_ids=2, pad_logp=3, what="polygon parse"):
    """one launch, every operand in one guard-banded arena; ids and logp rows are wider than their data (the padding holds 0xFF
    bytes: id -1, NaN).  -> (vertices [n, V, 2], records [n, P, 16], sums [n, P], rows [n, 4]) as numpy.  (The arena takes an output
    element of all-ones bits for unwritten: the cells of these launches keep every vertex >= 0.)"""
    from omniparser_amd.florence import poly_parse_op
    n, P, V = ids.shape[0], T // 2, (T - 1) // 2
    ar = CF.Arena()
    ar.add("ids", torch.int32, n, T + pad_ids, data=((0, torch.from_numpy(ids)),))
    ar.add("table", torch.int16, 1, len(table), data=((0, torch.from_numpy(table.astype(np.int16))[None]),))
    if logp is not None:
        ar.add("logp", torch.float32, n, T - 1 + pad_logp, data=((0, torch.from_numpy(logp)),))
    ar.add("cells", torch.int32, n, 6, data=((0, torch.tensor(cells, dtype=torch.int32)),))
    ar.add("verts", torch.int32, n * V, 2, out=((0, 2),))
    ar.add("rec", torch.int32, n * P, 16, out=((0, 16),))
    ar.add("sums", torch.float32, 1, n * P, out=((0, n * P),))
    ar.add("rows", torch.int32, n, 4, out=((0, 4),))
    ar.build(dev)
    op = poly_parse_op(ar.ptr("ids"), ar.ptr("table"), ar.ptr("logp") if logp is not None else None, ar.ptr("cells"), ar.ptr("verts"), ar.ptr("rec"),
                       ar.ptr("sums"), ar.ptr("rows"), n, T, len(table), R, EOS, ld_ids=T + pad_ids, ld_logp=T - 1 + pad_logp)
    L.launch(op)
    sync()
    ar.fetch(what)
    return (ar.get("verts", 0, 2).numpy().reshape(n, V, 2), ar.get("rec", 0, 16).numpy().reshape(n, P, 16),
            ar.get("sums", 0, n * P).numpy().reshape(n, P), ar.get("rows", 0, 4).numpy())


def _compare(L, dev, sync, tmp_dir, ids, logp, names, T, R, origins):
    """launch, then: bits of the twin; instances and polygons of transformers (rows without a HARD token) or the host fallback equal
    to transformers (rows with one).  -> (vertices, records, sums, rows)"""
    from omniparser_amd.util import utils as U
    proc, post, table, _texts = class_table(tmp_dir)
    n = ids.shape[0]
    cells = [[ox, oy, NEG, INF, NEG, INF] for ox, oy in origins]
    verts, rec, sums, rows = launch_polys(L, dev, sync, ids, table, logp, cells, T, R)
    t_verts, t_rec, t_sums, t_rows = twin_polys(ids, table, logp, cells, T, R)
    assert np.array_equal(rows, t_rows), (names, rows.tolist(), t_rows.tolist())
    assert np.array_equal(rec, t_rec), (names, np.argwhere(rec != t_rec)[:4].tolist())
    assert np.array_equal(verts, t_verts), names
    assert np.array_equal(sums.view(np.int32), t_sums.view(np.int32)), names
    assert not np.isnan(sums).any()
    if logp is None:
        assert not np.any(sums)
    for r in range(n):
        row = ids[r].tolist()
        found, insts, flags, kept = (int(v) for v in rows[r])
        name = names[r] if names else f"random row {r}"
        assert kept == len({int(rec[r, k, 1]) for k in range(found) if rec[r, k, 8]}) <= insts <= found
        if "beyond_table" in name:                          # transformers cannot render an id its tokenizer does not know
            assert flags & 1
            continue
        want = oracle_polys(post, row, R)
        if flags & 1:
            got = [g["polygons"] for g in U.parse_polygon_answer(row, proc, (R, R))]
        else:
            got = device_polys(rec[r], verts[r], found, origins[r])
            assert insts == len(got)
        assert got == want, (name, got, want)
        if names:
            assert ("hard" in name) == bool(flags & 1), name
    return verts, rec, sums, rows


def check_polys(L, dev, tmp_dir, T, n, R=64, sync=lambda: None, with_logp=True):
    """one launch of n listed rows of T tokens"""
    ids, logp, names = parse_rows(T, n)
    origins = [(13 * (r % 3), 7 * (r % 2)) for r in range(n)]
    _compare(L, dev, sync, tmp_dir, ids, logp if with_logp else None, names, T, R, origins)
    return names


def check_random(L, dev, tmp_dir, text_share, n=400, R=64, sync=lambda: None):
    """one launch of n rows of the seeded random generator (its condition first, on the oracle alone) -> polygons the device found"""
    random_rows_condition(tmp_dir, text_share, n)
    ids, logp = random_rows(n, text_share, seed=int(1000 * text_share) + 5)
    _verts, _rec, _sums, rows = _compare(L, dev, sync, tmp_dir, ids, logp, None, RANDOM_T, R, [(0, 0)] * n)
    assert not (rows[:, 2] & 2).any()                       # every row has its EOS
    return int(rows[:, 0].sum())


def check_expected(L, dev, tmp_dir, sync=lambda: None):
    """the rows of the issue's list give what it says they give (T = 65, every case once): instances, polygons, flags, and for the
    named ones the columns, vertices and slots"""
    _proc, _post, table, _texts = class_table(tmp_dir)
    T, R = 65, 64
    cases = gen_cases(T)
    names = list(cases)
    ids = np.full((len(names), T), PAD, np.int32)
    for r, name in enumerate(names):
        g, eos = cases[name]
        row = [START] + g + ([EOS] if eos else [])
        ids[r, :len(row)] = row
    cells = [[0, 0, NEG, INF, NEG, INF]] * len(names)
    verts, rec, sums, rows = launch_polys(L, dev, sync, ids, table, None, cells, T, R)
    assert not np.any(sums)
    got = {name: (int(rows[r, 1]), int(rows[r, 0]), int(rows[r, 2])) for r, name in enumerate(names)}
    P, V = T // 2, (T - 1) // 2
    want = dict(WANT, every_polygon_slot=(1, P, 2), every_vertex_slot=(1, 1, 2))
    assert got == want, got
    px = lambda *b: [((2 * k + 1) * R) // 2000 for k in b]                                                          # noqa: E731
    nvs = lambda r: rec[r, :int(rows[r, 0]), 4].tolist()                                                             # noqa: E731
    r = names.index("six_plain_bins")
    assert nvs(r) == [3] and verts[r, :3].reshape(-1).tolist() == px(100, 100, 900, 150, 500, 800) and rec[r, 0, 5:8].tolist() == [1, 7, 6]
    assert rec[r, 0, 10:14].tolist() == [px(100)[0], px(100)[0], px(900)[0], px(800)[0]] and rec[r, 0, 8] == 1
    r = names.index("two_polygons_one_instance")
    assert nvs(r) == [3, 3] and rec[r, :2, 1].tolist() == [0, 0] and rec[r, :2, 2].tolist() == [0, 1] and rec[r, :2, 3].tolist() == [0, 3]
    assert rec[r, 0, 10:14].tolist() == rec[r, 1, 10:14].tolist() == [0, 0, px(900)[0], px(800)[0]]                 # over BOTH polygons
    r = names.index("two_poly_instances")                   # <poly> L6 </poly> <poly> L7 </poly>: 3 vertices each, the seventh bin dropped
    assert nvs(r) == [3, 3] and rec[r, :2, 1].tolist() == [0, 1] and rec[r, 1, 5:8].tolist() == [10, 17, 7] and rec[r, :2, 9].tolist() == [0, 0]
    r = names.index("bins_then_poly_pair")                  # <s> L2 <poly> L6 </poly>: the two leading bins belong to no instance
    assert nvs(r) == [3] and rec[r, 0, 5:7].tolist() == [5, 11]
    r = names.index("poly_inside_poly")                     # the content is L6 <poly> L4: only L4 ends the content
    assert nvs(r) == [2] and rec[r, 0, 5:7].tolist() == [9, 13] and verts[r, :2].reshape(-1).tolist() == px(100, 900, 900, 100)
    r = names.index("text_six_text_four")
    assert nvs(r) == [3, 2] and rec[r, :2, 1].tolist() == [0, 1] and rec[r, :2, 9].tolist() == [0, 1]
    r = names.index("loc_sep_three")                        # polygons [] and one vertex
    assert nvs(r) == [0, 1] and rec[r, :2, 7].tolist() == [1, 3] and rec[r, 1, 5:7].tolist() == [3, 6] and rec[r, 0, 8] == 1
    r = names.index("strips_between_bins")
    assert nvs(r) == [3] and rec[r, 0, 5:8].tolist() == [2, 11, 6] and verts[r, :3].reshape(-1).tolist() == px(100, 100, 900, 150, 500, 800)
    r = names.index("eos_mid_run")
    assert nvs(r) == [2] and rows[r, 2] == 0
    r = names.index("every_polygon_slot")                   # no vertex anywhere: an instance that is not kept, a box of zeros
    assert nvs(r) == [0] * P and not rec[r, :, 8].any() and not rec[r, :, 10:14].any() and rows[r, 3] == 0 and rec[r, P - 1, 2] == P - 1
    r = names.index("every_vertex_slot")
    assert nvs(r) == [V] and verts[r].reshape(-1).tolist() == px(*[(37 * q) % 1000 for q in range(2 * V)])


def check_ownership(L, dev, tmp_dir, sync=lambda: None):
    """box_checks.check_ownership's 3 x 2 grid (x boundaries, doubled, 107 and 193; y boundary 100) for INSTANCE boxes: four instances
    per tile whose boxes are that check's four boxes (each a polygon of two opposite corners plus one between), and the y boundary
    exactly"""
    from omniparser_amd.pipeline import ScreenParser
    _proc, _post, table, _texts = class_table(tmp_dir)
    R, T = 64, 65
    origins = ScreenParser.tile_origins(150, 100, R, R, 16)[0]
    cells = RC.grid_cells(origins, R)
    assert cells[0] == [0, 0, NEG, 107, NEG, 100] and cells[4] == [43, 36, 107, 193, 100, INF]

    def tri(x0, y0, x1, y1):              # bins whose de-quantised vertices are (x0, y0), (x1, y1), (x0, y1) in tile pixels at R = 64
        return loc(*[next(k for k in range(1000) if ((2 * k + 1) * R) // 2000 == v) for v in (x0, y0, x1, y1, x0, y1)])
    row = [START, BOS, A] + tri(10, 5, 11, 9) + [B] + tri(10, 5, 10, 9) + [C] + tri(40, 30, 50, 34) + [A] + tri(11, 5, 10, 9) + [EOS]
    ids = np.full((len(origins), T), PAD, np.int32)
    ids[:, :len(row)] = row
    verts, rec, _sums, rows = launch_polys(L, dev, sync, ids, table, None, cells, T, R)
    t_verts, t_rec, _t, t_rows = twin_polys(ids, table, None, cells, T, R)
    assert np.array_equal(rec, t_rec) and np.array_equal(rows, t_rows) and np.array_equal(verts, t_verts)
    kept = [[int(rec[r, k, 8]) for k in range(4)] for r in range(len(origins))]
    # doubled centres in tile pixels: 21, 20, 90, 21 on x; 14, 14, 64, 14 on y (see RC.check_ownership for the arithmetic)
    assert kept == [[1, 1, 1, 1], [1, 0, 1, 1], [1, 0, 1, 1], [0, 0, 1, 0], [0, 0, 1, 0], [0, 0, 1, 0]], kept
    assert rows[:, 0].tolist() == [4] * 6 and rows[:, 1].tolist() == [4] * 6 and rows[:, 3].tolist() == [4, 3, 3, 1, 1, 1]
    row0 = [START, BOS, A] + tri(5, 50, 9, 50) + [EOS]      # doubled y centre 100 in frame pixels: tile 0 50 + 50, tile 3 14 + 14 + 72
    row3 = [START, BOS, A] + tri(5, 14, 9, 14) + [EOS]
    ids2 = np.full((2, T), PAD, np.int32)
    ids2[0, :len(row0)], ids2[1, :len(row3)] = row0, row3
    _v, rec2, _s, _r = launch_polys(L, dev, sync, ids2, table, None, [cells[0], cells[3]], T, R)
    assert rec2[0, 0, 11] + rec2[0, 0, 13] == 100 == rec2[1, 0, 11] + rec2[1, 0, 13] and [int(rec2[0, 0, 8]), int(rec2[1, 0, 8])] == [0, 1]


def check_errors(L, dev, tmp_dir, sync=lambda: None):
    """mode 3's argument errors in mode 5, wrong P, wrong V, T = 2, NULL vertices, modes 2 and 4 with mode-5 arguments; mode 6 with
    I = 0 and I = 65 and its own NULLs: OMNI_E_ARG, outputs untouched; then the good launches"""
    from omniparser_amd.florence import poly_mask_op, poly_parse_op
    _proc, _post, table, _texts = class_table(tmp_dir)
    T, n, R, I = 19, 3, 64, 2
    P, V, WR = T // 2, (T - 1) // 2, 2
    ids, logp, _ = parse_rows(T, n)
    ids[0, :8], logp[0, :7] = [START] + L6 + [EOS], -0.5    # a triangle for the raster
    cells = [[0, 0, NEG, INF, NEG, INF]] * n
    d = {"ids": torch.from_numpy(ids).to(dev), "table": torch.from_numpy(table.astype(np.int16)).to(dev), "logp": torch.from_numpy(logp).to(dev),
         "cells": torch.tensor(cells, dtype=torch.int32).to(dev), "verts": torch.full((n * V * 2,), -7, dtype=torch.int32).to(dev),
         "rec": torch.full((n * P * 16,), -7, dtype=torch.int32).to(dev), "sums": torch.full((n * P,), -7.0).to(dev),
         "rows": torch.full((n * 4,), -7, dtype=torch.int32).to(dev), "mask": torch.full((n * I * R * WR,), -7, dtype=torch.int32).to(dev),
         "cnt": torch.full((n * I * R,), -7, dtype=torch.int32).to(dev)}
    sync()
    p = {k: t.data_ptr() for k, t in d.items()}
    seen = []
    for what, kw in (("P too large", dict(slots=P + 1)), ("P too small", dict(slots=P - 1)), ("mode 3's M", dict(slots=(T - 1) // 4)),
                     ("V too large", dict(vslots=V + 1)), ("V too small", dict(vslots=V - 1)), ("V = 0", dict(vslots=0)),
                     ("T = 2", dict(T=2, slots=1, vslots=0)), ("T = 1", dict(T=1, slots=0, vslots=0)), ("T beyond the limit", dict(T=2050, slots=1025, vslots=1024)),
                     ("null ids", dict(ids=None)), ("null table", dict(table=None)), ("null vertices", dict(verts=None)), ("null records", dict(rec=None)),
                     ("null sums", dict(sums=None)), ("null rows", dict(rows=None)), ("null cells", dict(cells=None)), ("table_len = 0", dict(table_len=0)),
                     ("ids stride below T", dict(ld_ids=T - 1)), ("logp stride below T - 1", dict(ld_logp=T - 2)), ("n = 0", dict(n=0)), ("R = 0", dict(R=0)),
                     ("misaligned vertices", dict(verts=p["verts"] + 2)), ("mode 2", dict(mode=2)), ("mode 4", dict(mode=4)), ("mode 7", dict(mode=7))):
        a = dict(p, n=n, T=T, table_len=len(table), R=R, ld_ids=0, ld_logp=0, slots=None, vslots=None, mode=5)
        a.update(kw)
        op = poly_parse_op(a["ids"], a["table"], a["logp"], a["cells"], a["verts"], a["rec"], a["sums"], a["rows"], a["n"], a["T"], a["table_len"], a["R"],
                           EOS, ld_ids=a["ld_ids"], ld_logp=a["ld_logp"], slots=a["slots"], vertex_slots=a["vslots"])
        op.i[0] = a["mode"]
        rc = L.lib().omni_op_launch(ctypes.byref(op), L._stream_ptr(None))
        assert rc == E_ARG, (what, rc)
        seen.append((what, L.lib().omni_last_error().decode()))
    for what, kw in (("I = 0", dict(I=0)), ("I = 65", dict(I=65)), ("masks: T = 2", dict(T=2)), ("masks: n = 0", dict(n=0)), ("masks: R = 0", dict(R=0)),
                     ("masks: H = 0", dict(H=0)), ("masks: W = 0", dict(W=0)), ("masks: null records", dict(rec=None)), ("masks: null rows", dict(rows=None)),
                     ("masks: null vertices", dict(verts=None)), ("masks: null cells", dict(cells=None)), ("masks: null masks", dict(mask=None)),
                     ("masks: null counts", dict(cnt=None))):
        a = dict(p, n=n, T=T, I=I, H=100, W=150, R=R)
        a.update(kw)
        op = poly_mask_op(a["rec"], a["rows"], a["verts"], a["cells"], a["mask"], a["cnt"], a["n"], a["T"], a["I"], a["H"], a["W"], a["R"])
        rc = L.lib().omni_op_launch(ctypes.byref(op), L._stream_ptr(None))
        assert rc == E_ARG, (what, rc)
        seen.append((what, L.lib().omni_last_error().decode()))
    sync()
    assert all(bool((d[k].cpu() == -7).all()) for k in ("verts", "rec", "sums", "rows", "mask", "cnt"))
    L.launch(poly_parse_op(p["ids"], p["table"], p["logp"], p["cells"], p["verts"], p["rec"], p["sums"], p["rows"], n, T, len(table), R, EOS))
    L.launch(poly_mask_op(p["rec"], p["rows"], p["verts"], p["cells"], p["mask"], p["cnt"], n, T, I, 100, 150, R))
    sync()
    t_verts, t_rec, t_sums, t_rows = twin_polys(ids, table, logp, cells, T, R)
    assert np.array_equal(d["rec"].cpu().numpy().reshape(n, P, 16), t_rec) and np.array_equal(d["rows"].cpu().numpy().reshape(n, 4), t_rows)
    assert np.array_equal(d["verts"].cpu().numpy().reshape(n, V, 2), t_verts)
    assert np.array_equal(d["sums"].cpu().numpy().reshape(n, P).view(np.int32), t_sums.view(np.int32))
    t_mask, t_cnt = twin_masks(t_rec, t_rows, t_verts, cells, I, 100, 150, R)
    assert np.array_equal(d["mask"].cpu().numpy().view(np.uint32).reshape(n, I, R, WR), t_mask) and np.array_equal(d["cnt"].cpu().numpy().reshape(n, I, R), t_cnt)
    assert t_cnt.any()
    return seen


# ---------------------------------------------------------------------------------------------- mode 6: the literal twin
def inside_polygon(poly, R):
    """bool [R, R] (y, x): the centre of tile pixel (x, y) lies inside `poly` [(x, y), ...] by the header's rule — doubled coordinates,
    int64, edge a -> b counts when (ay > Py) != (by > Py) and (Px - ax)(by - ay) < (Py - ay)(bx - ax) for by > ay, > otherwise"""
    px = (2 * np.arange(R, dtype=np.int64) + 1)[None, :]
    py = (2 * np.arange(R, dtype=np.int64) + 1)[:, None]
    par = np.zeros((R, R), bool)
    for k in range(len(poly)):
        ax, ay = (2 * int(v) for v in poly[k])
        bx, by = (2 * int(v) for v in poly[(k + 1) % len(poly)])
        lhs, rhs = (px - ax) * (by - ay), (py - ay) * (bx - ax)
        par ^= ((ay > py) != (by > py)) & ((lhs < rhs) if by > ay else (lhs > rhs))
    return par


def twin_masks(rec, rows, verts, cells, I, H, W, R):
    """OMNI_OP_REGION_OCR mode 6 as include/omni_amd.h words it, from mode 5's outputs [n, ...] -> (masks u32 [n, I, R, (R + 31) // 32],
    counts i32 [n, I, R])"""
    n, WR = len(rows), (R + 31) // 32
    bits = np.zeros((n, I, R, WR * 32), bool)
    for r in range(n):
        ox, oy = cells[r][0], cells[r][1]
        xs, ys = np.arange(R) + ox, np.arange(R) + oy
        frame = ((ys >= 0) & (ys < H))[:, None] & ((xs >= 0) & (xs < W))[None, :]
        for k in range(int(rows[r][0])):
            s, nv, v0 = int(rec[r, k, 1]), int(rec[r, k, 4]), int(rec[r, k, 3])
            if s < I and rec[r, k, 8] and nv >= 3:
                poly = [(int(x) - ox, int(y) - oy) for x, y in verts[r, v0:v0 + nv]]
                bits[r, s, :, :R] |= inside_polygon(poly, R) & frame
    words = (bits.reshape(n, I, R, WR, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)
    return words, bits.sum(-1).astype(np.int32)


def unpack(mask, R):
    """bool [..., R, R] of mask words [..., R, WR]"""
    b = (mask[..., None] >> np.arange(32, dtype=np.uint32)) & 1
    return b.reshape(*mask.shape[:-1], -1)[..., :R].astype(bool)


# ---------------------------------------------------------------------------------------------- mode 6: cases
RECT, TRI, CONCAVE = [(5, 4), (40, 4), (40, 30), (5, 30)], [(3, 3), (60, 10), (20, 40)], [(5, 5), (60, 5), (60, 40), (32, 15), (5, 40)]
SLIVER, ELL = [(2, 2), (68, 3), (68, 5)], [(10, 10), (50, 10), (50, 20), (25, 20), (25, 40), (10, 40)]
BOWTIE = [(4, 4), (30, 28), (30, 4), (4, 28)]
SIMPLE = {"rect": RECT, "tri": TRI, "concave": CONCAVE, "sliver": SLIVER, "ell": ELL}


def fit(poly, R):
    """the polygon scaled into a tile of R pixels (the cases are written for 70 x 45)"""
    return [(x * (R - 1) // 70, y * (R - 1) // 45) for x, y in poly]


def zigzag(R, nv=1024):
    """nv vertices: a comb along the top, closed along the bottom"""
    top = [((k * (R - 2)) // (nv - 3), 1 + (k % 2) * (R // 2)) for k in range(nv - 2)]
    return top + [(R - 2, R - 1), (0, R - 1)]


def mask_scene(R, I, origins, T=None):
    """(T, records, rows, vertices) as mode 5 would leave them for len(origins) rows, built by hand (tile-local polygons + origin):
    row r holds instances drawn from the case list, rotated by r — among them an instance of a good polygon next to a 2-vertex and a
    0-vertex one, two overlapping polygons in one instance, an instance that is not kept, a bow-tie; slots beyond I on purpose"""
    groups = [[fit(RECT, R)], [fit(TRI, R), [(1, 1), (9, 9)], []], [fit(CONCAVE, R), fit(ELL, R)], [fit(BOWTIE, R)], [fit(SLIVER, R)], [fit(ELL, R)]]
    n = len(origins)
    per_row = []
    for r in range(n):
        g = groups[r % len(groups):] + groups[:r % len(groups)]
        per_row.append([(polys, not (r % 3 == 1 and s == 0)) for s, polys in enumerate(g[:I + 1])])       # (polygons, kept)
    return build_scene(per_row, origins, T)


def build_scene(per_row, origins, T=None):
    """mode 5's outputs for per_row[r] = [(polygons of an instance, kept), ...] in tile-local pixels"""
    n = len(origins)
    need_v = max(sum(len(p) for polys, _ in row for p in polys) for row in per_row)
    need_p = max(sum(len(polys) for polys, _ in row) for row in per_row)
    T = T or max(2 * need_v + 1, 2 * need_p, 3)
    P, V = T // 2, (T - 1) // 2
    assert need_v <= V and need_p <= P
    rec, rows, verts = np.zeros((n, P, 16), np.int32), np.zeros((n, 4), np.int32), np.zeros((n, V, 2), np.int32)
    for r, row in enumerate(per_row):
        ox, oy = origins[r]
        k = nv = 0
        for s, (polys, kept) in enumerate(row):
            pts = [(x + ox, y + oy) for p in polys for x, y in p]
            box = [min(x for x, _ in pts), min(y for _, y in pts), max(x for x, _ in pts), max(y for _, y in pts)] if pts else [0, 0, 0, 0]
            for o, p in enumerate(polys):
                rec[r, k, :14] = [r, s, o, nv, len(p), 0, 0, 2 * len(p), int(kept and bool(pts)), 0, *box]
                verts[r, nv:nv + len(p)] = np.array([(x + ox, y + oy) for x, y in p], np.int64).reshape(-1, 2)
                nv += len(p)
                k += 1
        rows[r] = [k, len(row), 0, sum(1 for polys, kept in row if kept and any(polys))]
    return T, rec, rows, verts


def launch_masks(L, dev, sync, rec, rows, verts, origins, T, I, H, W, R):
    """one launch; masks and counts sit between guard words and are prefilled with a pattern no mask word of these scenes has, so a
    word that was not written or a write outside shows.  -> (masks u32 [n, I, R, WR], counts i32 [n, I, R])"""
    from omniparser_amd.florence import poly_mask_op
    n, WR, G, FILL = len(origins), (R + 31) // 32, 64, 0x5A5AA5A5
    cells = torch.tensor([[ox, oy, NEG, INF, NEG, INF] for ox, oy in origins], dtype=torch.int32).to(dev)
    d_rec, d_rows, d_verts = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (rec, rows, verts))
    mask = torch.from_numpy(np.full((G + n * I * R * WR + G,), FILL, np.uint32).view(np.int32)).to(dev)
    cnt = torch.full((G + n * I * R + G,), -7, dtype=torch.int32).to(dev)
    sync()
    L.launch(poly_mask_op(d_rec.data_ptr(), d_rows.data_ptr(), d_verts.data_ptr(), cells.data_ptr(), mask.data_ptr() + 4 * G, cnt.data_ptr() + 4 * G,
                          n, T, I, H, W, R))
    sync()
    m, c = mask.cpu().numpy().view(np.uint32), cnt.cpu().numpy()
    assert (m[:G] == FILL).all() and (m[-G:] == FILL).all() and (c[:G] == -7).all() and (c[-G:] == -7).all(), "a write outside the masks or counts"
    m, c = m[G:-G].reshape(n, I, R, WR), c[G:-G].reshape(n, I, R)
    assert not (c == -7).any() and (c >= 0).all(), "a count was not written"
    assert np.array_equal(np.array([[bin(int(w)).count("1") for w in row] for row in m.reshape(-1, WR)]).sum(1), c.reshape(-1)), "counts are not the set bits"
    return m, c


def check_masks(L, dev, R, I, frame, sync=lambda: None):
    """`mask_scene` on a tile grid over a frame of `frame` = (W, H) (plus one tile at a negative origin and one mostly outside):
    bit-equal to the twin"""
    from omniparser_amd.pipeline import ScreenParser
    W, H = frame
    origins = ScreenParser.tile_origins(W, H, R, R, min(16, R - 1))[0][:6] + [(-5, -3), (W - 7, H - 9)]
    T, rec, rows, verts = mask_scene(R, I, origins)
    m, c = launch_masks(L, dev, sync, rec, rows, verts, origins, T, I, H, W, R)
    cells = [[ox, oy] for ox, oy in origins]
    t_m, t_c = twin_masks(rec, rows, verts, cells, I, H, W, R)
    assert np.array_equal(c, t_c) and np.array_equal(m, t_m), (R, I, frame, np.argwhere(m != t_m)[:4].tolist())
    assert t_c.any() and not t_c[1 % len(origins), 0].any()                # row 1's first instance is not kept
    return int(t_c.sum())


def check_masks_known(L, dev, sync=lambda: None):
    """written-down answers at R = 40 (a partial last word): the rectangle (x0, y0)-(x1, y1) sets exactly x0..x1-1 by y0..y1-1; the
    frame's edge removes exactly the outside columns and rows; a 1024-vertex zig-zag equals the twin"""
    R, I = 40, 1
    rect = [(5, 4), (33, 4), (33, 30), (5, 30)]
    origins = [(0, 0), (20, 10), (-5, -3)]
    T, rec, rows, verts = build_scene([[([rect], True)]] * 3, origins)
    W, H = 45, 35
    m, c = launch_masks(L, dev, sync, rec, rows, verts, origins, T, I, H, W, R)
    got = unpack(m, R)[:, 0]
    want = np.zeros((3, R, R), bool)
    want[0, 4:30, 5:33] = True
    want[1, 4:25, 5:25] = True                              # frame x = 20 + x < 45, frame y = 10 + y < 35
    want[2, 4:30, 5:33] = True                              # frame x = x - 5 >= 0 from x = 5 on: nothing is cut
    assert np.array_equal(got, want)
    assert c[0, 0].tolist() == [28 if 4 <= y < 30 else 0 for y in range(R)] and c[1, 0].tolist() == [20 if 4 <= y < 25 else 0 for y in range(R)]
    origins = [(-8, -6)]
    T, rec, rows, verts = build_scene([[([rect], True)]], origins)
    m, _c = launch_masks(L, dev, sync, rec, rows, verts, origins, T, I, H, W, R)
    want = np.zeros((R, R), bool)
    want[6:30, 8:33] = True                                 # columns 5..7 and rows 4..5 lie left of / above the frame
    assert np.array_equal(unpack(m, R)[0, 0], want)
    for Rz in (40, 64):
        zz = zigzag(Rz)
        assert len(zz) == 1024
        T, rec, rows, verts = build_scene([[([zz], True)]], [(3, 2)])
        assert T == 2049
        m, c = launch_masks(L, dev, sync, rec, rows, verts, [(3, 2)], T, 1, 500, 500, Rz)
        t_m, t_c = twin_masks(rec, rows, verts, [[3, 2]], 1, 500, 500, Rz)
        assert np.array_equal(m, t_m) and np.array_equal(c, t_c) and t_c.sum() > Rz


def check_masks_768(L, dev, sync=lambda: None):
    """one R = 768 row, two instance slots, a frame the tile reaches beyond"""
    R, I = 768, 2
    origins = [(132, 32)]
    scale = lambda p: [(x * 10, y * 16) for x, y in p]                                                              # noqa: E731
    T, rec, rows, verts = build_scene([[([scale(CONCAVE), scale(ELL)], True), ([scale(BOWTIE), [(700, 700), (760, 760)]], True), ([scale(RECT)], True)]], origins)
    m, c = launch_masks(L, dev, sync, rec, rows, verts, origins, T, I, 700, 800, R)
    t_m, t_c = twin_masks(rec, rows, verts, [[132, 32]], I, 700, 800, R)
    assert np.array_equal(m, t_m) and np.array_equal(c, t_c) and t_c[0, 0].sum() > 10000 and t_c[0, 1].sum() > 10000
    assert not unpack(m, R)[0, :, :, 800 - 132:].any() and not unpack(m, R)[0, :, 700 - 32:, :].any()


def check_masks_pillow(L, dev, sync=lambda: None):
    """Pillow on the five simple polygons in a 70 x 45 frame (R = 72, one tile): every pixel whose centre is farther than 1.5 px from
    every edge equals ImageDraw.polygon(fill = 1); the excluded band stays below 25 % of the frame"""
    from PIL import Image, ImageDraw
    R, W, H = 72, 70, 45
    names = list(SIMPLE)
    T, rec, rows, verts = build_scene([[([SIMPLE[k]], True)] for k in names], [(0, 0)] * len(names))
    m, _c = launch_masks(L, dev, sync, rec, rows, verts, [(0, 0)] * len(names), T, 1, H, W, R)
    got = unpack(m, R)[:, 0, :H, :W]
    cx, cy = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    worst = 0.0
    for k, name in enumerate(names):
        poly = SIMPLE[name]
        img = Image.new("L", (W, H), 0)
        ImageDraw.Draw(img).polygon(poly, fill=1)
        ref = np.asarray(img).astype(bool)
        dist = np.full((H, W), np.inf)
        for q in range(len(poly)):
            (ax, ay), (bx, by) = poly[q], poly[(q + 1) % len(poly)]
            dx, dy = bx - ax, by - ay
            t = np.clip(((cx - ax) * dx + (cy - ay) * dy) / (dx * dx + dy * dy), 0.0, 1.0)
            dist = np.minimum(dist, np.hypot(cx - (ax + t * dx), cy - (ay + t * dy)))
        far = dist > 1.5
        band = 1.0 - far.mean()
        worst = max(worst, band)
        assert band < 0.25, (name, band)
        assert np.array_equal(got[k][far], ref[far]), (name, int((got[k][far] != ref[far]).sum()))
    return worst


# ---------------------------------------------------------------------------------------------- the host surface
SQUARE = loc(200, 200, 700, 200, 700, 700, 200, 700)
RES, R2S = "<REFERRING_EXPRESSION_SEGMENTATION>", "<REGION_TO_SEGMENTATION>"


def _standin_base():
    import box_checks as BX
    return BX.StandInLocator


class StandInSegmenter(_standin_base()):
    """box_checks.StandInLocator with `segment_regions`: the captioner's argument checks and row layout, the tile cut and modes 5 and 6
    of the real op (launched on the emulated device), the DECODE between them a lookup — row k answers with a canned row chosen by k."""

    def canned_polys(self, k, T):
        inst = lambda bins: [POLY] + bins + [PEND]                                                                  # noqa: E731
        rows = [inst(L6) + inst(SQUARE),                    # two instances
                L6 + [SEP] + SQUARE + [SEP] + L2,           # one instance: two polygons and a 1-vertex one
                [A, TOK_NL] + L6,                           # a newline: re-parsed and rastered on the host
                [BOS, A, B],                                # nothing
                inst(SQUARE) + inst(L6) + inst(loc(100, 100, 400, 100, 100, 400)) + inst(L6) + inst(SQUARE),       # five: the fifth beyond 4 slots
                loc(7) + [SEP] + loc(320, 320, 3),          # one vertex at tile pixel (20, 20): kept, a box without width or height
                loc(100, 500, 300, 500, 600, 500) + [SEP] + loc(200, 100, 200, 400, 200, 900)]                      # flat: three vertices on one y, then on one x
        g = rows[k % len(rows)]
        return ([START] + g + [EOS] + [PAD] * T)[:T]

    def segment_regions(self, image_u8, origins, prompts, class_table, max_new_tokens=256, instances=4, masks=True, controls=None, cells=None):
        from types import SimpleNamespace
        from omniparser_amd import florence as FL
        R = self.resolution
        table = FL.check_class_table(class_table)
        if isinstance(instances, bool) or not isinstance(instances, int) or not 1 <= instances <= 64:
            raise ValueError("instances must be an integer in 1..64")
        prompts = self._checks(image_u8, prompts, max_new_tokens)
        origins = [(int(x), int(y)) for x, y in origins]
        if len(origins) != len(prompts):
            raise ValueError("origins and prompts of different lengths")
        cell_rows = FL.ocr_cells(origins, R) if cells is None else [[int(v) for v in c] for c in cells]
        if len(cell_rows) != len(origins) or any(len(c) != 6 or (c[0], c[1]) != o for c, o in zip(cell_rows, origins)):
            raise ValueError("cells must hold one row per origin")
        self.calls.append(dict(origins=origins, prompts=prompts, max_new_tokens=max_new_tokens, instances=instances, masks=masks, controls=controls,
                               cells=cell_rows))
        H, W = image_u8.shape[:2]
        n, T, I, WR = len(origins), max_new_tokens + 1, instances, (R + 31) // 32
        P, V = FL.poly_slots(T)
        self._cut(image_u8, origins)
        ids = torch.tensor([self.canned_polys(k, T) for k in range(n)], dtype=torch.int32)
        logp = -torch.rand((n, T), generator=torch.Generator().manual_seed(n))
        cells = torch.tensor(cell_rows, dtype=torch.int32)
        verts, rec = torch.zeros((n, V, 2), dtype=torch.int32), torch.zeros((n, P, 16), dtype=torch.int32)
        sums, rows = torch.zeros((n, P)), torch.zeros((n, 4), dtype=torch.int32)
        mask, cnt = torch.zeros((n, I, R, WR), dtype=torch.int32), torch.zeros((n, I, R), dtype=torch.int32)
        self.L.launch(FL.poly_parse_op(ids.data_ptr(), table.data_ptr(), logp.data_ptr() + 4, cells.data_ptr(), verts.data_ptr(), rec.data_ptr(),
                                       sums.data_ptr(), rows.data_ptr(), n, T, table.numel(), R, self.w.eos, ld_ids=T, ld_logp=T))
        self.L.launch(FL.poly_mask_op(rec.data_ptr(), rows.data_ptr(), verts.data_ptr(), cells.data_ptr(), mask.data_ptr(), cnt.data_ptr(), n, T, I, H, W, R))
        return SimpleNamespace(origins=origins, vertices=verts, records=rec, sums=sums, rows=rows, masks=mask, counts=cnt, ids=ids.long(), logp=logp[:, 1:])


def brute_point(mask, origin):
    """the set pixel nearest the centroid of the set pixels, by exhaustive search with exact fractions (ties: lower y, then lower x)"""
    from fractions import Fraction
    pts = [(int(x), int(y)) for y, x in zip(*np.nonzero(mask))]
    if not pts:
        return None
    cx, cy = Fraction(sum(x for x, _ in pts), len(pts)), Fraction(sum(y for _, y in pts), len(pts))
    x, y = min(pts, key=lambda p: ((p[0] - cx) ** 2 + (p[1] - cy) ** 2, p[1], p[0]))
    return [x + origin[0], y + origin[1]]


def check_segment(cmp_, img, kw, text=None, regions=None):
    """util.utils.segment against the segmenter's own raw output and the twins: input-major order, only kept instances, polygons and
    boxes in frame pixels, masks = the twin's bits cropped to the box (device slots, host raster beyond them and on fallback rows),
    area, point by exhaustive search, confidence = exp(sum / vertex tokens)"""
    import math
    from PIL import Image
    from omniparser_amd.florence import ocr_cells
    from omniparser_amd.pipeline import ScreenParser
    from omniparser_amd.util import utils as U
    model, proc = cmp_["model"], cmp_["processor"]
    table, _texts = proc.poly_class_table()
    R, (H, W) = model.resolution, img.shape[:2]
    got, stats = U.segment(img, cmp_, text=text, regions=regions, return_stats=True, **kw)
    again = U.segment(Image.fromarray(img), cmp_, text=text, regions=regions, **kw)
    assert len(again) == len(got) and all(np.array_equal(a["mask"], b["mask"]) and {k: v for k, v in a.items() if k != "mask"} ==
                                          {k: v for k, v in b.items() if k != "mask"} for a, b in zip(again, got))
    call = model.calls[-1]
    tiles = ScreenParser.tile_origins(W, H, R, R, kw.get("overlap", 128))[0]
    I = kw.get("instances", 4)
    # phrases: the cells of the frame's grid (every tile is a row); regions: every row owns the whole plane
    cells = ocr_cells(call["origins"], R) if text is not None else [[ox, oy, NEG, INF, NEG, INF] for ox, oy in call["origins"]]
    assert call["cells"] == cells and (text is None or sorted(set(call["origins"])) == sorted(tiles))
    raw = model.segment_regions(torch.from_numpy(img), call["origins"], call["prompts"], table, max_new_tokens=kw.get("max_new_tokens", 256), instances=64,
                                cells=cells)
    t_mask, _ = twin_masks(raw.records.numpy(), raw.rows.numpy(), raw.vertices.numpy(), cells, 64, H, W, R)
    want = []
    for r, (ox, oy) in enumerate(call["origins"]):
        flags = int(raw.rows[r, 2])
        assert stats[r]["fallback"] == bool(flags & 1) and stats[r]["tile"] == tiles.index((ox, oy))
        if flags & 1:
            insts = [([[v + (oy if q & 1 else ox) for q, v in enumerate(p)] for p in g["polygons"]], g["columns"])
                     for g in U.parse_polygon_answer(raw.ids[r].tolist(), proc, (R, R))]
        else:
            assert stats[r]["found"] == int(raw.rows[r, 1]) and stats[r]["kept"] == int(raw.rows[r, 3]) and stats[r]["polygons"] == int(raw.rows[r, 0])
            polys = device_polys(raw.records[r].numpy(), raw.vertices[r].numpy(), int(raw.rows[r, 0]), (0, 0))
            insts, k = [], 0
            for g in polys:
                cols = []
                for _p in g:
                    rec = raw.records[r, k].tolist()
                    cols += [j for j in range(rec[5], rec[6]) if table[int(raw.ids[r, j])] != STRIP][:2 * rec[4]]
                    k += 1
                insts.append((g, cols))
        for s, (g, cols) in enumerate(insts):
            xs, ys = [v for p in g for v in p[0::2]], [v for p in g for v in p[1::2]]
            if not xs or not U._owns(cells[r], [min(xs), min(ys), max(xs), max(ys)]):
                continue
            box = [min(xs), min(ys), max(xs), max(ys)]
            if flags & 1:
                full = np.zeros((R, R), bool)
                for p in g:
                    if len(p) >= 6:
                        full |= inside_polygon([(p[q] - ox, p[q + 1] - oy) for q in range(0, len(p), 2)], R)
                full &= ((np.arange(R) + oy < H) & (np.arange(R) + oy >= 0))[:, None] & ((np.arange(R) + ox < W) & (np.arange(R) + ox >= 0))[None, :]
            else:
                full = unpack(t_mask[r, s], R)
            mask = full[box[1] - oy:box[3] - oy, box[0] - ox:box[2] - ox]
            conf = math.exp(sum(float(raw.logp[r, j - 1]) for j in cols) / len(cols))
            want.append((stats[r]["index"], g, box, int(mask.sum()), conf, stats[r]["tile"], brute_point(mask, (box[0], box[1])), mask))
    assert len(got) == len(want), (len(got), len(want))
    for a, b in zip(got, want):
        assert (a["index"], a["polygons"], a["bbox"], a["area"], a["tile"], a["point"], a["mask_origin"]) == (*b[:4], b[5], b[6], (b[2][0], b[2][1])), (a, b[:7])
        assert abs(a["confidence"] - b[4]) <= 1e-6 * b[4] and 0.0 < a["confidence"] <= 1.0
        assert a["mask"].dtype == bool and np.array_equal(a["mask"], b[7])
        if a["point"] is not None:
            assert a["mask"][a["point"][1] - a["bbox"][1], a["point"][0] - a["bbox"][0]]
    assert all(g["mask"] is None for g in U.segment(img, cmp_, text=text, regions=regions, return_masks=False, **kw))
    strict = U.segment(img, cmp_, text=text, regions=regions, min_confidence=0.999999, **kw)
    assert all(g["confidence"] >= 0.999999 for g in strict) and len(strict) <= len(got)
    assert I == call["instances"]
    return got, stats


# ---------------------------------------------------------------------------------------------- captioner against transformers
SEG_PHRASE = "AB"                      # one <REFERRING_EXPRESSION_SEGMENTATION> phrase over the 6 tiles, then three <REGION_TO_SEGMENTATION> boxes
SEG_MAX_NEW = 48
SEG_SEED = 0                           # see `segment_reference` for what the oracle gives at it


def poly_suppress(vocab, keep=()):
    """suppress_tokens that leave only the location ids, <sep>, <poly>, </poly> and `keep` (bos, eos, forced tokens)"""
    allowed = set(range(LOC0, LOC0 + 1000)) | {SEP, POLY, PEND} | {int(k) for k in keep}
    return [t for t in range(vocab) if t not in allowed]


def caption_dir_with_poly_tokenizer(tmp_dir, eos_prone=False):
    """the stand-in caption checkpoint (or its EOS-prone twin) with the polygon tokenizer next to it"""
    import shutil
    import beam_checks as BC
    from tools.make_weights import ensure_caption_checkpoint
    src = BC.eos_prone_checkpoint(0) if eos_prone else ensure_caption_checkpoint(0)
    dst = Path(tmp_dir) / ("ckpt_poly_eos" if eos_prone else "ckpt_poly")
    if not (dst / "tokenizer.json").exists():
        dst.mkdir(parents=True, exist_ok=True)
        for f in ("model.safetensors", "config.json", "generation_config.json"):
            (dst / f).symlink_to((src / f).resolve())
        shutil.copy(write_poly_tokenizer(Path(tmp_dir) / "tok_poly_for_ckpt") / "tokenizer.json", dst / "tokenizer.json")
    return dst


def segment_reference(tmp_dir, eos_prone, seed=SEG_SEED, R=64, frame_whl=RC.OCR_FRAME, max_new=SEG_MAX_NEW):
    """transformers on the CPU for the 6 + 3 rows of the seeded frame: dict(img, tiles, origins, prompts, pix, suppress, seq, margins,
    logp [rows, T - 1], polys: per row the post-processor's instances (tile pixels), eos)

    What THE ORACLE ALONE gives at SEG_SEED with generation restricted to the location tokens, <sep>, <poly>, </poly> and EOS
    (transformers on the CPU, chosen and recorded before any device run; `check_segment_captioner` asserts it again), seeds scanned
    from 0:
      seed 0, stock checkpoint   every one of the 9 rows is 48 tokens long without an EOS and holds ONE instance of one polygon of 23
                                 vertices (the allowed set is 99.6 % location tokens: no <sep>, <poly> or </poly> is chosen); smallest
                                 top-1 / top-2 margin 4.2e-4, above gpu_checks.CAPTION_MARGIN: used
      EOS-prone checkpoint       the EOS token (13840) beats every allowed token at the first free step: 9 rows, no instance, 2 columns
                                 per row — the early exit after the first poll"""
    import beam_checks as BC
    import box_checks as BX
    import prompt_checks as P
    from omniparser_amd.pipeline import ScreenParser
    proc, post = oracle(tmp_dir)
    W, H, overlap = frame_whl
    img = RC.frame(W, H, seed)
    tiles = ScreenParser.tile_origins(W, H, R, R, overlap)[0]
    origins = list(tiles) + [tiles[t] for t in BX.DESCRIBE_TILES]
    prompts = [proc.segment_prompt_ids(RES, text=SEG_PHRASE)] * len(tiles)
    for b, (ox, oy) in zip(BX.DESCRIBE_BOXES, origins[len(tiles):]):
        clip = lambda v: min(max(v, 0), R)                  # noqa: E731
        prompts.append(proc.segment_prompt_ids(R2S, region=[clip(b[0] - ox), clip(b[1] - oy), clip(b[2] - ox), clip(b[3] - oy)], size=(R, R)))
    pix = RC.host_tiles(img, origins, R)
    model = BC.oracle_model(0, eos_prone)
    try:
        eos = model.generation_config.eos_token_id
        suppress = poly_suppress(model.config.get_text_config().vocab_size, keep=(BOS, EOS, eos))
        ids, mask = P.hf_inputs(model, R, prompts)
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
    polys = []
    for r in seq.tolist():
        end = next((j for j in range(1, len(r)) if r[j] == eos), len(r))
        known = [t for t in r[:end] if 0 <= t < 1403]           # (an id the synthetic tokenizer does not know cannot be rendered)
        polys.append(oracle_polys(post, known, R, eos=-1) if len(known) == end else None)
    return dict(img=img, tiles=tiles, origins=origins, prompts=prompts, pix=pix, suppress=suppress, seq=seq, margins=margins, logp=ts.float(), polys=polys, eos=eos)


def check_segment_captioner(tmp_dir, eos_prone, log=None):
    """util.utils.segment with the real captioner at R = 64 on the 150 x 100 frame: one phrase over the 6 tiles, then three boxes;
    48 new tokens, generation restricted to the location tokens, the three polygon tokens and EOS.  The rows `segment` decodes are
    token-exact against transformers on the CPU (margins asserted first), the polygons are the post-processor's on transformers'
    ids plus the tile's origin, the masks are the twin's on those polygons, the mean log-probability per instance lies within
    RC.TOL_LOGP of compute_transition_scores"""
    import math
    import os
    import box_checks as BX
    import prompt_checks as P
    from omniparser_amd.florence import ocr_cells
    from omniparser_amd.util import utils as U
    ref = segment_reference(tmp_dir, eos_prone)
    W, H, overlap = RC.OCR_FRAME
    R, n_t = 64, len(ref["tiles"])
    best = max((len(p) // 2 for row in ref["polys"] for g in row for p in g), default=0)
    if eos_prone:
        assert all(row == [] for row in ref["polys"]), ref["polys"]
    else:
        assert best >= 3, ref["polys"]
    finite = [m for m in ref["margins"] if m != float("inf")]
    if finite:
        P.assert_margins(finite, f"polygon answers eos_prone={eos_prone}")
    os.environ["OMNI_CAPTION_RES"] = "64"
    try:
        cmp_ = U.get_caption_model_processor("florence2", str(caption_dir_with_poly_tokenizer(tmp_dir, eos_prone)), "cuda")
    finally:
        os.environ.pop("OMNI_CAPTION_RES", None)
    model = cmp_["model"]
    # a prompt ends in the TOKENIZER's </s> (2), as transformers' processor writes it, whatever token the checkpoint's generation
    # config ends an answer with (13840 in the EOS-prone one): the processor is the oracle's, over the same tokenizer file
    cmp_["processor"] = oracle(tmp_dir)[0]
    calls, real = [], model.segment_regions

    def spy(image_u8, origins, prompts, class_table, **kw):
        out = real(image_u8, origins, prompts, class_table, **kw)
        calls.append((list(origins), [list(p) for p in prompts], out))
        return out
    model.segment_regions = spy
    gen = {"suppress_tokens": ref["suppress"]}
    kw = dict(max_new_tokens=SEG_MAX_NEW, overlap=overlap, generation=gen)
    try:
        by_text = U.segment(ref["img"], cmp_, text=SEG_PHRASE, **kw)
        steps_text = model.last_steps
        by_box = U.segment(ref["img"], cmp_, regions=[list(b) for b in BX.DESCRIBE_BOXES], **kw)
    finally:
        del model.segment_regions
    assert len(calls) == 2 and calls[0][0] == ref["origins"][:n_t] and calls[1][0] == ref["origins"][n_t:]
    assert calls[0][1] == ref["prompts"][:n_t] and calls[1][1] == ref["prompts"][n_t:]
    worst, want_all = 0.0, []
    for c, (origins, _prompts, out) in enumerate(calls):
        base = c * n_t
        cells = ocr_cells(origins, R) if c == 0 else [[ox, oy, NEG, INF, NEG, INF] for ox, oy in origins]
        rec, rows, verts = out.records.numpy(), out.rows.numpy(), out.vertices.numpy()
        t_mask, t_cnt = twin_masks(rec, rows, verts, cells, 4, H, W, R)
        assert np.array_equal(out.masks.numpy().view(np.uint32), t_mask) and np.array_equal(out.counts.numpy(), t_cnt)
        for r, (ox, oy) in enumerate(origins):
            assert P._trim(out.ids[r]) == P._trim(ref["seq"][base + r]), (base + r, out.ids[r].tolist(), ref["seq"][base + r].tolist())
            flags = int(rows[r, 2])
            assert flags in (0, 2), (base + r, flags)
            got = device_polys(rec[r], verts[r], int(rows[r, 0]), (ox, oy))
            assert got == ref["polys"][base + r], (base + r, got, ref["polys"][base + r])
            k = 0
            for s, g in enumerate(got):
                cols = []
                for _p in g:
                    cols += list(range(int(rec[r, k, 5]), int(rec[r, k, 5]) + 2 * int(rec[r, k, 4])))     # no STRIP token can be generated
                    k += 1
                if not cols:
                    continue
                want = float(sum(float(ref["logp"][base + r, j - 1]) for j in cols)) / len(cols)
                have = float(sum(float(out.sums[r, q]) for q in range(int(rows[r, 0])) if rec[r, q, 1] == s)) / len(cols)
                worst = max(worst, abs(want - have))
                if rec[r, k - 1, 8]:
                    frame_polys = [[v + (oy if q & 1 else ox) for q, v in enumerate(p)] for p in g]
                    want_all.append((c, frame_polys, math.exp(have), int(t_cnt[r, s].sum()) if s < 4 else None))
    got_all = [(0, g["polygons"], g["confidence"], g["area"]) for g in by_text] + [(1, g["polygons"], g["confidence"], g["area"]) for g in by_box]
    assert len(got_all) == len(want_all)
    for a, b in zip(got_all, want_all):
        assert a[:2] == b[:2] and abs(a[2] - b[2]) <= 1e-6 and (b[3] is None or a[3] == b[3]), (a, b)
    line = (f"segment eos_prone={eos_prone}: most vertices in a polygon {best}, instances returned {len(got_all)}, steps {steps_text} / {model.last_steps}, "
            f"max |d mean logp| = {worst:.3e} (bound {RC.TOL_LOGP:.2e})")
    print(line)
    if log is not None:
        log.append(line)
    assert worst <= RC.TOL_LOGP, worst
    if eos_prone:
        assert not got_all and steps_text < SEG_MAX_NEW and model.last_steps < SEG_MAX_NEW
    return by_text, by_box

"""Drop-in for the hot half of ref:util/utils.py on MI355X.

Same names, arguments and return values as the reference for the functions on the detect -> caption
path: `get_yolo_model`, `get_caption_model_processor`, `predict_yolo`,
`int_box_area`, `remove_overlap_new`, `get_parsed_content_icon`, `get_som_labeled_img`,
`check_ocr_box` (pass-through: OCR models are out of scope, SURVEY 2.1 #2b).  The two model stages run
as HIP plans (util/yolov9.py, florence.py); the glue between them reproduces the reference's list
semantics (App. E of SURVEY.md) and is pinned by golden fixtures generated from the reference's own
source under dependency shims (tests/golden/).
"""
import base64
import contextlib
import io
import os
import time
from pathlib import Path
from typing import List, Optional, Union

import numpy as np
import torch
from PIL import Image

from .. import _lib as L
from ..florence import CLIP_MEAN, CLIP_STD, PROMPT_IDS, Florence2Captioner
from .yolov9 import YOLOv9Detector


# ------------------------------------------------------------------------------------------ loaders
def get_yolo_model(model_path=None, device=None):
    """ref:util/utils.py:72-85 — local weights/icon_detect_v3/model.pt if present, YOLOv9-E adapter."""
    if model_path is None:
        local = Path(__file__).resolve().parents[2] / "weights/icon_detect_v3/model.pt"
        if local.is_file():
            model_path = local
    if model_path is None or "icon_detect_v3" in Path(model_path).parts:
        return YOLOv9Detector(model_path=model_path, device=device)
    raise NotImplementedError("only the YOLOv9-E icon_detect_v3 detector is implemented on MI355X "
                              "(the Ultralytics fallback of ref:util/utils.py:83-85 is out of scope)")


class _Batch(dict):
    """Minimal BatchFeature: mapping with `.to(device=, dtype=)` (ref:util/utils.py:121-123)."""

    def to(self, device=None, dtype=None, **kw):
        out = _Batch()
        for k, v in self.items():
            if isinstance(v, torch.Tensor):
                if dtype is not None and v.is_floating_point():
                    v = v.to(dtype)
                if device is not None:
                    v = v.to(device)
            out[k] = v
        return out

    __getattr__ = dict.get


# Florence-2 task tokens that take no input -> the sentence the model was trained on (hf:models/florence2/processing_florence2.py,
# `task_prompts_without_inputs`; restated, and compared with the installed transformers by the tests)
TASK_PROMPTS = {
    "<OCR>": "What is the text in the image?",
    "<OCR_WITH_REGION>": "What is the text in the image, with regions?",
    "<CAPTION>": "What does the image describe?",
    "<DETAILED_CAPTION>": "Describe in detail what is shown in the image.",
    "<MORE_DETAILED_CAPTION>": "Describe with a paragraph what is shown in the image.",
    "<OD>": "Locate the objects with category name in the image.",
    "<DENSE_REGION_CAPTION>": "Locate the objects in the image, with their descriptions.",
    "<REGION_PROPOSAL>": "Locate the region proposals in the image.",
}
# task tokens whose sentence embeds an {input}: `prompt_ids` refuses them (it has no input to put in); `task_prompt_ids` builds them
TASK_PROMPTS_WITH_INPUT = {
    "<CAPTION_TO_PHRASE_GROUNDING>": "Locate the phrases in the caption: {input}",
    "<OPEN_VOCABULARY_DETECTION>": "Locate {input} in the image.",
    "<REGION_TO_CATEGORY>": "What is the region {input}?",
    "<REGION_TO_DESCRIPTION>": "What does the region {input} describe?",
    "<REGION_TO_OCR>": "What text is in the region {input}?",
}
SEGMENT_PROMPTS = {                                     # the two tasks that answer in polygons: `segment_prompt_ids`, `segment`
    "<REFERRING_EXPRESSION_SEGMENTATION>": "Locate {input} in the image with mask",
    "<REGION_TO_SEGMENTATION>": "What is the polygon mask of region {input}",
}
TASKS_WITH_REGION = ("<REGION_TO_CATEGORY>", "<REGION_TO_DESCRIPTION>", "<REGION_TO_OCR>")
TASKS_WITH_INPUT = ("<CAPTION_TO_PHRASE_GROUNDING>", "<REFERRING_EXPRESSION_SEGMENTATION>", "<REGION_TO_SEGMENTATION>",
                    "<OPEN_VOCABULARY_DETECTION>", "<REGION_TO_CATEGORY>", "<REGION_TO_DESCRIPTION>", "<REGION_TO_OCR>")


class FlorenceProcessor:
    """Stand-in for AutoProcessor("microsoft/Florence-2-base") on the caption path
    (hf:models/florence2/processing_florence2.py:84-152 + CLIP image processor).  Tokenizer files are
    not shipped with the reference; if `tokenizer.json` sits next to the checkpoint it is used for
    `batch_decode` and for prompts other than `<CAPTION>`, otherwise token ids are rendered as text and only the
    default prompt exists."""

    def __init__(self, model_dir=None, image_token_id=51289, special_ids=(0, 1, 2, 3)):
        """special_ids: bos / pad / eos / unk of the checkpoint (Florence2Captioner passes what generation_config.json says) — used
        only WITHOUT a tokenizer.json; with one, the special ids are the tokens that file flags `special` (what
        `batch_decode(skip_special_tokens=True)` of the reference's AutoProcessor skips, ref:util/utils.py:128)."""
        self.image_token_id = image_token_id
        self.tok = None
        self.model_dir = model_dir
        sp = [int(i) for i in special_ids]
        self.bos_id, self.pad_id, self.eos_id = sp[0], sp[1], sp[2]
        self.special = set(int(i) for i in special_ids) | {int(image_token_id)}
        if model_dir is not None and (Path(model_dir) / "tokenizer.json").exists():
            import json as _json
            from tokenizers import Tokenizer
            path = Path(model_dir) / "tokenizer.json"
            self.tok = Tokenizer.from_file(str(path))
            added = _json.loads(path.read_text()).get("added_tokens", [])
            self.special = {int(t["id"]) for t in added if t.get("special")} | {int(image_token_id)}
            self.vocab_size = self.tok.get_vocab_size(with_added_tokens=True)

    def __call__(self, images=None, text=None, return_tensors="pt", do_resize=True, **kw):
        imgs = images if isinstance(images, (list, tuple)) else [images]
        arrs = []
        for im in imgs:
            if do_resize:
                im = im.convert("RGB").resize((768, 768), Image.Resampling.BICUBIC)
            a = (np.asarray(im.convert("RGB")).astype(np.float64) * (1 / 255)).astype(np.float32)
            a = (a - np.asarray(CLIP_MEAN, dtype=np.float32)) / np.asarray(CLIP_STD, dtype=np.float32)
            arrs.append(torch.from_numpy(a.transpose(2, 0, 1).copy()))
        pix = torch.stack(arrs)
        n_img = (pix.shape[-1] // 32) ** 2 + 1
        if isinstance(text, (list, tuple)):
            if len(text) != len(imgs):
                raise ValueError(f"{len(text)} prompts for {len(imgs)} images")
            rows = [self.prompt_ids(t) for t in text]
        else:
            rows = [self.prompt_ids(text)] * len(imgs)
        T = max(len(r) for r in rows)                      # unequal prompts: right-padded, with the matching attention mask
        ids = torch.tensor([[self.image_token_id] * n_img + r + [self.pad_id] * (T - len(r)) for r in rows])
        mask = torch.tensor([[1] * (n_img + len(r)) + [0] * (T - len(r)) for r in rows])
        return _Batch(input_ids=ids, pixel_values=pix, attention_mask=mask)

    def prompt_ids(self, text=None):
        """token ids (bos ... eos) of one prompt.  None and "<CAPTION>" are PROMPT_IDS, with or without a tokenizer.  The other
        Florence-2 task tokens without an input stand for their task sentences (TASK_PROMPTS), any other string is tokenised as
        it is: both need the `tokenizer.json` next to the checkpoint (ValueError naming the file when it is missing).  Task tokens
        that need an {input} are a ValueError."""
        if text is None or text == "<CAPTION>":
            return list(PROMPT_IDS)
        if not isinstance(text, str):
            raise ValueError(f"a prompt is a string (got {type(text).__name__})")
        for tk in TASKS_WITH_INPUT:
            if tk in text:
                raise ValueError(f"task {tk} needs an input and answers in location tokens: not supported by this captioner")
        for tk, sentence in TASK_PROMPTS.items():
            if tk in text:
                if text != tk:
                    raise ValueError(f"Task token {tk} should be the only content in the prompt.")
                text = sentence
                break
        if self.tok is None:
            where = Path(self.model_dir) / "tokenizer.json" if self.model_dir is not None else "tokenizer.json (no model directory was given)"
            raise ValueError(f"the prompt {text!r} needs a tokenizer: {where} is missing (only the default <CAPTION> prompt works without it)")
        return [self.bos_id] + list(self.tok.encode(text, add_special_tokens=False).ids) + [self.eos_id]

    @staticmethod
    def quantize_box(box, size):
        """location bins [x0, y0, x1, y1] of a box in pixels of an image of `size` (width, height): transformers'
        Florence2PostProcessor.quantize on an f32 tensor — floor(f32(v) / f32(size / 1000)) in f32 arithmetic, clamped to 0..999.
        (Not v * 1000 // size: f32(0.064) lies above 0.064, so 8 px of 64 fall into bin 124, not 125.)"""
        w, h = size
        per = (np.float32(w / 1000), np.float32(h / 1000))
        return [int(min(max(np.floor(np.float32(v) / per[k & 1]), 0), 999)) for k, v in enumerate(box)]

    def task_prompt_ids(self, task, text=None, region=None, size=None):
        """token ids (bos ... eos) of the prompt of a Florence-2 task WITH an input, the sentence transformers' processor builds
        (`_construct_prompts`: the input stripped and put into the task's sentence, TASK_PROMPTS_WITH_INPUT):
        <OPEN_VOCABULARY_DETECTION> and <CAPTION_TO_PHRASE_GROUNDING> take `text`; <REGION_TO_CATEGORY>, <REGION_TO_DESCRIPTION> and
        <REGION_TO_OCR> take `region`, a box [x0, y0, x1, y1] in pixels of an image of `size` (width, height), written as the four
        location tokens `quantize_box` gives.  Needs the tokenizer.json next to the checkpoint.  ValueError: another task (the
        polygon tasks included), the wrong kind of input for the task, no tokenizer."""
        if task not in TASK_PROMPTS_WITH_INPUT:
            raise ValueError(f"task {task!r} is not a task with an input this captioner supports ({', '.join(TASK_PROMPTS_WITH_INPUT)})")
        if task in TASKS_WITH_REGION:
            if text is not None or region is None or size is None:
                raise ValueError(f"task {task} takes a region (box in pixels) and the size of its image, no text")
            box = [float(v) for v in region]
            if len(box) != 4 or len(tuple(size)) != 2 or min(size) <= 0:
                raise ValueError("a region is [x0, y0, x1, y1] in pixels of an image of size (width, height)")
            given = "".join(f"<loc_{b}>" for b in self.quantize_box(box, size))
        else:
            if not isinstance(text, str) or region is not None:
                raise ValueError(f"task {task} takes a text, no region")
            given = text.replace(task, "").strip()
        sentence = TASK_PROMPTS_WITH_INPUT[task].format(input=given)
        if self.tok is None:
            where = Path(self.model_dir) / "tokenizer.json" if self.model_dir is not None else "tokenizer.json (no model directory was given)"
            raise ValueError(f"the prompt {sentence!r} needs a tokenizer: {where} is missing")
        return [self.bos_id] + list(self.tok.encode(sentence, add_special_tokens=False).ids) + [self.eos_id]

    def loc_class_table(self):
        """(class table u16 [vocab] as numpy, per-token texts) for OMNI_OP_REGION_OCR and `parse_ocr_regions`, built once from the
        tokenizer.json: a token's class is its location bin 0..999 (`<loc_N>`), L.OCR_CLASS_STRIP (`<s>`, `</s>`, `<pad>`, which
        transformers deletes from the text before it matches), L.OCR_CLASS_TEXT, or L.OCR_CLASS_HARD when its text is empty or holds
        a newline or '<' — the cases in which matching tokens and matching the decoded text can differ.  A token's text is what
        transformers' `Florence2PostProcessor.decode_with_spans` gives it: the token itself when it is special, else the decoder's
        rendering of that ONE token (not of the sequence).  ValueError: no tokenizer.json (naming the file), or a tokenizer whose
        `<loc_0>` .. `<loc_999>` are not 1000 ascending contiguous ids."""
        if getattr(self, "_loc", None) is not None:
            return self._loc
        if self.tok is None:
            where = Path(self.model_dir) / "tokenizer.json" if self.model_dir is not None else "tokenizer.json (no model directory was given)"
            raise ValueError(f"reading text regions needs a tokenizer with <loc_0>..<loc_999>: {where} is missing")
        base = self.tok.token_to_id("<loc_0>")
        if base is None or any(self.tok.token_to_id(f"<loc_{k}>") != base + k for k in range(1000)):
            raise ValueError(f"{Path(self.model_dir) / 'tokenizer.json'}: <loc_0>..<loc_999> must be 1000 contiguous ascending token ids "
                             "(the tokenizer of a Florence-2 checkpoint)")
        n, dec = self.vocab_size, self.tok.decoder
        table = np.full((n,), L.OCR_CLASS_HARD, dtype=np.uint16)
        texts = [""] * n
        for t in range(n):
            tok = self.tok.id_to_token(t)
            if tok is None:
                continue
            if tok in ("<s>", "</s>", "<pad>"):
                table[t], texts[t] = L.OCR_CLASS_STRIP, tok
                continue
            texts[t] = tok if (t in self.special or dec is None) else dec.decode([tok])
            if base <= t < base + 1000:
                table[t] = t - base
            elif texts[t] and "\n" not in texts[t] and "<" not in texts[t]:
                table[t] = L.OCR_CLASS_TEXT
        self._loc = (table, texts)
        return self._loc

    def poly_class_table(self):
        """(class table u16 [vocab], per-token texts) for OMNI_OP_REGION_OCR mode 5 and `parse_polygon_answer`: `loc_class_table`'s
        with `<sep>`, `<poly>` and `</poly>` re-classed L.OCR_CLASS_SEP / _POLY / _POLY_END (there they are HARD: they hold '<'), the same
        texts.  ValueError naming the tokenizer file when one of the three is missing."""
        if getattr(self, "_poly", None) is not None:
            return self._poly
        table, texts = self.loc_class_table()
        table = table.copy()
        for tok, c in (("<sep>", L.OCR_CLASS_SEP), ("<poly>", L.OCR_CLASS_POLY), ("</poly>", L.OCR_CLASS_POLY_END)):
            t = self.tok.token_to_id(tok)
            if t is None or not 0 <= t < len(table):
                raise ValueError(f"{Path(self.model_dir) / 'tokenizer.json'}: the polygon token {tok} is missing (the tokenizer of a Florence-2 "
                                 "checkpoint has <sep>, <poly> and </poly>)")
            table[t] = c
        self._poly = (table, texts)
        return self._poly

    def segment_prompt_ids(self, task, text=None, region=None, size=None):
        """token ids (bos ... eos) of the prompt of a segmentation task, the sentence transformers' `_construct_prompts` builds:
        <REFERRING_EXPRESSION_SEGMENTATION> takes `text`, <REGION_TO_SEGMENTATION> a `region` [x0, y0, x1, y1] in pixels of an image of
        `size` (width, height), written as the four location tokens `quantize_box` gives.  ValueError: another task, the wrong kind of
        input, no tokenizer.  (`task_prompt_ids` keeps refusing both tasks: their answers need `segment`, not `locate`.)"""
        if task not in SEGMENT_PROMPTS:
            raise ValueError(f"task {task!r} is not a segmentation task ({', '.join(SEGMENT_PROMPTS)})")
        if task == "<REGION_TO_SEGMENTATION>":
            if text is not None or region is None or size is None:
                raise ValueError(f"task {task} takes a region (box in pixels) and the size of its image, no text")
            box = [float(v) for v in region]
            if len(box) != 4 or len(tuple(size)) != 2 or min(size) <= 0:
                raise ValueError("a region is [x0, y0, x1, y1] in pixels of an image of size (width, height)")
            given = "".join(f"<loc_{b}>" for b in self.quantize_box(box, size))
        else:
            if not isinstance(text, str) or region is not None:
                raise ValueError(f"task {task} takes a text, no region")
            given = text.replace(task, "").strip()
        sentence = SEGMENT_PROMPTS[task].format(input=given)
        if self.tok is None:
            where = Path(self.model_dir) / "tokenizer.json" if self.model_dir is not None else "tokenizer.json (no model directory was given)"
            raise ValueError(f"the prompt {sentence!r} needs a tokenizer: {where} is missing")
        return [self.bos_id] + list(self.tok.encode(sentence, add_special_tokens=False).ids) + [self.eos_id]

    def batch_decode(self, ids, skip_special_tokens=True):
        special = self.special
        out = []
        for row in ids.tolist():
            toks = [t for t in row if not (skip_special_tokens and t in special)]
            if self.tok is not None:
                toks = [t for t in toks if 0 <= t < self.vocab_size]          # an id the tokenizer does not know (the image placeholder of another export)
                out.append(self.tok.decode(toks, skip_special_tokens=skip_special_tokens))
            else:
                out.append(" ".join(f"tok{t}" for t in toks))
        return out


def get_caption_model_processor(model_name, model_name_or_path="Salesforce/blip2-opt-2.7b", device=None):
    """ref:util/utils.py:48-69 for model_name == 'florence2' (BLIP-2 / phi3v are legacy, out of scope)."""
    if not device:
        device = "cuda" if torch.cuda.is_available() else "cpu"
    if model_name != "florence2":
        raise NotImplementedError(f"caption model '{model_name}': only 'florence2' is implemented on MI355X")
    model = Florence2Captioner(model_name_or_path, device)
    w = model.w
    processor = FlorenceProcessor(model_name_or_path, image_token_id=w.cfg.get("image_token_id", 51289),
                                  special_ids=(w.bos, w.pad, w.eos, w.cfg.get("text_config", {}).get("unk_token_id", 3)))
    return {"model": model, "processor": processor}


def get_xywh(input):
    """ref:util/utils.py:498-501 (quad corners -> truncated x, y, w, h)."""
    x, y, w, h = input[0][0], input[0][1], input[2][0] - input[0][0], input[2][1] - input[0][1]
    return int(x), int(y), int(w), int(h)


def get_xyxy(input):
    """ref:util/utils.py:503-506."""
    x, y, xp, yp = input[0][0], input[0][1], input[2][0], input[2][1]
    return int(x), int(y), int(xp), int(yp)


_OCR_ENGINES = {"easyocr": None, "paddleocr": None}      # process-wide engines, created on first use (the reference builds both at import)


def set_ocr_engine(easyocr_reader=None, paddle_ocr=None):
    """Install the OCR engine objects `check_ocr_box` calls: an EasyOCR-compatible `reader.readtext(image_np, **easyocr_args)` ->
    [(quad, text, conf)] and/or a PaddleOCR-compatible `ocr(image_np, cls=False)` -> [[[quad, (text, conf)], ...]]."""
    if easyocr_reader is not None:
        _OCR_ENGINES["easyocr"] = easyocr_reader
    if paddle_ocr is not None:
        _OCR_ENGINES["paddleocr"] = paddle_ocr


def _ocr_engine(kind):
    if _OCR_ENGINES[kind] is None:
        try:
            if kind == "easyocr":
                import easyocr
                _OCR_ENGINES[kind] = easyocr.Reader(["en"])                                  # ref:util/utils.py:21
            else:
                from paddleocr import PaddleOCR
                _OCR_ENGINES[kind] = PaddleOCR(lang="en", use_angle_cls=False, use_gpu=False, show_log=False, max_batch_size=1024,
                                               use_dilation=True, det_db_score_mode="slow", rec_batch_num=1024)   # ref:util/utils.py:22-30
        except ImportError:
            return None
    return _OCR_ENGINES[kind]


def check_ocr_box(image_source, display_img=True, output_bb_format="xywh", goal_filtering=None, easyocr_args=None,
                  use_paddleocr=False, ocr_result=None):
    """ref:util/utils.py:514-549 — the OCR front-end of every caller (`Omniparser.parse`, the Gradio demo).

    Everything the reference does AROUND its OCR engine is reproduced (fixture: tests/golden/reference_ocr_glue.json, recorded
    from the reference's own function): RGBA -> RGB, PaddleOCR's strict `> text_threshold` filter (default 0.5), `easyocr_args`
    handed to `readtext` untouched, int() truncation of the quad corners, xywh / xyxy output, and display_img=True always
    yielding xywh.  The engines themselves (EasyOCR = CRAFT + CRNN, PaddleOCR = PP-OCR) are third-party model packages that
    are not part of this path: they are used when importable or installed with `set_ocr_engine`; `ocr_result=(texts, xyxy
    boxes)` feeds precomputed OCR through the same formatting; with neither, the frame simply has no text boxes."""
    if isinstance(image_source, str):
        image_source = Image.open(image_source)
    if image_source.mode == "RGBA":
        image_source = image_source.convert("RGB")
    if ocr_result is not None:
        texts, boxes = ocr_result
        coord = [[[b[0], b[1]], [b[2], b[1]], [b[2], b[3]], [b[0], b[3]]] for b in boxes]
        text = list(texts)
    elif use_paddleocr:
        text_threshold = 0.5 if easyocr_args is None else easyocr_args["text_threshold"]
        engine = _ocr_engine("paddleocr")
        result = engine.ocr(np.array(image_source), cls=False)[0] if engine is not None else []
        coord = [item[0] for item in result if item[1][1] > text_threshold]
        text = [item[1][0] for item in result if item[1][1] > text_threshold]
    else:
        engine = _ocr_engine("easyocr")
        result = engine.readtext(np.array(image_source), **(easyocr_args or {})) if engine is not None else []
        coord = [item[0] for item in result]
        text = [item[1] for item in result]
    if display_img or output_bb_format == "xywh":        # the reference's display branch draws and keeps xywh
        bb = [get_xywh(item) for item in coord]
    elif output_bb_format == "xyxy":
        bb = [get_xyxy(item) for item in coord]
    else:
        raise UnboundLocalError(f"output_bb_format must be 'xywh' or 'xyxy', got {output_bb_format!r}")   # the reference leaves `bb` unbound
    return (text, bb), goal_filtering


# ------------------------------------------------------------------------------------------ glue (App. E)
def predict_yolo(model, image, box_threshold, imgsz, scale_img, iou_threshold=0.7):
    """ref:util/utils.py:388-409."""
    if scale_img:
        result = model.predict(source=image, conf=box_threshold, imgsz=imgsz, iou=iou_threshold)
    else:
        result = model.predict(source=image, conf=box_threshold, iou=iou_threshold)
    boxes = result[0].boxes.xyxy
    conf = result[0].boxes.conf
    phrases = [str(i) for i in range(len(boxes))]
    return boxes, conf, phrases


def int_box_area(box, w, h):
    """ref:util/utils.py:411-415."""
    x1, y1, x2, y2 = box
    ib = [int(x1 * w), int(y1 * h), int(x2 * w), int(y2 * h)]
    return (ib[2] - ib[0]) * (ib[3] - ib[1])


def _area(b):
    return (b[2] - b[0]) * (b[3] - b[1])


def _inter(a, b):
    return max(0, min(a[2], b[2]) - max(a[0], b[0])) * max(0, min(a[3], b[3]) - max(a[1], b[1]))


def _overlap(a, b):
    """the reference's IoU(): max(IoU with +1e-6 in the union, inter/areaA, inter/areaB)."""
    it = _inter(a, b)
    aa, ab = _area(a), _area(b)
    r1, r2 = (it / aa, it / ab) if (aa > 0 and ab > 0) else (0, 0)
    return max(it / (aa + ab - it + 1e-6), r1, r2)


def _inside(a, b):
    return _inter(a, b) / _area(a) > 0.80


def _remove_overlap_new_simple(boxes, iou_threshold, ocr_bbox=None):
    """Straightforward restatement of ref:util/utils.py:241-319 (kept as the cross-check of the vectorised
    version below; O(K^2 + K*M) Python)."""
    assert ocr_bbox is None or isinstance(ocr_bbox, list)
    out = list(ocr_bbox) if ocr_bbox else []
    bb = [e["bbox"] for e in boxes]
    for i, elem in enumerate(boxes):
        b1 = bb[i]
        a1 = _area(b1)
        if any(i != j and _overlap(b1, b2) > iou_threshold and a1 > _area(b2) for j, b2 in enumerate(bb)):
            continue
        if not ocr_bbox:
            out.append(b1)          # reference appends the bare box when there is no OCR list
            continue
        labels = ""
        swallowed = False
        for t in ocr_bbox:
            if _inside(t["bbox"], b1):
                labels += t["content"] + " "
                try:
                    out.remove(t)
                except ValueError:
                    pass
            elif _inside(b1, t["bbox"]):
                swallowed = True
                break
        if not swallowed:
            out.append({"type": "icon", "bbox": elem["bbox"], "interactivity": True,
                        "content": labels if labels else None,
                        "source": "box_yolo_content_ocr" if labels else "box_yolo_content_yolo"})
    return out


def _pair_inter(a, b):
    """f64 intersection areas [len(a), len(b)] with the reference's operation order."""
    iw = np.minimum(a[:, None, 2], b[None, :, 2]) - np.maximum(a[:, None, 0], b[None, :, 0])
    ih = np.minimum(a[:, None, 3], b[None, :, 3]) - np.maximum(a[:, None, 1], b[None, :, 1])
    return np.maximum(0, iw) * np.maximum(0, ih)


def remove_overlap_new(boxes, iou_threshold, ocr_bbox=None):
    """ref:util/utils.py:241-319 — same outputs and list-mutation quirks, vectorised (numpy f64 = the
    reference's Python-float arithmetic, same operation order) so the detect -> caption hand-off costs
    ~1 ms instead of ~100 ms of interpreter time at 300 boxes.

    An icon is dropped when some other icon overlaps it above the threshold and is smaller; OCR boxes
    lying inside a kept icon donate their text to it and are removed from the output (first dict-equal
    entry; a failed removal still donates the text); an icon lying inside an OCR box is dropped."""
    assert ocr_bbox is None or isinstance(ocr_bbox, list)
    out = list(ocr_bbox) if ocr_bbox else []
    n = len(boxes)
    if n == 0:
        return out
    bb = np.asarray([e["bbox"] for e in boxes], dtype=np.float64).reshape(n, 4)
    area = (bb[:, 2] - bb[:, 0]) * (bb[:, 3] - bb[:, 1])
    inter = _pair_inter(bb, bb)
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = inter / (area[:, None] + area[None, :] - inter + 1e-6)
        pos = (area[:, None] > 0) & (area[None, :] > 0)
        r1 = np.where(pos, inter / area[:, None], 0.0)
        r2 = np.where(pos, inter / area[None, :], 0.0)
    ov = np.maximum(np.maximum(iou, r1), r2)
    bad = (ov > iou_threshold) & (area[:, None] > area[None, :])
    np.fill_diagonal(bad, False)
    valid = ~bad.any(1)
    if not ocr_bbox:
        out.extend(boxes[i]["bbox"] for i in range(n) if valid[i])   # reference appends bare boxes without an OCR list
        return out
    m = len(ocr_bbox)
    ob = np.asarray([t["bbox"] for t in ocr_bbox], dtype=np.float64).reshape(m, 4)
    oarea = (ob[:, 2] - ob[:, 0]) * (ob[:, 3] - ob[:, 1])
    io = _pair_inter(bb, ob)                                     # [icons, ocr]
    ocr_in_icon = io / oarea[None, :] > 0.80                     # ZeroDivisionError in the reference <-> inf/nan here: never hit (int area > 0)
    icon_in_ocr = io / area[:, None] > 0.80
    # removal bookkeeping: `list.remove(x)` deletes the first remaining dict-equal entry
    key = [(tuple(t["bbox"]), t["content"], t["type"], t["interactivity"], t.get("source")) for t in ocr_bbox]
    alive = [True] * m
    members = {}
    for t_i, k in enumerate(key):
        members.setdefault(k, []).append(t_i)
    appended = []
    for i in np.nonzero(valid)[0]:
        stop = np.nonzero(~ocr_in_icon[i] & icon_in_ocr[i])[0]
        upto = stop[0] if len(stop) else m
        donors = np.nonzero(ocr_in_icon[i, :upto])[0]
        labels = ""
        for t_i in donors:
            labels += ocr_bbox[t_i]["content"] + " "
            for cand in members[key[t_i]]:
                if alive[cand]:
                    alive[cand] = False
                    break
        if len(stop):
            continue
        appended.append({"type": "icon", "bbox": boxes[i]["bbox"], "interactivity": True,
                         "content": labels if labels else None,
                         "source": "box_yolo_content_ocr" if labels else "box_yolo_content_yolo"})
    return [t for t_i, t in enumerate(ocr_bbox) if alive[t_i]] + appended


def crop_boxes_px(ratio_boxes, W, H):
    """Integer crop rectangles exactly as ref:util/utils.py:95-102 cuts them: `int(coord[k] * side)` there multiplies an element
    of an f32 TENSOR by a Python int — an f32 product, then truncation (NOT Python-float arithmetic: 100/1920 * 1920 is 100 in
    f32 and 99.99999 in f64).  Empty crops make cv2.resize raise and are skipped by the reference's bare `except`; numpy slicing
    clips the far edge at the image border.  Fixture: tests/golden/reference_glue.json::crop_shapes."""
    out = []
    fw, fh = np.float32(W), np.float32(H)
    for c in ratio_boxes:
        x0, x1 = int(np.float32(c[0]) * fw), int(np.float32(c[2]) * fw)
        y0, y1 = int(np.float32(c[1]) * fh), int(np.float32(c[3]) * fh)
        if x1 - x0 <= 0 or y1 - y0 <= 0 or x0 < 0 or y0 < 0:
            continue
        out.append([x0, y0, min(x1, W), min(y1, H)])
    return out


@torch.inference_mode()
def get_parsed_content_icon(filtered_boxes, starting_idx, image_source, caption_model_processor, prompt=None, batch_size=128,
                            return_confidence=False, max_new_tokens=None, generation=None, vocabulary=None):
    """ref:util/utils.py:88-132.  Crops are cut/resized/normalised on device and captioned by the HIP
    captioner; `image_source` may be the uint8 HWC numpy image (as in the reference) or a device tensor.
    prompt: the caption prompt of every crop, as the reference's (a Florence-2 task token or free text,
    `FlorenceProcessor.prompt_ids`); None = `<CAPTION>`.
    return_confidence: (caption, confidence) pairs instead of captions — `florence.caption_confidence` of the greedy tokens'
    log-probabilities, which the captioner then computes next to its arg-max (`caption_crops(return_scores=True)`).
    max_new_tokens: tokens generated per crop; None = 20, the reference's call.  With a prompt that asks for more than a label
    (`<DETAILED_CAPTION>`, free text) a larger value gives per-icon descriptions; the captioner validates it.
    generation: a dict of generation controls (repetition_penalty, no_repeat_ngram_size, min_new_tokens, suppress_tokens,
    begin_suppress_tokens, bad_words_ids; `Florence2Captioner.generate`) handed to `caption_crops(controls=...)`; None = the call
    as it was.
    vocabulary: a closed set of captions — a list of strings (tokenised by the processor's `prompt_ids`: they need the tokenizer.json
    next to the checkpoint, ValueError without it) or of token id lists ([forced BOS] text EOS; always work), handed to
    `caption_crops(vocabulary=...)`: every caption is then exactly one of them (a string entry comes back as it was given), chosen
    by ONE greedy decode however many there are, and the confidence is `caption_confidence` of the constrained log-probabilities.
    With max_new_tokens=None the longest label is generated in full even beyond 20 tokens.  Not together with `generation`.  None =
    the call as it was."""
    model, processor = caption_model_processor["model"], caption_model_processor["processor"]
    vocab = caption_vocabulary(vocabulary, processor)
    max_new = 20 if max_new_tokens is None else max_new_tokens
    if vocab is not None and max_new_tokens is None:
        max_new = max(max_new, vocab[0].longest)
    non_ocr = filtered_boxes[starting_idx:] if starting_idx else filtered_boxes
    H, W = image_source.shape[0], image_source.shape[1]
    boxes_px = crop_boxes_px(non_ocr.tolist() if isinstance(non_ocr, torch.Tensor) else non_ocr, W, H)
    if not boxes_px:
        return []
    img_dev = image_source if isinstance(image_source, torch.Tensor) else torch.from_numpy(np.array(image_source, order="C"))   # writable copy (PIL views are read-only)
    img_dev = img_dev.to(model.device)
    # prompt=None / "<CAPTION>": the call it always was (captioners without the keyword keep working); else the processor's ids
    pkw = {} if prompt is None or prompt == "<CAPTION>" else {"prompt_ids": processor.prompt_ids(prompt)}
    if generation is not None:
        pkw["controls"] = generation
    if vocab is not None:
        pkw["vocabulary"] = vocab[0]

    def texts_of(ids):
        texts = [t.strip() for t in processor.batch_decode(ids, skip_special_tokens=True)]
        if vocab is not None:                # a label given as a string comes back as that string
            for k, r in enumerate(ids.tolist()):
                j = vocab[0].label_index(r[1:], model.w.eos)
                if j >= 0 and vocab[1][j] is not None:
                    texts[k] = vocab[1][j]
        return texts
    if return_confidence:                    # only when asked for: captioners without the keyword keep working
        from ..florence import caption_confidence
        ids, logp = model.caption_crops(img_dev, boxes_px, max_new_tokens=max_new, batch_size=batch_size, return_scores=True, **pkw)
        w = model.w
        return [(t, caption_confidence(r, lp, w.eos, w.forced_bos, w.forced_eos, max_new)) for t, r, lp in zip(texts_of(ids), ids, logp)]
    ids = model.caption_crops(img_dev, boxes_px, max_new_tokens=max_new, batch_size=batch_size, **pkw)
    return texts_of(ids)


def caption_vocabulary(vocabulary, processor=None):
    """`vocabulary` of `get_parsed_content_icon` -> None, or (CaptionVocabulary, per distinct label the string it was given as or
    None).  Entries: strings (tokenised by `processor.prompt_ids`; ValueError without a tokenizer.json) or lists of token ids.
    ValueError: not a list, an entry of another type, and what `CaptionVocabulary` refuses."""
    if vocabulary is None:
        return None
    from ..florence import CaptionVocabulary
    if isinstance(vocabulary, CaptionVocabulary):
        return vocabulary, [None] * len(vocabulary.labels)
    if isinstance(vocabulary, (str, bytes, dict)) or not hasattr(vocabulary, "__iter__"):
        raise ValueError(f"a caption vocabulary is a list of strings or of token id lists, got {vocabulary!r}")
    rows, names = [], {}
    for entry in vocabulary:
        if isinstance(entry, str):
            if processor is None:
                raise ValueError("a caption vocabulary given as strings needs the caption processor to tokenise it")
            ids = tuple(int(t) for t in processor.prompt_ids(entry))
            names.setdefault(ids, entry)
        elif isinstance(entry, (bytes, dict)) or not hasattr(entry, "__iter__"):
            raise ValueError(f"caption vocabulary: an entry is a string or a list of token ids, got {entry!r}")
        else:
            ids = tuple(entry.tolist() if isinstance(entry, torch.Tensor) else entry)
        rows.append(ids)
    vocab = CaptionVocabulary(rows)
    return vocab, [names.get(lab) for lab in vocab.labels]


def _generation_kwargs(generation):
    """`generation` (None, a dict of generation controls or a GenerationControls) as keyword arguments of `generate`"""
    if generation is None:
        return {}
    if isinstance(generation, dict):
        return dict(generation)
    from ..florence import GEN_CTRL_KEYS
    return {k: getattr(generation, k) for k in GEN_CTRL_KEYS}


@torch.inference_mode()
def describe_image(image_source, caption_model_processor, task="<MORE_DETAILED_CAPTION>", max_new_tokens=256, return_ids=False,
                   generation=None):
    """Describe or read ONE WHOLE image (no detector, no crops): the image is resized to the captioner's resolution with Pillow
    bicubic — the processor's own resize at 768 — normalised by the processor, and decoded greedily from the task prompt; the text
    is `batch_decode` of the ids, stripped.  image_source: a path, a PIL image or an HWC uint8 array; a list of them gives a list
    of strings.  task: a Florence-2 task token without an input (`<CAPTION>`, `<DETAILED_CAPTION>`, `<MORE_DETAILED_CAPTION>`,
    `<OCR>`, ...) or free text, under the rules of `FlorenceProcessor.prompt_ids`: everything but `<CAPTION>` needs the
    tokenizer.json next to the checkpoint, tasks with an input are refused.  max_new_tokens: up to the decoder's position capacity
    (1024 for Florence-2-base).  return_ids: (text, ids i64 [T]) per image instead of the text.  generation: a dict of generation
    controls passed to `Florence2Captioner.generate` as keyword arguments (repetition_penalty, no_repeat_ngram_size, min_new_tokens,
    suppress_tokens, begin_suppress_tokens, bad_words_ids) — long greedy outputs are where a repetition penalty matters; None = the
    call as it was."""
    if isinstance(max_new_tokens, bool) or not isinstance(max_new_tokens, int) or max_new_tokens < 1:
        raise ValueError(f"max_new_tokens must be an integer >= 1, got {max_new_tokens!r}")
    if task is not None and not isinstance(task, str):
        raise ValueError(f"task is a Florence-2 task token or a free-text prompt (got {type(task).__name__})")
    if generation is not None:
        from ..florence import GenerationControls
        generation = dict(generation) if isinstance(generation, dict) else generation
        GenerationControls.of(generation)                  # a bad key or value: ValueError before the image is touched
    model, processor = caption_model_processor["model"], caption_model_processor["processor"]
    many = isinstance(image_source, (list, tuple))
    R = int(model.resolution)
    images = []
    for im in (image_source if many else [image_source]):
        if isinstance(im, str):
            im = Image.open(im)
        elif not isinstance(im, Image.Image):
            im = Image.fromarray(np.asarray(im))
        images.append(im.convert("RGB").resize((R, R), Image.Resampling.BICUBIC))
    if not images:
        return []
    inputs = processor(images=images, text=task, return_tensors="pt", do_resize=False)
    ids = model.generate(input_ids=inputs["input_ids"], pixel_values=inputs["pixel_values"], attention_mask=inputs["attention_mask"],
                         max_new_tokens=max_new_tokens, num_beams=1, do_sample=False, **(_generation_kwargs(generation)))
    texts = [t.strip() for t in processor.batch_decode(ids, skip_special_tokens=True)]
    out = [(t, r) for t, r in zip(texts, ids)] if return_ids else texts
    return out if many else out[0]


# ------------------------------------------------------------------------------------------ OCR by the caption model
_OCR_PATTERN = r"(.+?)" + r"<loc_(\d+)>" * 8            # transformers' Florence2PostProcessor pattern of the "ocr" task


def dequantize_bin(b: int, size: int) -> int:
    """pixel of location bin b (0..999) on an axis of `size` pixels: the bin's centre, truncated —
    Florence2PostProcessor.dequantize(...).int() in integers, and what OMNI_OP_REGION_OCR computes"""
    return ((2 * b + 1) * size) // 2000


def parse_ocr_regions(ids_row, processor, size):
    """The <OCR_WITH_REGION> answer of ONE image parsed on the host FROM ITS TEXT, as transformers'
    Florence2PostProcessor.parse_ocr_from_text_and_spans parses it: the tokens are rendered one by one (`loc_class_table` texts), the
    strings `<s>`, `</s>`, `<pad>` are deleted, and `(.+?)(<loc_N>){8}` is matched on what is left.  The device parses tokens
    instead (OMNI_OP_REGION_OCR) and flags the rows in which that can differ; this is what those rows fall back to.
    ids_row: the decoder start token and the generated ids (a row of `Florence2Captioner.read_regions().ids`); only the columns in
    front of the first EOS behind column 0 count.  size: (width, height) the bins are de-quantised to.
    -> [{"text" (stripped), "quad" [x0, y0, .. x3, y3] in pixels of the image, "columns": the columns of `ids_row` whose text the
    match covers}]"""
    _table, texts = processor.loc_class_table()
    row = [int(t) for t in (ids_row.tolist() if hasattr(ids_row, "tolist") else ids_row)]
    end = next((j for j in range(1, len(row)) if row[j] == processor.eos_id), len(row))
    text, owner = "", []
    for j in range(1, end):
        t = texts[row[j]] if 0 <= row[j] < len(texts) else ""
        text += t
        owner += [j] * len(t)
    for needle in ("<s>", "</s>", "<pad>"):                 # str.replace, with the owners of the deleted characters deleted too
        at = text.find(needle)
        while at >= 0:
            text = text[:at] + text[at + len(needle):]
            del owner[at:at + len(needle)]
            at = text.find(needle, at)
    import re
    w, h = size
    out = []
    for m in re.finditer(_OCR_PATTERN, text):
        bins = [int(g) for g in m.groups()[1:]]
        out.append({"text": m.group(1).strip(), "quad": [dequantize_bin(b, h if k & 1 else w) for k, b in enumerate(bins)],
                    "columns": sorted(set(owner[m.start():m.end()]))})
    return out


def _owns(cell, quad):
    """`florence.ocr_cells`' rule on the host: the doubled centre of the quad's box lies in the cell on both axes"""
    from ..florence import OCR_INF
    cx, cy = min(quad[0::2]) + max(quad[0::2]), min(quad[1::2]) + max(quad[1::2])
    return cell[2] <= cx and (cell[3] == OCR_INF or cx < cell[3]) and cell[4] <= cy and (cell[5] == OCR_INF or cy < cell[5])


@torch.inference_mode()
def read_text_regions(image_source, caption_model_processor, max_new_tokens=1024, overlap=128, min_confidence=0.0, generation=None,
                      return_stats=False):
    """Built-in OCR: the text of a screenshot with its places, read by the caption model itself (Florence-2's <OCR_WITH_REGION>
    task) — `Florence2Captioner.read_regions`: the frame is cut into tiles of the captioner's resolution on the device, unscaled,
    `overlap` pixels shared between neighbours; every tile is decoded greedily and its answer parsed on the device.
    image_source: a path, a PIL image, an HWC uint8 array or a device tensor.  generation: generation controls as in
    `describe_image`.  -> [{"text", "quad" [[x, y] x 4] and "bbox" [x0, y0, x1, y1] in frame pixels, "confidence", "tile"}], tile
    by tile, in reading order of the answer within a tile.  A region seen by two overlapping tiles is returned by the one whose cell
    holds the centre of its box (`florence.ocr_cells`); regions whose stripped text is empty and regions below `min_confidence` are
    dropped.  confidence = exp(mean log-probability of the region's tokens, content and location tokens alike).  A line of text
    that crosses a cell boundary is read twice, once per tile, each time as far as that tile sees it; both readings survive only
    when their box centres fall into their own cells.  Rows the device flags as holding a token it does not parse (a newline, a
    '<') are re-parsed from their text by `parse_ocr_regions` under the same ownership rule.
    return_stats=True: (regions, per tile {"found", "kept", "truncated", "fallback"}).
    ValueError before anything reaches the device: no tokenizer.json next to the checkpoint (naming the file), a tokenizer without
    Florence-2's location tokens, overlap outside 0 <= overlap < resolution, max_new_tokens beyond the decoder, min_confidence
    outside 0..1."""
    import math
    from ..florence import ocr_cells
    model, processor = caption_model_processor["model"], caption_model_processor["processor"]
    if isinstance(min_confidence, bool) or not isinstance(min_confidence, (int, float)) or not 0.0 <= min_confidence <= 1.0:
        raise ValueError(f"min_confidence must be a number in 0..1, got {min_confidence!r}")
    table, texts = processor.loc_class_table()
    prompt = processor.prompt_ids("<OCR_WITH_REGION>")
    if isinstance(image_source, str):
        image_source = Image.open(image_source)
    if isinstance(image_source, Image.Image):
        image_source = np.asarray(image_source.convert("RGB"))
    out = model.read_regions(_frame_on(image_source, model.device), max_new_tokens=max_new_tokens, overlap=overlap, prompt_ids=prompt,
                             class_table=table, controls=generation)
    R = int(model.resolution)
    cells = ocr_cells(out.origins, R)
    regions, stats = [], []
    for r, (ox, oy) in enumerate(out.origins):
        found, kept, flags = (int(v) for v in out.rows[r, :3])
        ids = out.ids[r].tolist()
        if flags & 1:                                       # from the text, on the host
            cands = []
            for reg in parse_ocr_regions(ids, processor, (R, R)):
                quad = [v + (oy if k & 1 else ox) for k, v in enumerate(reg["quad"])]
                cols = reg["columns"]
                cands.append((reg["text"], quad, float(sum(float(out.logp[r, j - 1]) for j in cols)), len(cols), _owns(cells[r], quad)))
            found, kept = len(cands), sum(1 for c in cands if c[4])
        else:
            cands = []
            for k in range(found):
                rec = out.records[r, k].tolist()
                text = "".join(texts[t] for t in ids[rec[1]:rec[2]] if table[t] != L.OCR_CLASS_STRIP).strip()
                cands.append((text, rec[3:11], float(out.sums[r, k]), rec[11], bool(rec[12])))
        stats.append({"found": found, "kept": kept, "truncated": bool(flags & 2), "fallback": bool(flags & 1)})
        for text, quad, total, count, own in cands:
            conf = math.exp(total / count) if count else 0.0
            if own and text and conf >= min_confidence:
                regions.append({"text": text, "quad": [[quad[0], quad[1]], [quad[2], quad[3]], [quad[4], quad[5]], [quad[6], quad[7]]],
                                "bbox": [min(quad[0::2]), min(quad[1::2]), max(quad[0::2]), max(quad[1::2])], "confidence": conf, "tile": r})
    return (regions, stats) if return_stats else regions


class FlorenceOCR:
    """The caption model as an OCR engine.  `readtext(image_np, **easyocr_args) -> [(quad, text, confidence)]` is EasyOCR's reader
    contract, so `set_ocr_engine(easyocr_reader=FlorenceOCR(cmp))` makes `check_ocr_box` read with it (EasyOCR's own keywords —
    text_threshold, paragraph, ... — are accepted and ignored); calling the object with a PIL image returns (texts, xyxy boxes), the
    `ocr_provider` contract of `Omniparser`.  defaults: max_new_tokens, overlap, min_confidence, generation of `read_text_regions`."""

    def __init__(self, caption_model_processor, **defaults):
        bad = sorted(set(defaults) - {"max_new_tokens", "overlap", "min_confidence", "generation"})
        if bad:
            raise ValueError(f"FlorenceOCR: unknown settings {bad} (max_new_tokens, overlap, min_confidence, generation)")
        self.caption_model_processor = caption_model_processor
        self.defaults = defaults

    def read(self, image):
        return read_text_regions(image, self.caption_model_processor, **self.defaults)

    def readtext(self, image_np, **easyocr_args):
        return [(r["quad"], r["text"], r["confidence"]) for r in self.read(image_np)]

    def __call__(self, pil_image):
        regions = self.read(pil_image)
        return [r["text"] for r in regions], [r["bbox"] for r in regions]


# ------------------------------------------------------------------------------------------ grounding: box answers and region prompts
_BOX_TASKS = {"<OD>": 0, "<DENSE_REGION_CAPTION>": 0, "<REGION_PROPOSAL>": 1,          # task -> grammar of OMNI_OP_REGION_OCR mode 3
              "<OPEN_VOCABULARY_DETECTION>": 0, "<CAPTION_TO_PHRASE_GROUNDING>": 0}
_PHRASE_PATTERNS = (r"[^<]+(?:<loc_\d+>){4,}", r"(?:<loc_\d+>){4,}")                      # grammar 0 / 1: transformers' phrase patterns
_PHRASE_TEXT = r"^\s*(.*?)(?=<od>|</od>|<box>|</box>|<bbox>|</bbox>|<loc_)"
_BOX_PATTERN = r"<loc_(\d+)>" * 4


def _answer_text(ids_row, processor):
    """(text, owner): the row's tokens in front of the first EOS behind column 0 rendered one by one (`loc_class_table` texts) with
    `<s>`, `</s>`, `<pad>` deleted as str.replace deletes them, and per character the column of `ids_row` it came from"""
    _table, texts = processor.loc_class_table()
    row = [int(t) for t in (ids_row.tolist() if hasattr(ids_row, "tolist") else ids_row)]
    end = next((j for j in range(1, len(row)) if row[j] == processor.eos_id), len(row))
    text, owner = "", []
    for j in range(1, end):
        t = texts[row[j]] if 0 <= row[j] < len(texts) else ""
        text += t
        owner += [j] * len(t)
    for needle in ("<s>", "</s>", "<pad>"):
        at = text.find(needle)
        while at >= 0:
            text = text[:at] + text[at + len(needle):]
            del owner[at:at + len(needle)]
            at = text.find(needle, at)
    return text, owner


def parse_box_answer(ids_row, processor, size, grammar):
    """The answer of ONE image to a task that replies "phrase <loc>x4 ..." parsed on the host FROM ITS TEXT, as transformers'
    Florence2PostProcessor parses it: grammar 0 is parse_description_with_bboxes_from_text_and_spans (and, but for its banned
    phrases, parse_phrase_grounding_from_text_and_spans), grammar 1 the same with allow_empty_phrase (<REGION_PROPOSAL>).  The device
    parses tokens instead (OMNI_OP_REGION_OCR mode 3) and flags the rows in which that can differ; this is what those rows fall
    back to.  ids_row, size: as in `parse_ocr_regions`.
    -> one entry per box, in the answer's order: {"label": the phrase, stripped, non-ASCII characters dropped, "raw_label": before
    they are dropped, "bbox" [x0, y0, x1, y1] in pixels of the image, "phrase": the ordinal of its phrase among those that gave
    boxes, "phrase_columns" / "box_columns": the columns of `ids_row` whose text the phrase / the box covers}"""
    import re
    if isinstance(grammar, bool) or grammar not in (0, 1):
        raise ValueError(f"grammar must be 0 (phrases with boxes) or 1 (boxes only), got {grammar!r}")
    text, owner = _answer_text(ids_row, processor)
    w, h = size
    out, ordinal = [], 0
    for m in re.finditer(_PHRASE_PATTERNS[grammar], text):
        chunk, own = m.group(0), owner[m.start():m.end()]
        for needle in ("<ground>", "<obj>"):                # str.replace(needle, "", 1)
            at = chunk.find(needle)
            if at >= 0:
                chunk = chunk[:at] + chunk[at + len(needle):]
                del own[at:at + len(needle)]
        if not chunk and grammar == 0:
            continue
        pm = re.search(_PHRASE_TEXT, chunk)
        if not pm:
            continue
        boxes = list(re.finditer(_BOX_PATTERN, chunk))
        if not boxes:
            continue
        raw = pm.group().strip()
        first_loc = chunk.find("<loc_")
        for b in boxes:
            bins = [int(g) for g in b.groups()]
            out.append({"label": raw.encode("ascii", "ignore").decode("ascii"), "raw_label": raw,
                        "bbox": [dequantize_bin(v, h if k & 1 else w) for k, v in enumerate(bins)], "phrase": ordinal,
                        "phrase_columns": sorted(set(own[:max(first_loc, 0)])), "box_columns": sorted(set(own[b.start():b.end()]))})
        ordinal += 1
    return out


_POLY_RUN = r"(?:(?:<loc_\d+>|<sep>|<poly>|</poly>){4,})"
_POLY_PHRASE = r"^\s*(.*?)(?=<od>|</od>|<box>|</box>|<bbox>|</bbox>|<loc_|<poly>)"


def parse_polygon_answer(ids_row, processor, size):
    """The answer of ONE image to a segmentation task parsed on the host FROM ITS TEXT, as transformers' Florence2PostProcessor parses
    it for the "polygons" type (parse_description_with_polygons_from_text_and_spans with allow_empty_phrase, no box at the start).  The
    device parses tokens instead (OMNI_OP_REGION_OCR mode 5) and flags the rows in which that can differ; this is what those rows
    fall back to.  ids_row, size: as in `parse_ocr_regions`.
    -> one entry per instance, in the answer's order: {"polygons": [[x0, y0, x1, y1, ...], ...] in pixels of the image (a polygon may
    be empty), "columns": the columns of `ids_row` whose location tokens made vertices}"""
    import re
    text, owner = _answer_text(ids_row, processor)
    w, h = size
    out = []
    for m in re.finditer(_POLY_RUN, text):
        phrase = m.group(0)
        if not re.search(_POLY_PHRASE, re.sub(r"^<loc_\d+>", "", phrase, count=1)):
            continue
        if "<poly>" in phrase and "</poly>" in phrase:
            contents = [(m.start() + q.start(1), q.group(1)) for q in re.finditer(r"<poly>(.*?)</poly>", phrase)]
        else:
            contents = [(m.start(), phrase)]
        for at, content in contents:
            found = list(re.finditer(r"((?:<loc_\d+>)+)(?:<sep>|$)", content))
            if not found:
                continue
            polygons, columns = [], []
            for q in found:
                bins = list(re.finditer(r"<loc_(\d+)>", q.group(1)))
                bins = bins[:len(bins) - len(bins) % 2]
                polygons.append([dequantize_bin(int(b.group(1)), h if k & 1 else w) for k, b in enumerate(bins)])
                columns += [owner[at + q.start(1) + b.start()] for b in bins]
            out.append({"polygons": polygons, "columns": columns})
    return out


def raster_polygons(polygons, origin, size, frame=None):
    """The mask rule of OMNI_OP_REGION_OCR mode 6 on the host (for instances beyond the device's instance slots and for fallback
    rows): bool [h, w] (y, x) of a window of `size` = (w, h) pixels whose top-left pixel is `origin` = (x, y) in the coordinates of
    `polygons` ([[x0, y0, x1, y1, ...], ...]).  A pixel is set when its centre lies inside at least one polygon of three or more
    vertices, even-odd per polygon, in exact integer arithmetic on doubled coordinates; with `frame` = (W, H) pixels outside
    [0, W) x [0, H) stay clear."""
    w, h = size
    ox, oy = origin
    px = (2 * (np.arange(w, dtype=np.int64) + ox) + 1)[None, :]
    py = (2 * (np.arange(h, dtype=np.int64) + oy) + 1)[:, None]
    out = np.zeros((h, w), bool)
    for poly in polygons:
        pts = [(2 * int(poly[k]), 2 * int(poly[k + 1])) for k in range(0, len(poly) - 1, 2)]
        if len(pts) < 3:
            continue
        par = np.zeros((h, w), bool)
        for k, (bx, by) in enumerate(pts):
            ax, ay = pts[k - 1]
            lhs, rhs = (px - ax) * (by - ay), (py - ay) * (bx - ax)
            par ^= ((ay > py) != (by > py)) & ((lhs < rhs) if by > ay else (lhs > rhs))
        out |= par
    if frame is not None:
        out &= (((py - 1) // 2 >= 0) & ((py - 1) // 2 < frame[1])) & (((px - 1) // 2 >= 0) & ((px - 1) // 2 < frame[0]))
    return out


def _box_tasks_check(task, text):
    """(grammar, queries): the phrases a box task is asked with, [None] for the tasks without an input"""
    if task not in _BOX_TASKS:
        raise ValueError(f"locate: task {task!r} does not answer in boxes ({', '.join(_BOX_TASKS)})")
    with_input = task in TASKS_WITH_INPUT
    if not with_input:
        if text is not None:
            raise ValueError(f"task {task} takes no text")
        return _BOX_TASKS[task], [None]
    queries = [text] if isinstance(text, str) else list(text) if text is not None else []
    if not queries or not all(isinstance(q, str) and q.strip() for q in queries):
        raise ValueError(f"task {task} needs a phrase or a list of phrases")
    return _BOX_TASKS[task], queries


@torch.inference_mode()
def locate(image_source, caption_model_processor, task="<OPEN_VOCABULARY_DETECTION>", text=None, max_new_tokens=256, overlap=128,
           min_confidence=0.0, banned_phrases=(), generation=None, return_stats=False):
    """Where is it?  Boxes in frame pixels from the caption model's own box tasks — `Florence2Captioner.locate_regions`: every
    phrase is put to every native-resolution tile of the frame (cut on the device, `overlap` pixels shared between neighbours),
    decoded greedily, and the answers "phrase <loc>x4 ..." are parsed on the device.
    task: <OPEN_VOCABULARY_DETECTION> or <CAPTION_TO_PHRASE_GROUNDING> with `text`, a phrase or a list of phrases (one decode row
    per phrase and tile); <OD>, <DENSE_REGION_CAPTION> or <REGION_PROPOSAL> (boxes without labels) with text=None.
    -> [{"label", "query", "bbox" [x0, y0, x1, y1] in frame pixels, "confidence", "tile", "phrase"}], query by query, tile by tile,
    in the answer's order within a tile.  label: the phrase the model wrote in front of the box, stripped, non-ASCII characters
    dropped (for phrase grounding a phrase in `banned_phrases` is dropped with its boxes, as transformers drops
    banned_grounding_tokens); query: the phrase asked for (None for the tasks without text); phrase: the ordinal of the label's
    phrase in its row — the boxes of one phrase share it.  A box seen by two overlapping tiles is returned by the tile whose cell
    holds its centre (`florence.ocr_cells`), as in `read_text_regions`.  confidence = exp((log-probability sum of the phrase's tokens
    + that of the box's four location tokens) / (phrase tokens + 4)); boxes below `min_confidence` are dropped.  Rows the device
    flags as holding a token it does not parse are re-parsed from their text by `parse_box_answer`; an <OPEN_VOCABULARY_DETECTION>
    row that answers with polygons (`<poly>`) yields no boxes.
    return_stats=True: (boxes, per row {"query", "tile", "found", "kept", "phrases", "truncated", "fallback", "polygons"}).
    ValueError before anything reaches the device: an unknown task, text missing or given to a task without one, no tokenizer.json,
    min_confidence outside 0..1, and `locate_regions`' own."""
    import math
    from ..florence import ocr_cells
    model, processor = caption_model_processor["model"], caption_model_processor["processor"]
    grammar, queries = _box_tasks_check(task, text)
    if isinstance(min_confidence, bool) or not isinstance(min_confidence, (int, float)) or not 0.0 <= min_confidence <= 1.0:
        raise ValueError(f"min_confidence must be a number in 0..1, got {min_confidence!r}")
    banned = set(banned_phrases) if task == "<CAPTION_TO_PHRASE_GROUNDING>" else set()
    table, texts = processor.loc_class_table()
    prompts = [processor.prompt_ids(task) if q is None else processor.task_prompt_ids(task, text=q) for q in queries]
    if isinstance(image_source, str):
        image_source = Image.open(image_source)
    if isinstance(image_source, Image.Image):
        image_source = np.asarray(image_source.convert("RGB"))
    out = model.locate_regions(_frame_on(image_source, model.device), prompts, table, grammar, max_new_tokens=max_new_tokens, overlap=overlap,
                               controls=generation)
    R = int(model.resolution)
    cells = ocr_cells(out.origins, R)
    found_boxes, stats = [], []
    for r, (ox, oy) in enumerate(out.origins):
        found, kept, flags, phrases = (int(v) for v in out.rows[r, :4])
        ids = out.ids[r].tolist()
        cands, poly = [], False                             # (raw label, label, bbox, log-probability sum, tokens, own, phrase ordinal)
        if flags & 1:                                       # from the text, on the host
            poly = task == "<OPEN_VOCABULARY_DETECTION>" and "<poly>" in _answer_text(ids, processor)[0]
            for g in ([] if poly else parse_box_answer(ids, processor, (R, R), grammar)):
                box = [g["bbox"][0] + ox, g["bbox"][1] + oy, g["bbox"][2] + ox, g["bbox"][3] + oy]
                cols = g["phrase_columns"] + g["box_columns"]
                own = _owns(cells[r], [box[0], box[1], box[2], box[3]])
                cands.append((g["raw_label"], g["label"], box, float(sum(float(out.logp[r, j - 1]) for j in cols)), len(cols), own, g["phrase"]))
            found, kept, phrases = len(cands), sum(1 for c in cands if c[5]), len({c[6] for c in cands})
        else:
            for k in range(found):
                rec = out.records[r, k].tolist()
                toks = [texts[t] for t in ids[rec[1]:rec[2]] if table[t] != L.OCR_CLASS_STRIP]
                if rec[11] and toks:
                    toks[0] = toks[0][1:]
                raw = "".join(toks).strip()
                cands.append((raw, raw.encode("ascii", "ignore").decode("ascii"), rec[3:7], float(out.sums[r, k, 0]) + float(out.sums[r, k, 1]),
                              rec[8] + 4, bool(rec[9]), rec[10]))
        q = queries[out.prompt_index[r]]
        stats.append({"query": q, "tile": out.tile_index[r], "found": found, "kept": kept, "phrases": phrases, "truncated": bool(flags & 2),
                      "fallback": bool(flags & 1), "polygons": poly})
        for raw, label, box, total, count, own, ordinal in cands:
            conf = math.exp(total / count)
            if own and raw not in banned and conf >= min_confidence:
                found_boxes.append({"label": label, "query": q, "bbox": [int(v) for v in box], "confidence": conf, "tile": out.tile_index[r],
                                    "phrase": ordinal})
    return (found_boxes, stats) if return_stats else found_boxes


def ground_elements(image_source, elements, caption_model_processor, phrases, min_iou=0.5, **locate_kw):
    """Which parsed element is "the Save button"?  `locate` for every phrase, and for each located box the element of `elements` (a
    `parsed_content_list` with ratio bboxes) it overlaps best.  On the host, with the box helpers of the overlap filter.
    -> per phrase a list of locate's boxes, each with "element": the index of the element with the largest IoU (ties: the lower
    index), or -1 when that IoU is below `min_iou`, and "iou": that IoU."""
    if isinstance(min_iou, bool) or not isinstance(min_iou, (int, float)) or not 0.0 <= min_iou <= 1.0:
        raise ValueError(f"min_iou must be a number in 0..1, got {min_iou!r}")
    phrases = [phrases] if isinstance(phrases, str) else list(phrases)
    locate_kw.setdefault("task", "<OPEN_VOCABULARY_DETECTION>")
    if locate_kw.get("return_stats"):
        raise ValueError("ground_elements returns boxes only: return_stats is not supported")
    if isinstance(image_source, str):
        image_source = Image.open(image_source)
    if isinstance(image_source, Image.Image):
        image_source = np.asarray(image_source.convert("RGB"))
    H, W = image_source.shape[0], image_source.shape[1]
    boxes = locate(image_source, caption_model_processor, text=phrases, **locate_kw)
    px = [[e["bbox"][0] * W, e["bbox"][1] * H, e["bbox"][2] * W, e["bbox"][3] * H] for e in elements]
    out = [[] for _ in phrases]
    for b in boxes:
        best, best_iou = -1, 0.0
        for k, e in enumerate(px):
            it = _inter(b["bbox"], e)
            union = _area(b["bbox"]) + _area(e) - it
            iou = it / union if union > 0 else 0.0
            if iou > best_iou:
                best, best_iou = k, iou
        out[phrases.index(b["query"])].append({**b, "element": best if best_iou >= min_iou else -1, "iou": best_iou})
    return out


@torch.inference_mode()
def describe_regions(image_source, boxes_px, caption_model_processor, task="<REGION_TO_DESCRIPTION>", max_new_tokens=64, overlap=128,
                     generation=None):
    """What is in this box, seen in its surroundings?  Florence-2's region tasks (<REGION_TO_DESCRIPTION>, <REGION_TO_CATEGORY>,
    <REGION_TO_OCR>) on native-resolution tiles: each box [x0, y0, x1, y1] in frame pixels goes to the tile of
    `ScreenParser.tile_origins(W, H, R, R, overlap)` whose cell (`florence.ocr_cells`) holds its centre, is clipped to that tile and
    written into the prompt as four location tokens quantised in tile coordinates (`FlorenceProcessor.task_prompt_ids`); one decode
    row per box (`Florence2Captioner.decode_tiles`).  -> the texts, `batch_decode`d and stripped, one per box.
    ValueError before anything reaches the device: another task, a box that is not four numbers with x0 <= x1 and y0 <= y1, no
    tokenizer.json, and `decode_tiles`' own."""
    from ..florence import ocr_cells
    from ..pipeline import ScreenParser
    model, processor = caption_model_processor["model"], caption_model_processor["processor"]
    if task not in ("<REGION_TO_DESCRIPTION>", "<REGION_TO_CATEGORY>", "<REGION_TO_OCR>"):
        raise ValueError(f"describe_regions: task {task!r} takes no region (<REGION_TO_DESCRIPTION>, <REGION_TO_CATEGORY>, <REGION_TO_OCR>)")
    R = int(model.resolution)
    if isinstance(overlap, bool) or not isinstance(overlap, int) or not 0 <= overlap < R:
        raise ValueError(f"overlap must be an integer in 0..{R - 1} (tiles are {R} x {R}), got {overlap!r}")
    boxes = [[float(v) for v in b] for b in boxes_px]
    if any(len(b) != 4 or not (b[0] <= b[2] and b[1] <= b[3]) for b in boxes):
        raise ValueError("a box is [x0, y0, x1, y1] in frame pixels with x0 <= x1 and y0 <= y1")
    if not boxes:
        return []
    if isinstance(image_source, str):
        image_source = Image.open(image_source)
    if isinstance(image_source, Image.Image):
        image_source = np.asarray(image_source.convert("RGB"))
    H, W = image_source.shape[0], image_source.shape[1]
    tiles = ScreenParser.tile_origins(W, H, R, R, overlap)[0]
    cells = ocr_cells(tiles, R)
    origins, prompts = [], []
    for b in boxes:
        k = next(k for k, c in enumerate(cells) if _owns(c, [b[0], b[1], b[2], b[3]]))     # the cells partition the plane
        ox, oy = tiles[k]
        region = [min(max(b[0] - ox, 0), R), min(max(b[1] - oy, 0), R), min(max(b[2] - ox, 0), R), min(max(b[3] - oy, 0), R)]
        origins.append((ox, oy))
        prompts.append(processor.task_prompt_ids(task, region=region, size=(R, R)))
    out = model.decode_tiles(_frame_on(image_source, model.device), origins, prompts, max_new_tokens, controls=generation)
    return [t.strip() for t in processor.batch_decode(out.ids, skip_special_tokens=True)]


def _mask_point(mask, origin):
    """[x, y] of the set pixel nearest the centroid of the set pixels of a bool mask whose top-left pixel is `origin` (ties: the lower
    y, then the lower x; exact: distances are compared as integers scaled by the pixel count), None for an empty mask"""
    ys, xs = np.nonzero(mask)
    if not len(xs):
        return None
    n = len(xs)
    d = (n * xs.astype(np.int64) - int(xs.sum())) ** 2 + (n * ys.astype(np.int64) - int(ys.sum())) ** 2
    k = int(np.argmin(d))                                  # the first of the equals: np.nonzero lists pixels by ascending y, then x
    return [int(xs[k]) + origin[0], int(ys[k]) + origin[1]]


@torch.inference_mode()
def segment(image_source, caption_model_processor, text=None, regions=None, max_new_tokens=256, overlap=128, min_confidence=0.0, instances=4,
            return_masks=True, generation=None, return_stats=False):
    """What shape is it?  Polygons and pixel masks in frame pixels from the caption model's two segmentation tasks —
    `Florence2Captioner.segment_regions`: rows over native-resolution tiles of the frame, decoded greedily, the polygon answers parsed
    and rastered on the device.  Exactly one of:
    text: a phrase or a list of phrases, <REFERRING_EXPRESSION_SEGMENTATION>; every phrase is put to every tile of
      `ScreenParser.tile_origins(W, H, R, R, overlap)`, and an instance seen by two overlapping tiles is returned by the tile whose cell
      holds the centre of its bounding box (`florence.ocr_cells`), as in `locate`;
    regions: boxes [x0, y0, x1, y1] in frame pixels, <REGION_TO_SEGMENTATION>; each box goes to the tile whose cell holds its centre,
      clipped to that tile and quantised in tile coordinates exactly as `describe_regions` does.  Every instance of the answer is
      returned: a box was put to ONE tile, so there is nothing to de-duplicate, and what a box gives does not depend on the other
      boxes of the call.
    -> [{"query" (the phrase) or "region" (the box), "index" (its ordinal in the input), "polygons" [[x0, y0, x1, y1, ...], ...],
    "bbox" [x0, y0, x1, y1] over all vertices, "area" (set pixels), "confidence", "tile", "point", "mask", "mask_origin"}], input by
    input, tile by tile, in the answer's order within a row.  mask: a bool array [bbox height, bbox width] whose top-left pixel is
    mask_origin = (bbox x0, bbox y0): a pixel is set when it lies in the frame and in its tile and its centre lies inside a polygon of
    three or more vertices of the instance (even-odd per polygon) — empty, [0, w] or [h, 0], for an instance whose vertices share
    an x or a y; None with return_masks=False.  point: [x, y] of the set pixel
    nearest the centroid of the set pixels (ties: the lower y, then the lower x) — a click point that lies ON the element; None for
    an empty mask.  confidence = exp(mean log-probability of the instance's vertex tokens); instances below `min_confidence` are
    dropped.  The first `instances` instances of a row are rastered on the device, later ones by `raster_polygons`; rows the device
    flags as holding a token it does not parse are re-parsed from their text by `parse_polygon_answer` and rastered on the host.
    return_stats=True: (instances, per row {"index", "tile", "polygons", "found", "kept", "truncated", "fallback"}).
    ValueError before anything reaches the model: both or neither of text and regions, an empty or non-string phrase, a box that is
    not four numbers with x0 <= x1 and y0 <= y1, no tokenizer.json or one without <sep> / <poly> / </poly>, min_confidence outside
    0..1, instances outside 1..64, overlap outside 0..R-1, and `segment_regions`' own."""
    import math
    from ..florence import ocr_cells
    from ..pipeline import ScreenParser
    model, processor = caption_model_processor["model"], caption_model_processor["processor"]
    if (text is None) == (regions is None):
        raise ValueError("segment takes exactly one of text (a phrase or a list of phrases) and regions (boxes in frame pixels)")
    if isinstance(min_confidence, bool) or not isinstance(min_confidence, (int, float)) or not 0.0 <= min_confidence <= 1.0:
        raise ValueError(f"min_confidence must be a number in 0..1, got {min_confidence!r}")
    if isinstance(instances, bool) or not isinstance(instances, int) or not 1 <= instances <= 64:
        raise ValueError(f"instances must be an integer in 1..64, got {instances!r}")
    R = int(model.resolution)
    if isinstance(overlap, bool) or not isinstance(overlap, int) or not 0 <= overlap < R:
        raise ValueError(f"overlap must be an integer in 0..{R - 1} (tiles are {R} x {R}), got {overlap!r}")
    if text is not None:
        queries = [text] if isinstance(text, str) else list(text)
        if not queries or not all(isinstance(q, str) and q.strip() for q in queries):
            raise ValueError("<REFERRING_EXPRESSION_SEGMENTATION> needs a phrase or a list of phrases")
    else:
        queries = [[float(v) for v in b] for b in regions]
        if any(len(b) != 4 or not (b[0] <= b[2] and b[1] <= b[3]) for b in queries):
            raise ValueError("a region is [x0, y0, x1, y1] in frame pixels with x0 <= x1 and y0 <= y1")
    table, _texts = processor.poly_class_table()
    if isinstance(image_source, str):
        image_source = Image.open(image_source)
    if isinstance(image_source, Image.Image):
        image_source = np.asarray(image_source.convert("RGB"))
    H, W = int(image_source.shape[0]), int(image_source.shape[1])
    tiles = ScreenParser.tile_origins(W, H, R, R, overlap)[0]
    grid = ocr_cells(tiles, R)
    origins, prompts, index, tile_of = [], [], [], []
    if text is not None:
        for i, q in enumerate(queries):
            row = processor.segment_prompt_ids("<REFERRING_EXPRESSION_SEGMENTATION>", text=q)
            for k, o in enumerate(tiles):
                origins.append(o)
                prompts.append(row)
                index.append(i)
                tile_of.append(k)
    else:
        for i, b in enumerate(queries):
            k = next(k for k, c in enumerate(grid) if _owns(c, [b[0], b[1], b[2], b[3]]))     # the cells partition the plane
            ox, oy = tiles[k]
            region = [min(max(b[0] - ox, 0), R), min(max(b[1] - oy, 0), R), min(max(b[2] - ox, 0), R), min(max(b[3] - oy, 0), R)]
            origins.append((ox, oy))
            prompts.append(processor.segment_prompt_ids("<REGION_TO_SEGMENTATION>", region=region, size=(R, R)))
            index.append(i)
            tile_of.append(k)
    if not origins:
        return ([], []) if return_stats else []
    # phrases: the cells of the frame's tile grid; regions: every row owns the whole plane
    cells = ocr_cells(origins, R) if text is not None else [[ox, oy, -2 ** 31, 2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1] for ox, oy in origins]
    out = model.segment_regions(_frame_on(image_source, model.device), origins, prompts, table, max_new_tokens=max_new_tokens, instances=instances,
                                masks=True, controls=generation, cells=cells)
    records, vertices, sums = np.asarray(out.records), np.asarray(out.vertices), np.asarray(out.sums)
    words = np.asarray(out.masks).view(np.uint32)
    key = "query" if text is not None else "region"
    found_instances, stats = [], []
    for r, (ox, oy) in enumerate(origins):
        n_poly, n_inst, flags, kept = (int(v) for v in out.rows[r, :4])
        cands = []                                          # (polygons in frame pixels, log-probability sum, tokens, device slot or None)
        if flags & 1:                                       # from the text, on the host
            ids = out.ids[r].tolist()
            for g in parse_polygon_answer(ids, processor, (R, R)):
                polys = [[v + (oy if q & 1 else ox) for q, v in enumerate(p)] for p in g["polygons"]]
                cands.append((polys, float(sum(float(out.logp[r, j - 1]) for j in g["columns"])), len(g["columns"]), None))
            n_poly, n_inst = sum(len(c[0]) for c in cands), len(cands)
        else:
            for k in range(n_poly):
                rec = records[r, k]
                if rec[2] == 0:
                    cands.append(([], 0.0, 0, int(rec[1]) if rec[1] < instances else None))
                c = cands[-1]
                cands[-1] = (c[0] + [vertices[r, rec[3]:rec[3] + rec[4]].reshape(-1).tolist()], c[1] + float(sums[r, k]), c[2] + 2 * int(rec[4]), c[3])
        kept = 0
        for polys, total, count, slot in cands:
            xs, ys = [v for p in polys for v in p[0::2]], [v for p in polys for v in p[1::2]]
            if not xs or not _owns(cells[r], [min(xs), min(ys), max(xs), max(ys)]):
                continue
            kept += 1
            conf = math.exp(total / count)
            if conf < min_confidence:
                continue
            bbox = [min(xs), min(ys), max(xs), max(ys)]
            w, h = bbox[2] - bbox[0], bbox[3] - bbox[1]
            if slot is not None:                            # the device's tile-local bits: only the box's pixel rows and words are unpacked
                x0, x1 = bbox[0] - ox, bbox[2] - ox
                w0, w1 = x0 // 32, (x1 + 31) // 32
                part = words[r, slot, bbox[1] - oy:bbox[3] - oy, w0:w1]
                bits = ((part[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).reshape(h, 32 * (w1 - w0))
                mask = np.ascontiguousarray(bits[:, x0 - 32 * w0:x1 - 32 * w0])
            else:
                mask = raster_polygons(polys, (bbox[0], bbox[1]), (w, h), frame=(W, H))
                mask &= raster_polygons([[ox, oy, ox + R, oy, ox + R, oy + R, ox, oy + R]], (bbox[0], bbox[1]), (w, h))    # tile pixels only
            found_instances.append({key: queries[index[r]], "index": index[r], "polygons": polys, "bbox": bbox, "area": int(mask.sum()),
                                    "confidence": conf, "tile": tile_of[r], "point": _mask_point(mask, (bbox[0], bbox[1])),
                                    "mask": mask if return_masks else None, "mask_origin": (bbox[0], bbox[1])})
        stats.append({"index": index[r], "tile": tile_of[r], "polygons": n_poly, "found": n_inst, "kept": kept, "truncated": bool(flags & 2),
                      "fallback": bool(flags & 1)})
    return (found_instances, stats) if return_stats else found_instances


def segment_elements(image_source, elements, caption_model_processor, **kw):
    """The shape of every parsed element: `segment(regions=...)` with the elements' boxes (a `parsed_content_list` with ratio bboxes)
    -> per element the most confident instance its box gave, or None when it gave none."""
    if kw.get("return_stats") or "text" in kw or "regions" in kw:
        raise ValueError("segment_elements takes the regions from the elements and returns instances only")
    if isinstance(image_source, str):
        image_source = Image.open(image_source)
    if isinstance(image_source, Image.Image):
        image_source = np.asarray(image_source.convert("RGB"))
    H, W = image_source.shape[0], image_source.shape[1]
    boxes = [[e["bbox"][0] * W, e["bbox"][1] * H, e["bbox"][2] * W, e["bbox"][3] * H] for e in elements]
    best = [None] * len(boxes)
    for g in segment(image_source, caption_model_processor, regions=boxes, **kw):
        if best[g["index"]] is None or g["confidence"] > best[g["index"]]["confidence"]:
            best[g["index"]] = g
    return best


@torch.inference_mode()
def rank_elements(image_source, elements, caption_model_processor, queries, top_k=None, prompt=None, normalize="mean"):
    """Rank the elements of a screenshot by how likely the caption model finds each query as the text of the element's crop ("which
    element is the save button?"): `Florence2Captioner.score_crops` — one encode per crop, every query a teacher-forced row of the
    same decode — and `florence.sequence_score`.
    image_source: the uint8 HWC numpy image or a device tensor; elements: a `parsed_content_list` with ratio bboxes, of any element
    type; queries: strings (tokenised by the processor's `prompt_ids`: they need the tokenizer.json next to the checkpoint, ValueError
    without it) or lists of token ids (bos ... eos; always work); prompt: the caption prompt of every crop (None = <CAPTION>).
    Crops are cut as `crop_boxes_px` cuts them; elements whose crop is empty are skipped.
    -> per query a list of {"index": position in `elements`, "score"} by descending score (ties: the lower index), cut to top_k."""
    from ..florence import sequence_score
    model, processor = caption_model_processor["model"], caption_model_processor["processor"]
    if top_k is not None and (isinstance(top_k, bool) or not isinstance(top_k, int) or top_k < 1):
        raise ValueError(f"top_k must be a positive integer or None, got {top_k!r}")
    labels = [processor.prompt_ids(q) if isinstance(q, str) else [int(t) for t in q] for q in queries]
    if not labels:
        raise ValueError("no queries: at least one is needed")
    H, W = image_source.shape[0], image_source.shape[1]
    index, boxes_px = [], []
    for k, e in enumerate(elements):
        px = crop_boxes_px([e["bbox"]], W, H)
        if px:
            index.append(k)
            boxes_px.append(px[0])
    img_dev = image_source if isinstance(image_source, torch.Tensor) else torch.from_numpy(np.array(image_source, order="C"))
    pkw = {} if prompt is None or prompt == "<CAPTION>" else {"prompt_ids": processor.prompt_ids(prompt) if isinstance(prompt, str) else list(prompt)}
    out = model.score_crops(img_dev.to(model.device), boxes_px, labels, **pkw)
    scores = sequence_score(out.token_logprobs, out.lengths, labels=[labels] * len(boxes_px), normalize=normalize,
                            forced_bos=model.w.forced_bos)
    ranked = []
    for j in range(len(labels)):
        order = sorted(range(len(index)), key=lambda b: (-float(scores[b, j]), index[b]))
        ranked.append([{"index": index[b], "score": float(scores[b, j])} for b in order][:top_k])
    return ranked


def _frame_on(image_source, device):
    img = image_source if isinstance(image_source, torch.Tensor) else torch.from_numpy(np.array(image_source, order="C"))
    return img.to(device)


@torch.inference_mode()
def embed_elements(image_source, elements, caption_model_processor):
    """Visual embeddings of the elements of a screenshot ("which element looks like this one?"): `Florence2Captioner.embed_crops`
    — the DaViT tower and the projector per crop, no encoder and no decode.
    image_source: the uint8 HWC numpy image or a device tensor; elements: a `parsed_content_list` with ratio bboxes, of any element
    type.  Crops are cut as `crop_boxes_px` cuts them; elements whose crop is empty are skipped.
    -> (index, embeddings): positions in `elements` (as `rank_elements` reports them) and f32 [len(index), d_model] unit vectors
    on the device, a pure function of each crop's pixels."""
    model = caption_model_processor["model"]
    H, W = image_source.shape[0], image_source.shape[1]
    index, boxes_px = [], []
    for k, e in enumerate(elements):
        px = crop_boxes_px([e["bbox"]], W, H)
        if px:
            index.append(k)
            boxes_px.append(px[0])
    return index, model.embed_crops(_frame_on(image_source, model.device), boxes_px)


@torch.inference_mode()
def embed_exemplars(exemplars, caption_model_processor):
    """f32 [m, d_model] on the device: `exemplars` as it is when it is such a tensor of embeddings, else one embedding per image
    (HWC uint8 arrays or PIL images), each through the 64x64 bilinear step and the resize to the captioner's resolution that a crop
    of the image's full rectangle takes (`embed_crops` of [0, 0, W, H])."""
    model = caption_model_processor["model"]
    if isinstance(exemplars, torch.Tensor):
        if exemplars.dtype != torch.float32 or exemplars.dim() != 2:
            raise ValueError(f"exemplar embeddings are an f32 [m, D] tensor, got {exemplars.dtype} {tuple(exemplars.shape)}")
        return exemplars.to(model.device)
    if isinstance(exemplars, (str, bytes, dict, np.ndarray)) or not hasattr(exemplars, "__iter__"):
        raise ValueError("exemplars are a list of images (HWC uint8 arrays or PIL images) or an f32 [m, D] tensor of embeddings")
    rows = []
    for ex in exemplars:
        arr = np.array(ex.convert("RGB") if isinstance(ex, Image.Image) else ex, order="C")
        if arr.dtype != np.uint8 or arr.ndim != 3 or arr.shape[2] != 3 or not arr.shape[0] or not arr.shape[1]:
            raise ValueError(f"an exemplar image is HWC uint8 with 3 channels, got {arr.dtype} {arr.shape}")
        rows.append(model.embed_crops(torch.from_numpy(arr).to(model.device), [[0, 0, arr.shape[1], arr.shape[0]]]))
    if not rows:
        raise ValueError("no exemplars: at least one is needed")
    return torch.cat(rows)


def _match_lists(index, idx, score, min_score):
    """device (idx, score) of a match against the embeddings of `index` -> per query [{"index", "score"}], cut at min_score"""
    out = []
    for irow, srow in zip(idx.tolist(), score.tolist()):
        out.append([{"index": index[i], "score": s} for i, s in zip(irow, srow) if i >= 0 and (min_score is None or s >= min_score)])
    return out


@torch.inference_mode()
def match_elements(image_source, elements, caption_model_processor, exemplars, top_k=5, min_score=None):
    """Find by exemplar: which elements of the screenshot look like these images?  `embed_elements`, `embed_exemplars` and
    `Florence2Captioner.match` (cosine similarity of the embeddings, top-k on the device).
    exemplars: a list of images or an f32 [m, D] tensor of embeddings (`embed_exemplars`); top_k: 1..8; min_score: drop matches
    below this similarity (None = keep all).
    -> per exemplar a list of {"index": position in `elements`, "score"} by descending score (ties: the lower index), at most top_k."""
    from ..florence import check_match_args
    model = caption_model_processor["model"]
    if min_score is not None and (isinstance(min_score, bool) or not isinstance(min_score, (int, float))):
        raise ValueError(f"min_score must be a number or None, got {min_score!r}")
    if isinstance(exemplars, torch.Tensor):
        check_match_args(exemplars, exemplars, top_k)
    index, emb = embed_elements(image_source, elements, caption_model_processor)
    queries = embed_exemplars(exemplars, caption_model_processor)
    if not index:
        check_match_args(queries, queries, top_k)
        return [[] for _ in range(queries.shape[0])]
    idx, score = model.match(queries, emb, top_k=top_k)
    return _match_lists(index, idx, score, min_score)


@torch.inference_mode()
def track_elements(prev, cur, min_score=0.9, top_k=4):
    """Track across screenshots: which element of `cur` is which element of `prev`?  prev, cur: (index, embeddings) pairs as
    `embed_elements` returns them.  Both directions' top_k come from the device (`florence.match_topk`); the filter runs on the
    host: a pair is a candidate when each side is among the other's top_k with a score of at least min_score, and candidates are
    accepted by descending score (ties: the lower prev index, then the lower cur index) while both sides are still free — every
    accepted pair is the mutual best among the elements still unpaired, each element is paired at most once.
    -> [(prev_index, cur_index, score)] by ascending prev_index."""
    from ..florence import match_topk
    (pi, pe), (ci, ce) = prev, cur
    if isinstance(min_score, bool) or not isinstance(min_score, (int, float)):
        raise ValueError(f"min_score must be a number, got {min_score!r}")
    if len(pi) != pe.shape[0] or len(ci) != ce.shape[0]:
        raise ValueError("an (index, embeddings) pair whose index and embeddings differ in length")
    if not len(pi) or not len(ci):
        if isinstance(top_k, bool) or not isinstance(top_k, int) or not 1 <= top_k <= 8:
            raise ValueError(f"top_k must be an integer in 1..8, got {top_k!r}")
        return []
    fi, fs = match_topk(pe, ce, top_k)
    bi, _ = match_topk(ce, pe, top_k, fi.device)
    fi, fs, bi = fi.tolist(), fs.tolist(), bi.tolist()
    cand = sorted((-s, pi[a], ci[b], a, b) for a in range(len(pi)) for b, s in zip(fi[a], fs[a])
                  if b >= 0 and s >= min_score and a in bi[b])
    used_a, used_b, out = set(), set(), []
    for neg, ia, ib, a, b in cand:
        if a not in used_a and b not in used_b:
            used_a.add(a); used_b.add(b)
            out.append((ia, ib, -neg))
    return sorted(out)


def _box_convert_xyxy_to_cxcywh(b: torch.Tensor) -> torch.Tensor:
    x1, y1, x2, y2 = b.unbind(-1)
    return torch.stack(((x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1), -1)


def annotate(image_source: np.ndarray, boxes: torch.Tensor, logits, phrases, text_scale=0.4, text_padding=5,
             text_thickness=2, thickness=3):
    """ref:util/utils.py:336-364: boxes cxcywh ratios -> (annotated RGB frame, {str(phrase): xywh px}).  Labels are
    the running box indices (not `phrases`), exactly as the reference; layout = util/overlay.py (pinned to the
    reference's cv2 call sequence), raster = Pillow (cv2/supervision are absent)."""
    from .overlay import BoxAnnotator
    h, w, _ = image_source.shape
    b = boxes * torch.Tensor([w, h, w, h])
    cx, cy, bw, bh = b.unbind(-1)
    xyxy = torch.stack((cx - 0.5 * bw, cy - 0.5 * bh, cx + 0.5 * bw, cy + 0.5 * bh), -1).numpy()    # torchvision box_convert
    xywh = torch.stack((cx - 0.5 * bw, cy - 0.5 * bh, bw, bh), -1).numpy()
    labels = [f"{i}" for i in range(b.shape[0])]
    frame = np.array(image_source, order="C")
    BoxAnnotator(text_scale=text_scale, text_padding=text_padding, text_thickness=text_thickness, thickness=thickness).annotate(
        frame, xyxy, labels=labels, image_size=(w, h))
    label_coordinates = {f"{phrase}": v for phrase, v in zip(phrases, xywh)}
    return frame, label_coordinates


def encode_png_b64(frame: np.ndarray, compress_level: int = 6) -> str:
    """ref:util/utils.py:485-488: RGB frame -> PNG -> base64 ascii (compress_level: zlib effort, 6 = Pillow's default)."""
    buf = io.BytesIO()
    Image.fromarray(frame).save(buf, format="PNG", compress_level=compress_level)
    return base64.b64encode(buf.getvalue()).decode("ascii")


def overlay_on_device(device=None) -> bool:
    """Where the tail of `get_som_labeled_img` (ref:util/utils.py:478-488: annotate + PNG + base64) runs.  OMNI_OVERLAY = device | host
    decides; unset (round 6 on): on the device whenever the models live on a GPU — 18 ms instead of 51 ms per 1080p screenshot and a
    PNG within 1.16x of Pillow's bytes (tools/annotate_bench.py, profiles/r6_s4_annotate_bench.json) — on the host otherwise
    (rounds 2-5 defaulted to the host because the device PNG was 2.7x Pillow's size)."""
    mode = os.environ.get("OMNI_OVERLAY", "auto")
    if mode in ("device", "host"):
        return mode == "device"
    try:
        return device is not None and torch.device(device).type == "cuda"
    except (TypeError, RuntimeError):
        return False


def png_pack_device(frame: torch.Tensor, want_b64=True, stream=None):
    """OMNI_OP_PNG_PACK: uint8 [H,W,3] device tensor -> (PNG file bytes, base64 ASCII) as device tensors (stored-deflate PNG:
    include/omni_amd.h; layout restated in oracle/png_ref.py).  Five small launches, no host work."""
    H, W = frame.shape[:2]
    assert frame.dtype == torch.uint8 and frame.is_contiguous() and frame.shape[2] == 3
    u = H * (3 * W + 1)
    size = u + 5 * ((u + 65534) // 65535) + 63
    nseg = (size - 53 + 4095) // 4096
    png = torch.empty(size, dtype=torch.uint8, device=frame.device)
    part = torch.empty(2 * H + nseg, dtype=torch.int32, device=frame.device)
    b64 = torch.empty(4 * ((size + 2) // 3), dtype=torch.uint8, device=frame.device) if want_b64 else None
    L.launch(L.make_op(L.OP_PNG_PACK, L.F32, p=[frame.data_ptr(), png.data_ptr(), part.data_ptr(), b64.data_ptr() if want_b64 else None],
                       i={0: H, 1: W, 2: part.numel(), 3: size}), stream)
    return png, b64


def png_deflate_device(frame: torch.Tensor, want_b64=True, stream=None, lz=True):
    """OMNI_OP_PNG_DEFLATE: like png_pack_device with a compressed stream.  lz=True (default since round 6): Up filter + LZ77 +
    dynamic Huffman, one GPU lane per 32 KiB unit — within 1.1-1.3x of Pillow's zlib level 6 (oracle/png_ref.py::deflate_png_lz is
    the byte-exact restatement); lz=False: the fixed-Huffman run-length stream of rounds 3-5 (one thread per 4096-byte unit, 2.7x
    Pillow's bytes; oracle/png_ref.py::deflate_png).  The size is decided on the device:
    -> (PNG buffer, base64 buffer, meta) device tensors; meta[1] = file bytes, meta[2] = base64 bytes."""
    H, W = frame.shape[:2]
    assert frame.dtype == torch.uint8 and frame.is_contiguous() and frame.shape[2] == 3
    dev = frame.device
    u = H * (3 * W + 1)
    units = (u + 4095) // 4096
    units_lz = (u + 32767) // 32768
    cap = u + 5 * units + 63
    nseg = (cap - 53 + 4095) // 4096
    png = torch.empty(cap, dtype=torch.uint8, device=dev)
    filt = torch.empty(u, dtype=torch.uint8, device=dev)
    slots = torch.empty(max(units * 4640, units_lz * 33792 if lz else 0), dtype=torch.uint8, device=dev)
    meta = torch.zeros(4 + 2 * units, dtype=torch.int32, device=dev)
    part = torch.empty(2 * H + nseg, dtype=torch.int32, device=dev)
    b64 = torch.empty(4 * ((cap + 2) // 3), dtype=torch.uint8, device=dev) if want_b64 else None
    toks = torch.empty(units_lz * 32768, dtype=torch.int32, device=dev) if lz else None
    L.launch(L.make_op(L.OP_PNG_DEFLATE, L.F32,
                       p=[frame.data_ptr(), png.data_ptr(), filt.data_ptr(), slots.data_ptr(), meta.data_ptr(), part.data_ptr(),
                          b64.data_ptr() if want_b64 else None, toks.data_ptr() if lz else None],
                       i={0: H, 1: W, 2: cap, 3: meta.numel(), 4: part.numel(), 5: 1 if lz else 0}), stream)
    return png, b64, meta


def annotate_encode_device(image_np: np.ndarray, boxes: torch.Tensor, phrases, device, text_scale=0.4, text_padding=5, text_thickness=2,
                           thickness=3, frame_dev: Optional[torch.Tensor] = None, stored: bool = False):
    """`annotate` + `encode_png_b64` with the raster, the PNG packing and the base64 on the device (OMNI_OVERLAY=device): same
    layout (util/overlay.py::plan_overlay), same pixels as the host raster, stored-deflate PNG; the host uploads the frame and a
    few KB of primitives and reads back ASCII.  -> (base64 str, label_coordinates)."""
    from .overlay import BoxAnnotator, render_device
    h, w = (image_np.shape if image_np is not None else frame_dev.shape)[:2]
    b = boxes * torch.Tensor([w, h, w, h])
    cx, cy, bw, bh = b.unbind(-1)
    xyxy = torch.stack((cx - 0.5 * bw, cy - 0.5 * bh, cx + 0.5 * bw, cy + 0.5 * bh), -1).numpy()
    xywh = torch.stack((cx - 0.5 * bw, cy - 0.5 * bh, bw, bh), -1).numpy()
    ann = BoxAnnotator(text_scale=text_scale, text_padding=text_padding, text_thickness=text_thickness, thickness=thickness)
    cmds = ann.plan(xyxy, [f"{i}" for i in range(b.shape[0])], (w, h))
    # `frame_dev`: the caller's own uint8 [H,W,3] device copy of the screenshot (the batch route uploads one per request): drawn on
    # in place, no second upload
    frame = frame_dev if frame_dev is not None else torch.from_numpy(np.array(image_np, order="C")).to(device)
    render_device(frame, cmds)
    if stored:                                         # stored-deflate PNG (pixels + 0.02 %); default: the run-length deflate stream
        _, b64 = png_pack_device(frame)
        text = b64.cpu().numpy().tobytes()
    else:
        _, b64, meta = png_deflate_device(frame)
        n = int(meta[2].item())                        # the one synchronising read: the base64 length decided on the device
        text = b64[:n].cpu().numpy().tobytes()
    return text.decode("ascii"), {f"{phrase}": v for phrase, v in zip(phrases, xywh)}


class AnnotateScratch:
    """Device buffers of the batched overlay + PNG tail for B frames of H x W (about 60 MB per 1080p frame: the annotated frames,
    the filtered stream, the unit slots, 25 MB of tokens, the PNG and its base64), every one [B][per-frame capacity] as the
    frame-batched OMNI_OP_PNG_DEFLATE (i5 = 2) lays them out.  A caller that annotates batch after batch keeps one (or two,
    alternating, when the next batch is queued before this one is read back) instead of allocating per call."""

    def __init__(self, B, H, W, device):
        u = H * (3 * W + 1)
        units, units_lz = (u + 4095) // 4096, (u + 32767) // 32768
        self.B, self.H, self.W = B, H, W
        self.cap = u + 5 * units + 63
        nseg = (self.cap - 53 + 4095) // 4096
        e = lambda shape, dt=torch.uint8: torch.empty(shape, dtype=dt, device=device)
        self.frames = e((B, H, W, 3))
        self.png, self.filt, self.slots = e((B, self.cap)), e((B, u)), e((B, units_lz * 33792))
        self.meta, self.part = e((B, 4 + 2 * units), torch.int32), e((B, 2 * H + nseg), torch.int32)
        self.b64, self.toks = e((B, 4 * ((self.cap + 2) // 3))), e((B, units_lz * 32768), torch.int32)
        self.table = None                                  # the last overlay upload (alive until the next launch on this scratch)

    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in (self.frames, self.png, self.filt, self.slots, self.meta, self.part, self.b64, self.toks))


def png_deflate_device_batch(frames_bhwc: torch.Tensor, want_b64=True, stream=None, scratch: Optional[AnnotateScratch] = None):
    """`png_deflate_device(lz=True)` of B equal-sized frames (uint8 [B,H,W,3], contiguous) in the nine launches of one: the
    frame-batched OMNI_OP_PNG_DEFLATE (i5 = 2), B times the unit lanes in flight.  Every file is oracle/png_ref.py::deflate_png_lz of
    its frame.  -> (PNG [B, capacity], base64 [B, 4 ceil(capacity / 3)] or None, meta [B, words]) device tensors, a row per frame:
    meta[f, 1] = file bytes, meta[f, 2] = base64 bytes of frame f."""
    assert frames_bhwc.dtype == torch.uint8 and frames_bhwc.is_contiguous() and frames_bhwc.dim() == 4 and frames_bhwc.shape[3] == 3
    B, H, W = frames_bhwc.shape[:3]
    sc = scratch if scratch is not None else AnnotateScratch(B, H, W, frames_bhwc.device)
    assert (sc.B, sc.H, sc.W) == (B, H, W)
    L.launch(L.make_op(L.OP_PNG_DEFLATE, L.F32,
                       p=[frames_bhwc.data_ptr(), sc.png.data_ptr(), sc.filt.data_ptr(), sc.slots.data_ptr(), sc.meta.data_ptr(),
                          sc.part.data_ptr(), sc.b64.data_ptr() if want_b64 else None, sc.toks.data_ptr()],
                       i={0: H, 1: W, 2: sc.cap, 3: sc.meta.shape[1], 4: sc.part.shape[1], 5: 2, 6: B}), stream)
    return sc.png, (sc.b64 if want_b64 else None), sc.meta


def annotate_encode_device_batch_launch(frames, boxes_per_frame, phrases_per_frame, text_scale=0.4, text_padding=5, text_thickness=2,
                                        thickness=3, stream=None, scratch: Optional[AnnotateScratch] = None):
    """Queue `annotate_encode_device` of B equal-sized frames on `stream` (None: the current one) without reading anything back:
    the layout per frame on the host, ONE overlay launch (out of place: `frames`, uint8 [H,W,3] device tensors, are only read) and
    ONE deflate chain.  boxes_per_frame: cxcywh ratio tensors; phrases_per_frame: the label-coordinate keys.  -> handle for
    `annotate_encode_device_batch_finish`."""
    from .overlay import BoxAnnotator, render_device_batch
    B = len(frames)
    h, w = frames[0].shape[:2]
    ann = BoxAnnotator(text_scale=text_scale, text_padding=text_padding, text_thickness=text_thickness, thickness=thickness)
    cmds_all, coords = [], []
    for boxes, phrases in zip(boxes_per_frame, phrases_per_frame):
        b = boxes * torch.Tensor([w, h, w, h])
        cx, cy, bw, bh = b.unbind(-1)
        xyxy = torch.stack((cx - 0.5 * bw, cy - 0.5 * bh, cx + 0.5 * bw, cy + 0.5 * bh), -1).numpy()
        xywh = torch.stack((cx - 0.5 * bw, cy - 0.5 * bh, bw, bh), -1).numpy()
        cmds_all.append(ann.plan(xyxy, [f"{i}" for i in range(b.shape[0])], (w, h)))
        coords.append({f"{phrase}": v for phrase, v in zip(phrases, xywh)})
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        sc = scratch if scratch is not None else AnnotateScratch(B, h, w, frames[0].device)
        sc.table = render_device_batch(frames, sc.frames, cmds_all, stream)
        _, b64, meta = png_deflate_device_batch(sc.frames, stream=stream, scratch=sc)
    return (sc, b64, meta, coords, stream, list(frames))


def annotate_encode_device_batch_finish(handle):
    """-> [(base64 str, label_coordinates)] per frame: ONE synchronising read of the B meta rows (the sizes decided on the device),
    then the B base64 slices."""
    sc, b64, meta, coords, stream, _frames = handle
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        sizes = meta[:, :4].cpu()
        texts = [b64[f, :int(sizes[f, 2])].cpu() for f in range(len(coords))]
    return [(t.numpy().tobytes().decode("ascii"), c) for t, c in zip(texts, coords)]


def annotate_encode_device_batch(frames, boxes_per_frame, phrases_per_frame, **kw):
    """`annotate_encode_device` for B equal-sized device frames, batched on the device: one overlay launch and one deflate chain for
    all of them, one read-back of their sizes.  Same layout, pixels, file bytes and label coordinates per frame; the frames
    themselves are not drawn on.  -> [(base64 str, label_coordinates)]."""
    return annotate_encode_device_batch_finish(annotate_encode_device_batch_launch(frames, boxes_per_frame, phrases_per_frame, **kw))


def get_som_labeled_img(image_source: Union[str, Image.Image], model=None, BOX_TRESHOLD=0.01, output_coord_in_ratio=False,
                        ocr_bbox=None, text_scale=0.4, text_padding=5, draw_bbox_config=None, caption_model_processor=None,
                        ocr_text=[], use_local_semantics=True, iou_threshold=0.9, prompt=None, scale_img=False, imgsz=None,
                        batch_size=128, caption_confidence=False, max_new_tokens=None, generation=None, caption_vocabulary=None):
    """ref:util/utils.py:417-496 — returns (base64 PNG, label_coordinates, filtered_boxes_elem).
    caption_confidence (or a caption model with `token_scores` set): every element whose content the captioner wrote gains
    "confidence", see `florence.caption_confidence`; OCR elements and icons that took OCR text have no such key.
    max_new_tokens: tokens generated per captioned icon, None = 20 (`get_parsed_content_icon`).
    generation: generation controls of the icon captions, None = none (`get_parsed_content_icon`).
    caption_vocabulary: a closed set of icon captions (strings or token id lists), None = free text (`get_parsed_content_icon`'s
    `vocabulary`): every captioned icon's content is one of them."""
    if isinstance(image_source, str):
        image_source = Image.open(image_source)
    image_source = image_source.convert("RGB")
    w, h = image_source.size
    if not imgsz:
        imgsz = (h, w)
    xyxy, logits, phrases = predict_yolo(model=model, image=image_source, box_threshold=BOX_TRESHOLD, imgsz=imgsz,
                                         scale_img=scale_img, iou_threshold=0.1)
    xyxy = xyxy.cpu() / torch.Tensor([w, h, w, h])       # f32 divide, as the reference (on its device)
    image_np = np.asarray(image_source)
    if ocr_bbox:
        ocr_bbox = (torch.tensor(ocr_bbox) / torch.Tensor([w, h, w, h])).tolist()
    else:
        ocr_bbox, ocr_text = [], []        # the reference raises TypeError here (zip(None, ...)); we tolerate it
    ocr_elems = [{"type": "text", "bbox": box, "interactivity": False, "content": txt, "source": "box_ocr_content_ocr"}
                 for box, txt in zip(ocr_bbox, ocr_text) if int_box_area(box, w, h) > 0]
    icon_elems = [{"type": "icon", "bbox": box, "interactivity": True, "content": None}
                  for box in xyxy.tolist() if int_box_area(box, w, h) > 0]
    filtered = remove_overlap_new(boxes=icon_elems, iou_threshold=iou_threshold, ocr_bbox=ocr_elems)
    if not ocr_elems:   # reference returns bare boxes in that (crashing) configuration; normalise to elements
        filtered = [e if isinstance(e, dict) else {"type": "icon", "bbox": e, "interactivity": True, "content": None,
                                                    "source": "box_yolo_content_yolo"} for e in filtered]
    elems = sorted(filtered, key=lambda x: x["content"] is None)
    starting_idx = next((i for i, box in enumerate(elems) if box["content"] is None), -1)
    filtered_boxes = torch.tensor([box["bbox"] for box in elems]).reshape(-1, 4)
    if use_local_semantics:
        conf = bool(caption_confidence or getattr(caption_model_processor["model"], "token_scores", False))
        parsed = get_parsed_content_icon(filtered_boxes, starting_idx, image_np, caption_model_processor, prompt=prompt,
                                         batch_size=batch_size, **({"return_confidence": True} if conf else {}),
                                         **({"max_new_tokens": max_new_tokens} if max_new_tokens is not None else {}),
                                         **({"generation": generation} if generation is not None else {}),
                                         **({"vocabulary": caption_vocabulary} if caption_vocabulary is not None else {}))
        for box in elems:
            if box["content"] is None and parsed:
                if conf:
                    box["content"], box["confidence"] = parsed.pop(0)
                else:
                    box["content"] = parsed.pop(0)
    boxes_cxcywh = _box_convert_xyxy_to_cxcywh(filtered_boxes)
    phrases = [i for i in range(len(boxes_cxcywh))]
    if os.environ.get("OMNI_SKIP_ANNOTATE", "0") == "1":
        encoded = ""
        label_coordinates = {f"{i}": v for i, v in enumerate(
            torch.stack((filtered_boxes[:, 0] * w, filtered_boxes[:, 1] * h, (filtered_boxes[:, 2] - filtered_boxes[:, 0]) * w,
                         (filtered_boxes[:, 3] - filtered_boxes[:, 1]) * h), -1).numpy())} if len(filtered_boxes) else {}
    else:
        cfg = draw_bbox_config or {"text_scale": text_scale, "text_padding": text_padding}
        if overlay_on_device(getattr(model, "device", None)):        # raster + PNG + base64 on the MI355X (csrc/overlay_png.hip)
            encoded, label_coordinates = annotate_encode_device(image_np, boxes_cxcywh, phrases, model.device, **cfg)
        else:
            frame, label_coordinates = annotate(image_source=image_np, boxes=boxes_cxcywh, logits=logits, phrases=phrases, **cfg)
            encoded = encode_png_b64(frame)
    if output_coord_in_ratio:
        label_coordinates = {k: [v[0] / w, v[1] / h, v[2] / w, v[3] / h] for k, v in label_coordinates.items()}
    return encoded, label_coordinates, elems

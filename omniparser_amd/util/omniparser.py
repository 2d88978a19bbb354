"""`Omniparser` facade of the MI355X path.

Mirrors the public contract of ref:util/omniparser.py:7-32 — the same config keys (`som_model_path`,
`caption_model_name`, `caption_model_path`, `BOX_TRESHOLD`), `parse(image_base64) -> (labeled_png_b64,
parsed_content_list)` — on top of the gfx950 detector / captioner adapters.  OCR is not part of the hot
path: an optional `ocr_provider` in the config supplies `(texts, xyxy_px_boxes)` — a callable,
or "florence" for the caption model's own `<OCR_WITH_REGION>` reading (utils.FlorenceOCR); without it the
screenshot is parsed with icons only, exactly what the reference produces when its OCR engine returns nothing.
"""
import base64
import io
from typing import Callable, Dict, Optional, Sequence, Tuple

import numpy as np
import torch
from PIL import Image

from . import utils as U

# ref:util/omniparser.py:21-27 — overlay geometry grows linearly with the longer image side, 3200 px == 1.0
_OVERLAY_REF_SIDE = 3200
_OVERLAY_BASE = (("text_scale", 0.8, None), ("text_thickness", 2, 1), ("text_padding", 3, 1), ("thickness", 3, 1))
# fixed arguments the reference facade passes down (ref:util/omniparser.py:29-30)
_OCR_ARGS = dict(display_img=False, output_bb_format="xyxy", easyocr_args={"text_threshold": 0.8}, use_paddleocr=False)
_SOM_ARGS = dict(output_coord_in_ratio=True, use_local_semantics=True, iou_threshold=0.7, scale_img=False, batch_size=128)


def overlay_style(image_size: Tuple[int, int]) -> Dict[str, float]:
    """Annotation style for an image of `image_size` (w, h): integer fields are floored and clamped to >= 1."""
    ratio = max(image_size) / _OVERLAY_REF_SIDE
    return {name: (base * ratio if floor is None else max(int(base * ratio), floor)) for name, base, floor in _OVERLAY_BASE}


def decode_image(image_base64: str) -> Image.Image:
    return Image.open(io.BytesIO(base64.b64decode(image_base64)))


class Omniparser(object):
    def __init__(self, config: Dict):
        self.config = config
        device = "cuda" if torch.cuda.is_available() else "cpu"     # "cpu" makes the adapters raise: no CPU fallback
        self.som_model = U.get_yolo_model(model_path=config.get("som_model_path"), device=device)
        self.caption_model_processor = U.get_caption_model_processor(
            model_name=config["caption_model_name"], model_name_or_path=config["caption_model_path"], device=device)
        self.ocr_provider: Optional[Callable] = config.get("ocr_provider")
        # ocr_provider: None (no OCR of its own), a callable image -> (texts, xyxy px boxes), or "florence": the caption model reads
        # the screenshot itself (utils.FlorenceOCR over this object's caption model: <OCR_WITH_REGION> over tiles of the captioner's
        # resolution; it needs the tokenizer.json next to the checkpoint).  ocr_max_new_tokens (tokens per tile, default 1024),
        # ocr_overlap (pixels shared by neighbouring tiles, default 128), ocr_min_confidence (0..1, default 0) and ocr_generation
        # (generation controls of the reading, as caption_generation) belong to it; ranges the captioner knows are checked per call.
        ocr_keys = {k: config[k] for k in ("ocr_max_new_tokens", "ocr_overlap", "ocr_min_confidence", "ocr_generation") if config.get(k) is not None}
        if isinstance(self.ocr_provider, str):
            if self.ocr_provider != "florence":
                raise ValueError(f"ocr_provider must be None, a callable or \"florence\", got {self.ocr_provider!r}")
            for k, lo in (("ocr_max_new_tokens", 1), ("ocr_overlap", 0)):
                v = ocr_keys.get(k)
                if v is not None and (isinstance(v, bool) or not isinstance(v, int) or v < lo):
                    raise ValueError(f"{k} must be an integer >= {lo}, got {v!r}")
            mc = ocr_keys.get("ocr_min_confidence")
            if mc is not None and (isinstance(mc, bool) or not isinstance(mc, (int, float)) or not 0.0 <= mc <= 1.0):
                raise ValueError(f"ocr_min_confidence must be a number in 0..1, got {mc!r}")
            if "ocr_generation" in ocr_keys:
                from ..florence import GenerationControls
                if not isinstance(ocr_keys["ocr_generation"], dict):
                    raise ValueError(f"ocr_generation must be a dict of generation controls or None, got {ocr_keys['ocr_generation']!r}")
                GenerationControls.of(ocr_keys["ocr_generation"])
            self.ocr_provider = U.FlorenceOCR(self.caption_model_processor, **{k[4:]: v for k, v in ocr_keys.items()})
        elif ocr_keys:
            raise ValueError(f"{sorted(ocr_keys)} belong to ocr_provider=\"florence\"")
        elif self.ocr_provider is not None and not callable(self.ocr_provider):
            raise ValueError(f"ocr_provider must be None, a callable or \"florence\", got {self.ocr_provider!r}")
        # crop resolution of the captioner: 768 = the reference's CPU branch (bicubic to 768x768; the parity target and the
        # default here), 64 = its cuda branch (do_resize=False, ref:util/utils.py:120-121).  An explicit choice, not a device side effect.
        if config.get("caption_resolution") is not None:
            res = int(config["caption_resolution"])
            if res not in (64, 768):
                raise ValueError(f"caption_resolution must be 64 or 768, got {res}")
            self.caption_model_processor["model"].resolution = res
        # beam width of the captioner's decoder: 1 (default) = greedy, the reference's call (ref:util/utils.py:125); 2..8 = beam
        # search, the best hypothesis per crop.  Like caption_resolution, an explicit choice set on the caption model.
        if config.get("caption_num_beams") is not None:
            nb = config["caption_num_beams"]
            if isinstance(nb, bool) or not isinstance(nb, int) or not 1 <= nb <= 8:
                raise ValueError(f"caption_num_beams must be an integer in 1..8, got {nb!r}")
            self.caption_model_processor["model"].num_beams = nb
        # caption_confidence: True = every captioned icon of parsed_content_list gains "confidence" (florence.caption_confidence of the
        # greedy tokens' log-probabilities, computed on the device next to the arg-max).  Greedy decoding only.
        if config.get("caption_confidence") is not None:
            cc = config["caption_confidence"]
            if not isinstance(cc, bool):
                raise ValueError(f"caption_confidence must be a bool, got {cc!r}")
            self.caption_model_processor["model"].token_scores = cc
        # caption_max_new_tokens: tokens generated per captioned icon (default 20, the reference's call).  With a caption prompt that
        # asks for more than a label, a larger value gives per-icon descriptions; the captioner refuses what its decoder cannot hold.
        self.caption_max_new_tokens = 20
        if "caption_max_new_tokens" in config:
            mn = config["caption_max_new_tokens"]
            if isinstance(mn, bool) or not isinstance(mn, int) or mn < 1:
                raise ValueError(f"caption_max_new_tokens must be an integer >= 1, got {mn!r}")
            self.caption_max_new_tokens = mn
        # caption_generation: a dict of generation controls for the icon captions and `describe` (repetition_penalty,
        # no_repeat_ngram_size, min_new_tokens, suppress_tokens, begin_suppress_tokens, bad_words_ids — Florence2Captioner.generate);
        # None (default) = the calls as they were.  Types and limits are checked here, ids against the vocabulary by the captioner.
        self.caption_generation = None
        if config.get("caption_generation") is not None:
            from ..florence import GenerationControls
            cg = config["caption_generation"]
            if not isinstance(cg, dict):
                raise ValueError(f"caption_generation must be a dict of generation controls or None, got {cg!r}")
            GenerationControls.of(cg)
            self.caption_generation = dict(cg)
        # caption_vocabulary: a closed set of icon captions — a list of strings (tokenised per call by the caption processor, which
        # needs the tokenizer.json next to the checkpoint) or of token id lists ([forced BOS] text EOS): every captioned icon's content
        # is then exactly one of them, picked by one greedy decode on the device (Florence2Captioner.generate(vocabulary=...)).  None
        # (default) = free text.  Types and limits are checked here, ids against the model by the captioner.  Not together with
        # caption_generation or caption_num_beams > 1: the captioner refuses both.
        self.caption_vocabulary = None
        if config.get("caption_vocabulary") is not None:
            from ..florence import CaptionVocabulary
            cv = config["caption_vocabulary"]
            if not isinstance(cv, (list, tuple)) or not cv:
                raise ValueError(f"caption_vocabulary must be a non-empty list of strings or token id lists, or None; got {cv!r}")
            for entry in cv:
                if isinstance(entry, str):
                    if not entry.strip():
                        raise ValueError("caption_vocabulary: an empty string")
                elif not isinstance(entry, (list, tuple)):
                    raise ValueError(f"caption_vocabulary: an entry is a string or a list of token ids, got {entry!r}")
            id_rows = [e for e in cv if not isinstance(e, str)]
            if id_rows:
                CaptionVocabulary(id_rows)
            if self.caption_generation is not None:
                raise ValueError("caption_vocabulary cannot be combined with caption_generation: a closed vocabulary is decoded without "
                                 "generation controls")
            self.caption_vocabulary = list(cv)

    def _ocr(self, image: Image.Image, ocr=None):
        """`ocr` = (texts, xyxy px boxes) handed over by the caller for THIS image; else the configured provider."""
        found = ocr if ocr is not None else (self.ocr_provider(image) if self.ocr_provider is not None else None)
        (texts, boxes), _ = U.check_ocr_box(image, ocr_result=found, **_OCR_ARGS)
        return texts, boxes

    def parse_image(self, image: Image.Image, ocr=None):
        texts, boxes = self._ocr(image, ocr)
        labeled, _coords, elements = U.get_som_labeled_img(
            image, self.som_model, BOX_TRESHOLD=self.config["BOX_TRESHOLD"], ocr_bbox=boxes, ocr_text=texts,
            draw_bbox_config=overlay_style(image.size), caption_model_processor=self.caption_model_processor, **_SOM_ARGS,
            **({"max_new_tokens": self.caption_max_new_tokens} if self.caption_max_new_tokens != 20 else {}),
            **({"generation": self.caption_generation} if self.caption_generation is not None else {}),
            **({"caption_vocabulary": self.caption_vocabulary} if self.caption_vocabulary is not None else {}))
        return labeled, elements

    def describe(self, image_base64: str, task="<MORE_DETAILED_CAPTION>", max_new_tokens=256, generation=None):
        """`utils.describe_image` of the whole screenshot: one description (or, with task="<OCR>", the text) from the caption model
        alone — no detector, no OCR engine.  generation: a dict of generation controls for this call; None = the configured
        `caption_generation` (default: none)."""
        generation = self.caption_generation if generation is None else generation
        return U.describe_image(decode_image(image_base64), self.caption_model_processor, task=task, max_new_tokens=max_new_tokens,
                                **({"generation": generation} if generation is not None else {}))

    def parse(self, image_base64: str, ocr=None):
        return self.parse_image(decode_image(image_base64), ocr)

    def ground(self, image_base64: str, queries, top_k=5):
        """`parse`, then `utils.rank_elements` of the parsed elements: (parsed_content_list, per query the top_k elements as
        {"index", "score"} by descending likelihood of the query under the caption model).  queries: strings (they need the
        checkpoint's tokenizer.json) or token-id lists."""
        image = decode_image(image_base64)
        _labeled, elements = self.parse_image(image)
        rankings = U.rank_elements(np.asarray(image.convert("RGB")), elements, self.caption_model_processor, queries, top_k=top_k)
        return elements, rankings

    def locate(self, image_base64: str, phrases, **kw):
        """`utils.locate` of the screenshot: where are `phrases` (a phrase or a list; None for the box tasks without text,
        task=...)?  Boxes in frame pixels, [{"label", "query", "bbox", "confidence", "tile", "phrase"}], from the caption model alone
        — no detector, no OCR engine.  kw: `utils.locate`'s (task, max_new_tokens, overlap, min_confidence, banned_phrases,
        generation, return_stats)."""
        return U.locate(np.asarray(decode_image(image_base64).convert("RGB")), self.caption_model_processor, text=phrases, **kw)

    def segment(self, image_base64: str, phrases=None, regions=None, **kw):
        """`utils.segment` of the screenshot: the shape of `phrases` (a phrase or a list) or of what the boxes `regions` (frame
        pixels) hold — polygons, bit masks and a click point that lies on the shape, from the caption model alone.  kw:
        `utils.segment`'s (max_new_tokens, overlap, min_confidence, instances, return_masks, generation, return_stats)."""
        return U.segment(np.asarray(decode_image(image_base64).convert("RGB")), self.caption_model_processor, text=phrases, regions=regions, **kw)

    def find_similar(self, image_base64: str, exemplars_base64, top_k=5):
        """`parse`, then `utils.match_elements` of the parsed elements against exemplar images (base64, as the screenshot is):
        (parsed_content_list, per exemplar the top_k elements as {"index", "score"} by descending cosine similarity of the caption
        model's visual embeddings).  The sibling of `ground`: that one asks with a text, this one with a picture."""
        if isinstance(exemplars_base64, (str, bytes)):
            raise ValueError("exemplars_base64 is a list of base64 images")
        image = decode_image(image_base64)
        exemplars = [np.asarray(decode_image(b).convert("RGB")) for b in exemplars_base64]
        _labeled, elements = self.parse_image(image)
        matches = U.match_elements(np.asarray(image.convert("RGB")), elements, self.caption_model_processor, exemplars, top_k=top_k)
        return elements, matches

    def parse_many(self, images_base64: Sequence[str]):
        """Service helper: parse several screenshots with the same models (sequentially; the batched device path
        for equally sized frames is `omniparser_amd.pipeline.ScreenParser.parse_batch`)."""
        return [self.parse(b) for b in images_base64]

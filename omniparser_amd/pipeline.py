"""Batched screen parser: B screenshots -> parsed elements, everything model-side on device.

The reference parses one screenshot at a time (ref:util/omniparser.py:16-32).  Screenshots are
independent units, so here a batch is parsed as: ONE detector graph over all B frames -> host glue per
frame (the reference's list semantics, util/utils.py) -> the crops of ALL frames packed into 128-crop
caption micro-batches (ref batch_size=128) -> on-device greedy decode.  Results equal a per-frame
`get_som_labeled_img(...)[2]` call (same functions underneath); only the packing differs.
"""
import contextlib
import os
from types import SimpleNamespace
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from .florence import Florence2Captioner, caption_confidence
from .util import utils as U
from .util.yolov9 import YOLOv9Detector


OCR_CAP = 1024           # OMNI_OP_GLUE capacities (csrc/glue_ops.hip)
MASK_WORDS = OCR_CAP // 64


def _f64_bits(x: float):
    import struct
    lo, hi = struct.unpack("<ii", struct.pack("<d", float(x)))
    return lo, hi


class _GlueState:
    """Device side of the detect -> caption hand-off for one detector plan (batch B): fixed buffers + one small plan of B
    OMNI_OP_GLUE ops replayed right behind the detector graph on the detector's stream."""

    def __init__(self, dp, det, iw, ih, thr):
        dev, B, md = det.device, dp.batch, dp.out_boxes.shape[1]
        self.B, self.md = B, md
        with torch.cuda.stream(det.stream):
            self.ocr = torch.zeros(B, OCR_CAP, 4, dtype=torch.float64, device=dev)
            self.meta = torch.zeros(B, 2 + 2 * OCR_CAP, dtype=torch.int32, device=dev)
            self.elems = torch.zeros(B, md + OCR_CAP, 2, dtype=torch.int32, device=dev)
            self.crops = torch.zeros(B, md, 4, dtype=torch.int32, device=dev)
            self.counts = torch.zeros(B, 4, dtype=torch.int32, device=dev)
            self.donors = torch.zeros(B, md, MASK_WORDS, dtype=torch.int64, device=dev)
        self.h_ocr = torch.zeros(B, OCR_CAP, 4, dtype=torch.float64)          # host staging of the per-frame OCR tables (a few KB)
        self.h_meta = torch.zeros(B, 2 + 2 * OCR_CAP, dtype=torch.int32)
        lo, hi = _f64_bits(thr)
        ops = [L.make_op(L.OP_GLUE, L.F32,
                         p=[dp.out_boxes[b].data_ptr(), dp.out_count[b:].data_ptr(), self.ocr[b].data_ptr(), self.meta[b].data_ptr(),
                            self.elems[b].data_ptr(), self.crops[b].data_ptr(), self.counts[b].data_ptr(), self.donors[b].data_ptr()],
                         i={0: md, 1: OCR_CAP, 2: iw, 3: ih, 4: MASK_WORDS, 5: 0, 6: md + OCR_CAP, 7: 1, 8: lo, 9: hi})
               for b in range(B)]
        # detector ops AND hand-off ops as ONE plan, captured as ONE hipGraph (kernel nodes only): one launch per batch.  Round 2
        # saw the second replay of the detector graph stall whenever hand-off kernels followed it; the detector graph then held a
        # hipMemsetAsync node (the candidate-counter reset of OMNI_OP_DETECT_DECODE).  With that reset done by a kernel both
        # arrangements ran 100 consecutive replays on the MI355X with the host twin's results (profiles/r3_s1_handoff_graph_replays.jsonl)
        self.plan = L.Plan(list(dp.plan.ops) + ops)
        det.stream.synchronize()
        if det.use_graph:
            self.plan.run(det.stream)
            det.stream.synchronize()
            self.plan.capture(det.stream)
            det.stream.synchronize()

    def launch(self, det):
        if det.use_graph:
            self.plan.replay(det.stream)
        else:
            self.plan.run(det.stream)


class ScreenParser:
    def __init__(self, detector: YOLOv9Detector, captioner: Florence2Captioner, processor=None,
                 box_threshold=0.05, iou_threshold=0.7, nms_iou=0.1, max_det=300, imgsz=640, batch_size=128,
                 tile_large=False):
        self.det, self.cap = detector, captioner
        self.tile_large = tile_large      # False = reference behaviour (whole frame letterboxed to `imgsz`)
        # detect -> caption hand-off ON THE DEVICE (csrc/glue_ops.hip, inside the detector's graph): boxes never visit the host between
        # the stages.  OMNI_DEVICE_GLUE=0 = the host twin (`glue`: the reference's list code), also taken automatically for inputs
        # beyond the kernel's capacities (more than 512 detections or 1024 OCR boxes per frame)
        self.device_glue = os.environ.get("OMNI_DEVICE_GLUE", "1") != "0" and max_det <= 512
        self.proc = processor or (U.FlorenceProcessor(captioner.w.dir) if captioner is not None else None)
        self.box_threshold, self.iou_threshold, self.nms_iou = box_threshold, iou_threshold, nms_iou
        self.max_det, self.imgsz, self.batch_size = max_det, imgsz, max(1, min(int(batch_size), 128))   # caption plan capacity
        self.max_new_tokens = 20          # ref:util/utils.py:125 generate(max_new_tokens=20)
        self.encode_lanes = 2             # parse_stream: caption micro-batches in flight at once (HIP streams; 1 = one after the other)
        self._ev = {}                     # HIP events of the last parse_batch (stage boundaries on the streams the stages run on)
        self.stats = {}

    # ---- stage 1: detector over the whole batch (one graph launch)
    @torch.inference_mode()
    def detect(self, frames: Sequence[torch.Tensor], pad_to: Optional[int] = None):
        """`pad_to`: run the plan of that batch size even for fewer frames (the unused slots keep whatever they held
        and their results are ignored) — streams with ragged batches then need ONE plan per resolution."""
        ih, iw = frames[0].shape[:2]
        dp = self.det.get_plan(iw, ih, self.imgsz, self.box_threshold, self.nms_iou, self.max_det, batch=max(len(frames), pad_to or 0))
        self.det.stream.wait_stream(torch.cuda.current_stream(frames[0].device))     # frames the caller is still producing on its stream
        with torch.cuda.stream(self.det.stream):
            for bi, f in enumerate(frames):
                dp.img[bi].copy_(f, non_blocking=True)
            dp.launch(self.det)
            counts = dp.out_count.cpu()                     # sync
            boxes = dp.out_boxes.cpu()
        return [boxes[bi, : int(counts[bi])] for bi in range(len(frames))]

    # ---- stage 1b: tiled detection for frames larger than 1080p (BASELINE configs[4]; policy is OURS, the
    #      reference letterboxes the whole image: SURVEY 0.7).  Tiles overlap by 64 px, each tile goes through the
    #      ordinary detector (one batch), boxes are shifted back and a global batched_nms(nms_iou)[:max_det] + clamp
    #      merges them (same NMS kernel as inside the detector).  oracle/tiling_ref.py is the CPU statement.
    @staticmethod
    def tile_origins(iw, ih, tile_w=1952, tile_h=1112, overlap=64):
        def axis(n, t):
            if n <= t:
                return [0]
            k = -(-(n - overlap) // (t - overlap))
            step = (n - t) / (k - 1)
            return [int(round(i * step)) for i in range(k)]
        return [(x, y) for y in axis(ih, tile_h) for x in axis(iw, tile_w)], min(tile_w, iw), min(tile_h, ih)

    @torch.inference_mode()
    def detect_tiled(self, frame: torch.Tensor):
        ih, iw = frame.shape[:2]
        origins, tw, th = self.tile_origins(iw, ih)
        dp = self.det.get_plan(tw, th, self.imgsz, self.box_threshold, self.nms_iou, self.max_det, batch=len(origins))
        # The detector's stream is a NON-BLOCKING stream: nothing orders it behind work the caller queued on its own (current) stream.
        # Rounds 2-5 cut the tiles with `.contiguous()` on the CALLER's stream and copied them into the plan on the detector's — a
        # race a few microseconds wide that the round-6 closing check lost once in six suite runs (two `detect_tiled` calls on the same
        # frame returned different boxes).  Now the detector's stream first waits for everything the caller has queued (the frame itself
        # may still be in flight, e.g. a service's upload), and the tiles are cut ON it.
        self.det.stream.wait_stream(torch.cuda.current_stream(frame.device))
        with torch.cuda.stream(self.det.stream):
            tiles = [frame[y:y + th, x:x + tw].contiguous() for (x, y) in origins]
            for bi, t in enumerate(tiles):
                dp.img[bi].copy_(t, non_blocking=True)
            dp.launch(self.det)
            counts = dp.out_count.cpu()
            boxes, scores, cls = dp.out_boxes.cpu(), dp.out_scores.cpu(), dp.out_cls.cpu()
        recs = []
        for bi, (x0, y0) in enumerate(origins):
            k = int(counts[bi])
            b = boxes[bi, :k].numpy() + np.asarray([x0, y0, x0, y0], dtype=np.float32)
            r = np.zeros((k, 8), dtype=np.float32)
            r[:, :4] = b
            r[:, 4] = scores[bi, :k].numpy()
            ri = r.view(np.int32)
            ri[:, 5] = cls[bi, :k].numpy()
            recs.append(r)
        rec = np.concatenate(recs, 0) if recs else np.zeros((0, 8), dtype=np.float32)
        n = rec.shape[0]
        rec.view(np.int32)[:, 6] = np.arange(n)               # stable tie-break = concatenation order (tile-major)
        dev = self.det.device
        cap_n = max(n, 1)
        with torch.cuda.stream(self.det.stream):               # scratch is created AND consumed on the detector's stream
            cand = torch.from_numpy(np.concatenate([rec, np.zeros((cap_n - n, 8), dtype=np.float32)], 0)).to(dev)
            count = torch.tensor([n], dtype=torch.int32, device=dev)
            srt = torch.zeros((cap_n + 1) * 8, dtype=torch.float32, device=dev)
            mask = torch.empty(cap_n * ((cap_n + 63) // 64), dtype=torch.int64, device=dev)
            ob = torch.zeros(self.max_det, 4, device=dev); osc = torch.zeros(self.max_det, device=dev)
            oc = torch.zeros(self.max_det, dtype=torch.int32, device=dev); on = torch.zeros(1, dtype=torch.int32, device=dev)
            op = L.make_op(L.OP_NMS, L.F32, p=[cand.data_ptr(), count.data_ptr(), srt.data_ptr(), mask.data_ptr(), ob.data_ptr(),
                                              osc.data_ptr(), oc.data_ptr(), on.data_ptr()],
                           i={0: cap_n, 1: self.max_det, 2: iw, 3: ih}, f={0: self.nms_iou})
            L.launch(op, self.det.stream)
            k = int(on.cpu())
            return ob[:k].cpu(), osc[:k].cpu(), oc[:k].cpu().long()

    # ---- stage 2: host glue (reference semantics) -> elements + crop boxes
    def glue(self, xyxy_px: torch.Tensor, w: int, h: int, ocr_bbox, ocr_text):
        xyxy = xyxy_px / torch.Tensor([w, h, w, h])
        if ocr_bbox:
            ocr_r = (torch.tensor(ocr_bbox) / torch.Tensor([w, h, w, h])).tolist()
        else:
            ocr_r, ocr_text = [], []
        ocr_el = [{"type": "text", "bbox": b, "interactivity": False, "content": t, "source": "box_ocr_content_ocr"}
                  for b, t in zip(ocr_r, ocr_text) if U.int_box_area(b, w, h) > 0]
        icon_el = [{"type": "icon", "bbox": b, "interactivity": True, "content": None}
                   for b in xyxy.tolist() if U.int_box_area(b, w, h) > 0]
        filtered = U.remove_overlap_new(boxes=icon_el, iou_threshold=self.iou_threshold, ocr_bbox=ocr_el)
        if not ocr_el:
            filtered = [e if isinstance(e, dict) else {"type": "icon", "bbox": e, "interactivity": True, "content": None,
                                                        "source": "box_yolo_content_yolo"} for e in filtered]
        elems = sorted(filtered, key=lambda x: x["content"] is None)
        start = next((i for i, b in enumerate(elems) if b["content"] is None), -1)
        boxes = [e["bbox"] for e in elems]
        non_ocr = boxes[start:] if start else boxes        # ref:util/utils.py:92-95 quirk kept
        return elems, U.crop_boxes_px(non_ocr, w, h)

    # ---- stage 2': the same hand-off on the device.  Host work before the launch touches the OCR list only (its ratio
    #      boxes, int_box_area filter and dict-equality classes do not depend on the detector); after the launch the host
    #      reads four counters per frame, and builds the element dicts at the very end from the device tables.
    @staticmethod
    def ocr_elements(w, h, ocr_bbox, ocr_text):
        if ocr_bbox:
            ocr_r = (torch.tensor(ocr_bbox) / torch.Tensor([w, h, w, h])).tolist()
        else:
            ocr_r, ocr_text = [], []
        return [{"type": "text", "bbox": b, "interactivity": False, "content": t, "source": "box_ocr_content_ocr"}
                for b, t in zip(ocr_r, ocr_text) if U.int_box_area(b, w, h) > 0]

    @torch.inference_mode()
    def detect_glue(self, frames, ocr, pad_to=None, snapshot=False):
        """snapshot: the tables the rest of the batch reads (detector outputs, element table, donor masks, crop rectangles: ~0.5 MB)
        are copied behind the graph on the detector's stream and returned instead of the plan's own buffers, so the NEXT batch's
        detector pass may overwrite those while this batch is still being captioned (parse_stream)."""
        ih, iw = frames[0].shape[:2]
        det = self.det
        dp = det.get_plan(iw, ih, self.imgsz, self.box_threshold, self.nms_iou, self.max_det, batch=max(len(frames), pad_to or 0))
        ocr_els = [self.ocr_elements(iw, ih, *(reversed(ocr[fi]) if ocr is not None else ([], []))) for fi in range(len(frames))]
        if any(len(els) > OCR_CAP for els in ocr_els):
            return None                                   # beyond the kernel's OCR capacity: the caller takes the host twin
        key = ("glue", float(self.iou_threshold))
        gs = getattr(dp, "_glue", {}).get(key)
        if gs is None:
            with torch.cuda.device(det.device):
                gs = _GlueState(dp, det, iw, ih, self.iou_threshold)
            dp._glue = {**getattr(dp, "_glue", {}), key: gs}
        gs.h_meta.zero_()
        for fi in range(len(frames)):
            els = ocr_els[fi]
            m = len(els)
            if m:
                gs.h_ocr[fi, :m] = torch.tensor([e["bbox"] for e in els], dtype=torch.float64)
                first, seen = {}, {}
                tab = gs.h_meta[fi, 2:2 + 2 * m].view(m, 2)
                for j, e in enumerate(els):                      # list.remove() works on dict equality: bbox + content decide it
                    k = (tuple(e["bbox"]), e["content"])
                    cls = first.setdefault(k, j)
                    tab[j, 0] = cls
                    tab[j, 1] = seen.get(cls, 0)
                    seen[cls] = seen.get(cls, 0) + 1
            gs.h_meta[fi, 0] = m
        det.stream.wait_stream(torch.cuda.current_stream(frames[0].device))          # frames the caller is still producing on its stream
        with torch.cuda.stream(det.stream):
            self._ev["det0"] = det.stream.record_event(torch.cuda.Event(enable_timing=True))
            for bi, f in enumerate(frames):
                dp.img[bi].copy_(f, non_blocking=True)
            gs.ocr.copy_(gs.h_ocr)
            gs.meta.copy_(gs.h_meta)
            gs.launch(det)                                        # detector + hand-off: one graph
            self._ev["det1"] = det.stream.record_event(torch.cuda.Event(enable_timing=True))
            tables = (dp, gs)
            if snapshot:
                snap = SimpleNamespace(out_boxes=dp.out_boxes.clone(), out_count=dp.out_count.clone(), elems=gs.elems.clone(),
                                       donors=gs.donors.clone(), crops=gs.crops.clone())
                tables = (snap, snap)
            counts = gs.counts.to("cpu", copy=True)               # the one synchronising read-back: 4 ints per frame
        return tables[0], tables[1], ocr_els, counts

    @torch.inference_mode()
    def assemble(self, dp, gs, ocr_els, counts, iw, ih, n_frames):
        """element dicts of every frame from the device tables (called once, after the caption micro-batches were queued)."""
        with torch.cuda.stream(self.det.stream):
            boxes = dp.out_boxes.cpu(); kcnt = dp.out_count.cpu(); elems = gs.elems.cpu(); donors = gs.donors.cpu()
        out = []
        for f in range(n_frames):
            k = int(kcnt[f])
            ratios = (boxes[f, :k] / torch.Tensor([iw, ih, iw, ih])).tolist()
            els = []
            for kind, src in elems[f, : int(counts[f, 0])].tolist():
                if kind == 0:
                    els.append(ocr_els[f][src])
                    continue
                label = None
                if kind == 1:
                    label = ""
                    for wd in range(MASK_WORDS):
                        bits = int(donors[f, src, wd]) & 0xFFFFFFFFFFFFFFFF
                        while bits:
                            low = bits & -bits
                            label += ocr_els[f][wd * 64 + low.bit_length() - 1]["content"] + " "
                            bits ^= low
                els.append({"type": "icon", "bbox": ratios[src], "interactivity": True, "content": label,
                            "source": "box_yolo_content_ocr" if kind == 1 else "box_yolo_content_yolo"})
            out.append(els)
        return out

    # ---- stage 3: caption all crops of all frames in packed micro-batches
    @torch.inference_mode()
    def caption(self, frames: Sequence[torch.Tensor], crops_per_frame, max_new_tokens=None, crops_dev: Optional[torch.Tensor] = None,
                prompt=None, scores=False):
        """crops_per_frame: host rectangles per frame, or — with `crops_dev` (int32 [frames, max_det, 4] on the device, rows in
        caption order) — just the number of crops per frame: the rectangles then never visit the host.  prompt: see `prompt_ids`.
        -> per frame a list of (text, ids row) per crop; scores (or a captioner with `token_scores` set): (text, ids row, confidence),
        `florence.caption_confidence` of the greedy tokens' log-probabilities."""
        return self.caption_finish(self.caption_launch(frames, crops_per_frame, max_new_tokens, crops_dev, prompt=prompt,
                                                       **({"scores": True} if scores else {})))

    def rank(self, frame: torch.Tensor, elements, queries, top_k=None):
        """`util.utils.rank_elements` for a frame already on the device: per query the elements of `elements` (one frame's list from
        `parse_batch`) by descending likelihood of the query as their crop's text, [{"index", "score"}]"""
        return U.rank_elements(frame, elements, {"model": self.cap, "processor": self.proc}, queries, top_k=top_k)

    def embed(self, frame: torch.Tensor, elements):
        """`util.utils.embed_elements` for a frame already on the device: (index, unit embeddings f32 [len(index), d_model] on the
        device) of one frame's elements (its list from `parse_batch`).  A call of its own beside `parse_batch` / `parse_stream`,
        whose results and wire format do not carry embeddings."""
        return U.embed_elements(frame, elements, {"model": self.cap, "processor": self.proc})

    def match(self, frame: torch.Tensor, elements, exemplars, top_k=5):
        """`util.utils.match_elements` for a frame already on the device: per exemplar (images, or an f32 [m, D] tensor of
        embeddings) the elements that look like it, [{"index", "score"}] by descending cosine similarity"""
        return U.match_elements(frame, elements, {"model": self.cap, "processor": self.proc}, exemplars, top_k=top_k)

    def locate(self, frame: torch.Tensor, phrases, task="<OPEN_VOCABULARY_DETECTION>", **kw):
        """`util.utils.locate` for a frame already on the device: boxes in frame pixels for every phrase (None for the box tasks
        without text), [{"label", "query", "bbox", "confidence", "tile", "phrase"}]"""
        return U.locate(frame, {"model": self.cap, "processor": self.proc}, task=task, text=phrases, **kw)

    def segment(self, frame: torch.Tensor, phrases=None, regions=None, **kw):
        """`util.utils.segment` for a frame already on the device: polygons, masks and click points for every phrase, or for every box
        of `regions` (frame pixels); exactly one of the two"""
        return U.segment(frame, {"model": self.cap, "processor": self.proc}, text=phrases, regions=regions, **kw)

    def track(self, prev_frame: torch.Tensor, prev_elements, frame: torch.Tensor, elements, min_score=0.9):
        """`util.utils.track_elements` of two frames already on the device: [(prev_index, index, score)], the one-to-one mutual
        best matches between the elements of the previous frame and of this one"""
        return U.track_elements(self.embed(prev_frame, prev_elements), self.embed(frame, elements), min_score=min_score)

    def prompt_ids(self, prompt):
        """one caption prompt for a call: None (the default <CAPTION> prompt), text (a Florence-2 task token or free text, tokenised
        by the parser's processor) or a list of token ids (bos ... eos) -> list of ids, or None"""
        if prompt is None:
            return None
        if isinstance(prompt, str):
            return self.proc.prompt_ids(prompt)
        return [int(t) for t in prompt]

    @torch.inference_mode()
    def caption_launch(self, frames: Sequence[torch.Tensor], crops_per_frame, max_new_tokens=None, crops_dev: Optional[torch.Tensor] = None,
                       overlap=False, prompt=None, scores=False):
        """queue the crop / encode / decode work of every micro-batch on the captioner's stream; nothing is read back.  The handle
        keeps the frames alive until `caption_finish`.  overlap (parse_stream): micro-batches alternate between `self.encode_lanes`
        HIP streams, and the merged decode runs on a further stream on one of two alternating decode plans, so the next batch's
        encode does not wait for it.  prompt: one prompt for every crop of the call (`prompt_ids`); the default prompt takes the
        plans it always took.  scores (or `cap.token_scores`): the decoding plans also write the token log-probabilities
        (OMNI_OP_GREEDY_STEP p4), snapshotted next to the ids; greedy decoding only.  Off: the plans and the calls they always were."""
        cap = self.cap
        R = cap.resolution
        prompt = self.prompt_ids(prompt)
        pr = cap.prompt_batch([prompt], R) if prompt is not None else None      # (ids [1, n_txt], keys [1], n_txt) or None = default
        pkw = {}
        if pr is not None:
            pkw = {"n_txt": pr[2]}
            # the device copies are read by copies queued on the lane streams: they stay alive in a small cache (a stream uses one prompt)
            held = self.__dict__.setdefault("_prompt_dev", {})
            if (tuple(prompt), R) not in held:
                if len(held) >= 8:
                    torch.cuda.synchronize(cap.device)
                    held.clear()
                held[(tuple(prompt), R)] = (pr[0].to(cap.device), pr[1].to(cap.device))
            pr_ids, pr_keys = held[(tuple(prompt), R)]
        max_new_tokens = max_new_tokens or self.max_new_tokens
        if crops_dev is not None:
            flat = [(fi, k) for fi, n in enumerate(crops_per_frame) for k in range(int(n))]
        else:
            flat = [(fi, b) for fi, cl in enumerate(crops_per_frame) for b in cl]
        ids_all = []
        # more than one micro-batch: the encode side runs per micro-batch, the 20 decode steps ONCE over all crops
        # (florence.py::_DecodePlans); OMNI_MERGED_DECODE=0 = every micro-batch decodes on its own (A/B knob)
        merged = len(flat) > self.batch_size and os.environ.get("OMNI_MERGED_DECODE", "1") != "0"
        beam = cap.beam_config()       # cap.num_beams > 1: beam search in the decode plans (the encode-only plans of a merged batch stay greedy)
        # overlap (parse_stream): micro-batches alternate between two encode lanes (HIP streams); 128-row plans exist once per lane, the
        # smaller capacities once — a plan's `free_evt` orders its next use, on whichever lane, behind its last one
        lanes = [cap.encode_lane(k) for k in range(max(1, self.encode_lanes))] if overlap else [cap.stream]
        cap.begin_batch()              # the plan sets this batch takes from the captioner's cache stay resident until the next batch
        if overlap and merged:
            self._dec_slot = 1 - getattr(self, "_dec_slot", 1)
        bkw = {"beam": beam} if beam else {}
        if scores or getattr(cap, "token_scores", False):
            if beam:
                raise ValueError("caption confidence needs greedy decoding (num_beams = 1): beam search has no token scores")
            bkw = {"scores": True}     # like the beams: only the plans that decode carry it, the encode-only plans of a merged batch do not change
        dec = cap.decode_plans(cap.decode_bucket(len(flat)), R, max_new_tokens, slot=self._dec_slot if overlap else 0, **bkw, **pkw) if merged else None
        if merged and not overlap:
            with torch.cuda.stream(cap.stream):
                dec.reset()
        if not overlap:
            self._ev["cap0"] = cap.stream.record_event(torch.cuda.Event(enable_timing=True))
        used = []
        for mbi, s in enumerate(range(0, len(flat), self.batch_size)):
            chunk = flat[s:s + self.batch_size]
            n = len(chunk)
            lane = 0
            if overlap and merged:
                lane = self._mb_count = (getattr(self, "_mb_count", -1) + 1) % len(lanes)
            stream = lanes[lane]
            # full micro-batches: one plan set per lane.  The remainder of a merged batch encodes exactly its n rows as a second graph over
            # the buffers of ITS LANE's full-capacity plan set (florence.py::_CaptionPlans.encode_rows, taken inside `_encode_into`);
            # otherwise (single micro-batch, OMNI_EXACT_ROWS=0) a padded bucket plan with buffers of its own
            if merged and cap.exact_rows and n < self.batch_size:
                cp = cap.plans(cap.bucket(self.batch_size), R, max_new_tokens, slot=lane, **pkw)
            else:
                cp = cap.plans(cap.bucket(n), R, max_new_tokens, slot=lane if n == self.batch_size else 0, **({} if merged else bkw), **pkw)
            with torch.cuda.stream(stream):
                if cp.free_evt is not None:
                    stream.wait_event(cp.free_evt)
                if merged and dec.free_evt is not None and stream not in used:
                    stream.wait_event(dec.free_evt)      # the decode two batches ago read this decode plan's cross-attention K/V
                if not merged:
                    cp.reset()
                c64, tmp = cap.crop_scratch(n, R)
                if crops_dev is None:
                    bx = torch.tensor([b for _, b in chunk], dtype=torch.int32).to(cap.device, non_blocking=True)
                o = 0
                while o < n:                                   # one crop launch per source frame run
                    fi = chunk[o][0]
                    e = o
                    while e < n and chunk[e][0] == fi:
                        e += 1
                    rects = crops_dev[fi, chunk[o][1]:] if crops_dev is not None else bx[o:]     # rows of one frame are contiguous
                    cap.launch_crops(cp, o, e - o, frames[fi], rects, c64[o:], tmp[o:] if tmp is not None else None, stream)
                    o = e
                if pr is not None:
                    cp.set_prompt(pr_ids, pr_keys, n)
                if merged:
                    cap._encode_into(cp, n, dec, s, stream)
                else:
                    ids_all.append(cap._run(cp, n, max_new_tokens, defer=True))   # keep the GPU fed: no sync between micro-batches
                if overlap:
                    cp.free_evt = stream.record_event()
            if stream not in used:
                used.append(stream)
        ids_stream = cap.stream
        if merged and not overlap:
            with torch.cuda.stream(cap.stream):
                self._ev["cap1"] = cap.stream.record_event(torch.cuda.Event(enable_timing=True))
                ids_all.append(cap._decode_merged(dec, len(flat), max_new_tokens))
                self._ev["cap2"] = cap.stream.record_event(torch.cuda.Event(enable_timing=True))
        elif merged:
            ids_stream = cap.dec_stream
            encoded = [st.record_event() for st in used]
            with torch.cuda.stream(ids_stream):
                for ev in encoded:
                    ids_stream.wait_event(ev)
                dec.reset()
                ids_all.append(cap._decode_merged(dec, len(flat), max_new_tokens, ids_stream))
                dec.free_evt = ids_stream.record_event()
        if not overlap:
            self._ev["capE"] = cap.stream.record_event(torch.cuda.Event(enable_timing=True))
        return (list(frames), flat, ids_all, ids_stream)

    def _settle_gc(self):
        """Python's generational collector, not the GPU, produced the one-step-in-twenty +40...70 ms of the round-5 bench lines
        (profiles/r6_s2_gc_*.json: one gen-2 collection inside the driver's 20 steps = the one 733 ms step; none with the collector off
        or frozen).  The plans of a parser are tens of thousands of long-lived Python objects (op descriptors, views, tensors): every
        full collection walks them all while the GPU pipeline waits for the host to queue the next batch.  After each of the first
        batches (all plan sets of the steady state exist by then: two encode lanes, the remainder plan, two decode plans) the survivors
        are moved to the permanent generation (`gc.freeze`), so later collections only look at what a batch allocates.  The collector
        stays on; OMNI_GC_FREEZE=0 turns this off."""
        n = getattr(self, "_gc_settled", 0)
        if n >= 3 or os.environ.get("OMNI_GC_FREEZE", "1") == "0":
            return
        import gc
        gc.unfreeze()                  # what an earlier parser of this process froze and has since died must be collectable (its plans hold HBM)
        gc.collect()
        gc.freeze()
        self._gc_settled = n + 1

    def _check_range(self):
        """Range guard of the split-f16 GEMM operands (include/omni_amd.h::omni_overflow_count), read where the host has just waited for
        a batch's ids anyway: a value beyond the f16 range was clamped (format B) or lost (format A) somewhere in the last batch(es) —
        the fp32 reference has no such limit, so the result may differ from it.  Accumulated in `range_overflow_total`, the last
        reading in `stats["split_overflow"]` (filled by the callers), fatal with OMNI_STRICT_RANGE=1 (what the parity tests run with)."""
        n = L.overflow_count(reset=True)
        self.range_overflow_last = n
        self.range_overflow_total = getattr(self, "range_overflow_total", 0) + n
        if n and os.environ.get("OMNI_STRICT_RANGE", "0") == "1":
            raise L.OmniError(f"split-f16 range guard: {n} threads produced a GEMM operand beyond +-65504 in this batch "
                              "(the fp32 reference has no such limit; results may differ from it)")

    @torch.inference_mode()
    def caption_finish(self, handle):
        frames, flat, ids_all, ids_stream = handle
        cap = self.cap
        # single read-back point.  The snapshots were produced on one of the captioner's streams (non-blocking streams: the default
        # stream does not order against them), so the copies are issued ON that stream — stream order alone makes them see the finished ids
        # (a scores plan's snapshot is (ids, token log-probabilities): both are read here)
        with torch.cuda.stream(ids_stream):
            ids_all = [tuple(x.cpu() for x in t) if isinstance(t, tuple) else t.cpu() for t in ids_all]
        logp_all = [t[1] if isinstance(t, tuple) else None for t in ids_all]
        ids_all = [cap._finish_ids((t[0] if isinstance(t, tuple) else t).long()) for t in ids_all]
        self._check_range()
        self._settle_gc()
        out = [[] for _ in frames]
        k = 0
        for ids, logp in zip(ids_all, logp_all):
            texts = [t.strip() for t in self.proc.batch_decode(ids, skip_special_tokens=True)]
            for r, (t, row) in enumerate(zip(texts, ids)):
                if logp is None:
                    out[flat[k][0]].append((t, row))
                else:                      # logp [n, max_new + 1], column 0 = the start token
                    w = cap.w
                    out[flat[k][0]].append((t, row, caption_confidence(row, logp[r, 1:], w.eos, w.forced_bos, w.forced_eos,
                                                                       logp.shape[1] - 1)))
                k += 1
        return out

    # ---- stage 4 (return_image=True): the tail of get_som_labeled_img for the whole batch.  The overlay depends on the boxes only, which
    #      are final once the hand-off has run, so it is queued on a stream of its own BEFORE the caption work and read back after it.
    def _annotate_scratch(self, B, H, W, device):
        """`U.AnnotateScratch` per (B, H, W), two alternating sets (parse_stream queues batch i+1 before it reads batch i back, and
        reads batch i back before it queues batch i+2), cached on the parser, least recently used shape evicted first
        (OMNI_MAX_ANNOTATE_SCRATCH shapes stay, default 2; `release_annotate_scratch` drops them all)."""
        cache = self.__dict__.setdefault("_ann_scratch", {})
        key = (B, H, W)
        if key in cache:
            cache[key] = cache.pop(key)
        else:
            keep = max(1, int(os.environ.get("OMNI_MAX_ANNOTATE_SCRATCH", "2")))
            while len(cache) >= keep:
                self._ann_stream.synchronize()           # the evicted buffers may still be in use on the annotate stream
                cache.pop(next(iter(cache)))
            cache[key] = [0, [None, None]]
        ent = cache[key]
        ent[0] = 1 - ent[0]
        if ent[1][ent[0]] is None:
            with torch.cuda.device(device):
                ent[1][ent[0]] = U.AnnotateScratch(B, H, W, device)
        return ent[1][ent[0]]

    def release_annotate_scratch(self):
        """free the cached overlay / PNG scratch (about 60 MB per 1080p frame and set); call it where the plans are cleared"""
        if self.__dict__.get("_ann_scratch"):
            self._ann_stream.synchronize()
            self._ann_scratch.clear()

    def annotate_hbm_bytes(self):
        return sum(sc.nbytes() for ent in self.__dict__.get("_ann_scratch", {}).values() for sc in ent[1] if sc is not None)

    @torch.inference_mode()
    def _annotate_launch(self, frames, elems_all, iw, ih, draw_bbox_config=None):
        """elems_all: the element lists of the batch (geometry final, captions not needed).  Labels are the running indices of each
        list, boxes its `bbox` ratios, style `draw_bbox_config` or util.omniparser.overlay_style((w, h)).  On the device (`U.
        overlay_on_device`): ONE overlay launch + ONE deflate chain on the annotate stream, behind everything the caller's and the
        detector's streams hold so far, out of place — the caption crops read the same frames.  -> handle for `_annotate_finish`."""
        from .util.omniparser import overlay_style
        cfg = dict(draw_bbox_config or overlay_style((iw, ih)))
        boxes = [U._box_convert_xyxy_to_cxcywh(torch.tensor([e["bbox"] for e in el], dtype=torch.float32).reshape(-1, 4)) for el in elems_all]
        phrases = [list(range(len(el))) for el in elems_all]
        dev = frames[0].device
        if os.environ.get("OMNI_SKIP_ANNOTATE", "0") == "1":
            return ("skip", boxes, phrases, iw, ih)
        if not U.overlay_on_device(dev):
            return ("host", list(frames), boxes, phrases, cfg)
        if self.__dict__.get("_ann_stream") is None:
            with torch.cuda.device(dev):
                self._ann_stream = torch.cuda.Stream(dev)
        st = self._ann_stream
        st.wait_stream(torch.cuda.current_stream(dev))       # frames the caller is still producing on its stream
        if self.det is not None and getattr(self.det, "stream", None) is not None:
            st.wait_stream(self.det.stream)
        sc = self._annotate_scratch(len(frames), ih, iw, dev)
        self._ev["ann0"] = st.record_event(torch.cuda.Event(enable_timing=True))
        handle = U.annotate_encode_device_batch_launch(frames, boxes, phrases, stream=st, scratch=sc, **cfg)
        self._ev["ann1"] = st.record_event(torch.cuda.Event(enable_timing=True))
        return ("device", handle)

    @torch.inference_mode()
    def _annotate_finish(self, handle):
        """-> [(som_image_base64, label_coordinates)] per frame (pixel xywh, what `get_som_labeled_img` returns first and second)"""
        if handle[0] == "device":
            return U.annotate_encode_device_batch_finish(handle[1])
        if handle[0] == "skip":
            _, boxes, phrases, iw, ih = handle
            out = []
            for b, ph in zip(boxes, phrases):
                cx, cy, bw, bh = (b * torch.Tensor([iw, ih, iw, ih])).unbind(-1)
                xywh = torch.stack((cx - 0.5 * bw, cy - 0.5 * bh, bw, bh), -1).numpy()
                out.append(("", {f"{k}": v for k, v in zip(ph, xywh)}))
            return out
        _, frames, boxes, phrases, cfg = handle
        out = []
        for f, b, ph in zip(frames, boxes, phrases):
            frame, coords = U.annotate(f.cpu().numpy(), b, None, ph, **cfg)
            out.append((U.encode_png_b64(frame), coords))
        return out

    @staticmethod
    def _with_images(result, return_ids, images):
        return (*result, images) if return_ids else (result, images)

    @torch.inference_mode()
    def parse_batch(self, frames: Sequence[torch.Tensor], ocr: Optional[Sequence] = None, return_ids=False,
                    pad_to: Optional[int] = None, prompt=None, return_image=False, draw_bbox_config=None, return_confidence=False):
        """frames: uint8 [H,W,3] device tensors (same size); ocr: per frame (texts, xyxy px boxes) or None;
        pad_to: detector plan batch size to use when fewer frames arrive (see `detect`); prompt: the caption prompt of this call
        (`prompt_ids`: text or token ids; None = <CAPTION>).
        return_image: the result gains a LAST member, per frame (som_image_base64, label_coordinates) — the set-of-marks PNG and
        the pixel xywh of every element, the first two members of `get_som_labeled_img`'s result; labels are the running indices of
        the frame's element list, style = draw_bbox_config or util.omniparser.overlay_style((w, h)).  The frames are not drawn on.
        OMNI_OVERLAY=host: Pillow per frame; OMNI_SKIP_ANNOTATE=1: "" for the image.
        return_confidence (or a captioner with `token_scores` set): every element whose `content` the captioner wrote gains
        "confidence" in (0, 1] (`florence.caption_confidence`: the geometric-mean probability of its greedy tokens, computed on the
        device next to the arg-max); OCR elements and icons that took OCR text have no such key.  Greedy decoding only."""
        ih, iw = frames[0].shape[:2]
        prompt = self.prompt_ids(prompt)
        ckw = {"conf": True} if self._confidence(return_confidence) else {}
        with self.det._lock, self.cap._lock:
            if return_image:
                return self._parse_batch_locked(frames, ocr, return_ids, iw, ih, pad_to, prompt, True, draw_bbox_config, **ckw)
            return self._parse_batch_locked(frames, ocr, return_ids, iw, ih, pad_to, prompt, **ckw)

    def _confidence(self, return_confidence) -> bool:
        if not isinstance(return_confidence, bool):
            raise ValueError(f"return_confidence must be a bool, got {return_confidence!r}")
        return return_confidence or bool(getattr(self.cap, "token_scores", False))

    def parse_stream(self, batches, return_ids=False, pad_to: Optional[int] = None, prompt=None, return_image=False, draw_bbox_config=None,
                     return_confidence=False):
        """Generator over an iterable of (frames, ocr) batches -> what `parse_batch` returns for each, in order, as a software
        pipeline: the detector pass and the host hand-off of batch i+1 run on a helper thread (their stream is the detector's)
        while the captions of batch i occupy the GPU, and the caption work of batch i+1 is queued BEFORE the read-back of batch i
        blocks — the GPU never waits for the host between batches.  Same kernels, same order per batch, same results as
        `parse_batch`.  (Host hand-off only: with OMNI_DEVICE_GLUE the crop table of a batch lives in per-plan device buffers.)
        prompt: one caption prompt for the whole stream (`prompt_ids`).  return_image / draw_bbox_config: as `parse_batch`; the
        overlay + PNG work of a batch is queued on the annotate stream before its caption work and read back with its ids.
        return_confidence: as `parse_batch`, for the whole stream."""
        from concurrent.futures import ThreadPoolExecutor
        prompt = self.prompt_ids(prompt)
        img = (True, draw_bbox_config) if return_image else None
        skw = {"scores": True} if self._confidence(return_confidence) else {}
        if self.device_glue:
            yield from self._parse_stream_device(batches, return_ids, pad_to, prompt, *(() if img is None else (img,)),
                                                 **({"conf": True} if skw else {}))
            return

        def stage_a(frames, ocr):
            with torch.inference_mode(), self.det._lock:
                ih, iw = frames[0].shape[:2]
                det_boxes = self.detect(frames, pad_to)
                elems_all, crops_all = [], []
                for fi, xy in enumerate(det_boxes):
                    texts, boxes = ocr[fi] if ocr is not None else ([], [])
                    el, cr = self.glue(xy, iw, ih, boxes, texts)
                    elems_all.append(el); crops_all.append(cr)
                return frames, elems_all, crops_all, [len(b) for b in det_boxes]

        def finish(pending):
            handle, elems_all, crops_all, nbox, ann = pending
            with torch.inference_mode(), self.cap._lock:
                caps = self.caption_finish(handle)
            ids_out = self._fill_captions(elems_all, caps)
            self.stats = {"crops": [len(c) for c in crops_all], "boxes": nbox, "split_overflow": getattr(self, "range_overflow_last", 0)}
            self.last_crops = crops_all
            res = (elems_all, ids_out) if return_ids else elems_all
            return res if ann is None else self._with_images(res, return_ids, self._annotate_finish(ann))

        it = iter(batches)
        first = next(it, None)
        if first is None:
            return
        with ThreadPoolExecutor(1) as helper:
            fut = helper.submit(stage_a, *first)
            pending = None
            while fut is not None:
                frames, elems_all, crops_all, nbox = fut.result()
                nxt = next(it, None)
                fut = helper.submit(stage_a, *nxt) if nxt is not None else None
                ann = None
                if img is not None:                       # before the caption work, so that it runs under the encode
                    ann = self._annotate_launch(frames, elems_all, frames[0].shape[1], frames[0].shape[0], draw_bbox_config)
                with torch.inference_mode(), self.cap._lock:
                    handle = self.caption_launch(frames, crops_all, **({} if prompt is None else {"prompt": prompt}), **skw)
                if pending is not None:
                    yield finish(pending)
                pending = (handle, elems_all, crops_all, nbox, ann)
            yield finish(pending)

    def _parse_stream_device(self, batches, return_ids, pad_to, prompt=None, img=None, conf=False):
        """parse_stream with the device hand-off (the default): four HIP streams, one host thread.  Batch i+1's detector + hand-off
        graph runs on the detector's stream while batch i encodes; its tables are snapshotted (`detect_glue`) so nothing of batch i
        reads the detector plan's buffers afterwards; caption micro-batches alternate between two encode streams (the HBM-bound
        kernels of one fill what the MFMA-bound GEMMs of the other leave idle); batch i's 20 decode steps run on a fourth stream, on
        one of two decode plans, while batch i+1 encodes.  Same kernels on the same data per batch as `parse_batch`."""
        def finish(p):
            handle, snap, ocr_els, counts, iw, ih, n_frames, n_crops = p[:8]
            early = p[8] if len(p) > 8 else None         # return_image: (elements assembled before the captions, annotate handle)
            with torch.inference_mode(), self.cap._lock:
                caps = self.caption_finish(handle)
                elems_all = early[0] if early is not None else self.assemble(snap, snap, ocr_els, counts, iw, ih, n_frames)
            ids_out = self._fill_captions(elems_all, caps)
            self.stats = {"crops": n_crops, "boxes": [int(v) for v in snap.out_count[:n_frames].tolist()], "split_overflow": getattr(self, "range_overflow_last", 0)}
            self.last_crops = [snap.crops[f, :n].tolist() for f, n in enumerate(n_crops)]
            res = (elems_all, ids_out) if return_ids else elems_all
            return res if early is None else self._with_images(res, return_ids, self._annotate_finish(early[1]))

        try:
            yield from self._stream_loop(batches, return_ids, pad_to, finish, prompt, *(() if img is None else (img,)),
                                         **({"conf": True} if conf else {}))
        finally:
            torch.cuda.synchronize(self.cap.device)      # an abandoned generator leaves no work behind on the side streams

    def _stream_loop(self, batches, return_ids, pad_to, finish, prompt=None, img=None, conf=False):
        pending = None
        for frames, ocr in batches:
            ih, iw = frames[0].shape[:2]
            tiled = self.tile_large and (iw > 1952 or ih > 1112)
            with self.det._lock:
                handed = None if tiled else self.detect_glue(frames, ocr, pad_to, snapshot=True)
            if handed is None:                       # beyond the hand-off kernel's capacities / tiled: drain, then the ordinary path
                if pending is not None:
                    yield finish(pending)
                    pending = None
                yield self.parse_batch(frames, ocr, return_ids=return_ids, pad_to=pad_to, **({} if prompt is None else {"prompt": prompt}),
                                       **({} if img is None else {"return_image": True, "draw_bbox_config": img[1]}),
                                       **({"return_confidence": True} if conf else {}))
                continue
            snap, _, ocr_els, counts = handed
            n_crops = [int(counts[f, 1]) for f in range(len(frames))]
            early = ()
            if img is not None:
                # the element geometry does not depend on the captions: assemble now and queue overlay + PNG on the annotate stream
                # BEFORE this batch's caption work, so that it runs under the encode; `finish` fills the captions into these elements
                with self.det._lock:
                    elems_all = self.assemble(snap, snap, ocr_els, counts, iw, ih, len(frames))
                early = ((elems_all, self._annotate_launch(frames, elems_all, iw, ih, img[1])),)
            with torch.inference_mode(), self.cap._lock:
                handle = self.caption_launch(frames, n_crops, crops_dev=snap.crops, overlap=True, **({} if prompt is None else {"prompt": prompt}),
                                             **({"scores": True} if conf else {}))
            if pending is not None:
                yield finish(pending)
            pending = (handle, snap, ocr_els, counts, iw, ih, len(frames), n_crops, *early)
        if pending is not None:
            yield finish(pending)

    def stage_ms(self):
        """device time of the stages of the last `parse_batch` (HIP events recorded on the stream each stage runs on; everything has
        been read back by now, so the events have completed): detector + hand-off graph, caption encode (crop -> DaViT -> BART encoder
        -> cross K/V of every micro-batch), the 20 decode steps.  The reference returns one wall-clock `latency` per request
        (ref:omnitool/omniparserserver/omniparserserver.py:42-44); the batch route adds this split."""
        ev, out = self._ev, {}
        for name, a, b in (("detect+handoff", "det0", "det1"), ("caption", "cap0", "capE"), ("caption_encode", "cap0", "cap1"),
                           ("caption_decode", "cap1", "cap2"), ("annotate", "ann0", "ann1")):
            if a in ev and b in ev:
                try:
                    out[name] = round(float(ev[a].elapsed_time(ev[b])), 3)
                except RuntimeError:       # an event of an earlier batch that never completed on this path
                    pass
        self._ev = {}
        return out

    @staticmethod
    def _fill_captions(elems_all, caps):
        ids_out = []
        for el, cl in zip(elems_all, caps):
            q = list(cl)
            for e in el:
                if e["content"] is None and q:
                    c = q.pop(0)           # (text, ids row) or, from scores plans, (text, ids row, confidence)
                    e["content"] = c[0]
                    if len(c) > 2:
                        e["confidence"] = c[2]
            ids_out.append([c[1] for c in cl])
        return ids_out

    def _parse_batch_locked(self, frames, ocr, return_ids, iw, ih, pad_to=None, prompt=None, return_image=False, draw_bbox_config=None,
                            conf=False):
        tiled = self.tile_large and (iw > 1952 or ih > 1112)
        pkw = {} if prompt is None else {"prompt": prompt}       # no prompt: the calls they always were (subclasses override `caption`)
        if conf:
            pkw["scores"] = True
        handed = self.detect_glue(frames, ocr, pad_to) if (self.device_glue and not tiled) else None
        if handed is not None:
            dp, gs, ocr_els, counts = handed
            n_crops = [int(counts[f, 1]) for f in range(len(frames))]
            # crop rectangles were produced on the detector's stream, which the counts read-back above has drained: no event needed
            ann = None
            if return_image:                              # geometry is final: overlay + PNG run on their own stream under the captions
                elems_all = self.assemble(dp, gs, ocr_els, counts, iw, ih, len(frames))
                ann = self._annotate_launch(frames, elems_all, iw, ih, draw_bbox_config)
            caps = self.caption(frames, n_crops, crops_dev=gs.crops, **pkw)
            if not return_image:
                elems_all = self.assemble(dp, gs, ocr_els, counts, iw, ih, len(frames))
            ids_out = self._fill_captions(elems_all, caps)
            images = self._annotate_finish(ann) if ann is not None else None
            self.stats = {"crops": n_crops, "boxes": [int(v) for v in dp.out_count[: len(frames)].tolist()], "stage_ms": self.stage_ms(),
                          "split_overflow": getattr(self, "range_overflow_last", 0)}
            self.last_crops = [gs.crops[f, :n].tolist() for f, n in enumerate(n_crops)]
            res = (elems_all, ids_out) if return_ids else elems_all
            return res if ann is None else self._with_images(res, return_ids, images)
        if tiled:
            det_boxes = [self.detect_tiled(f)[0] for f in frames]      # >1080p: overlapping tiles + global NMS (our policy)
        else:
            det_boxes = self.detect(frames, pad_to)
        elems_all, crops_all = [], []
        for fi, xy in enumerate(det_boxes):
            texts, boxes = ocr[fi] if ocr is not None else ([], [])
            el, cr = self.glue(xy, iw, ih, boxes, texts)
            elems_all.append(el); crops_all.append(cr)
        ann = self._annotate_launch(frames, elems_all, iw, ih, draw_bbox_config) if return_image else None
        caps = self.caption(frames, crops_all, **pkw)
        ids_out = self._fill_captions(elems_all, caps)
        self.stats = {"crops": [len(c) for c in crops_all], "boxes": [len(b) for b in det_boxes], "split_overflow": getattr(self, "range_overflow_last", 0)}
        self.last_crops = crops_all            # integer crop boxes per frame, in caption order (parity tests read them)
        res = (elems_all, ids_out) if return_ids else elems_all
        return res if ann is None else self._with_images(res, return_ids, self._annotate_finish(ann))

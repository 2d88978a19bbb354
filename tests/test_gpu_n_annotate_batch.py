"""`-m gpu`: annotated PNGs from `ScreenParser.parse_batch` / `parse_stream` (return_image=True) — the frame-batched overlay + LZ
deflate tail (csrc/overlay_png.hip: OMNI_OP_OVERLAY p3 / p4 / i3, OMNI_OP_PNG_DEFLATE i5 = 2) queued on its own stream under the
captions.  Everything here is bytes: the strings against the single-frame `annotate_encode_device` (pinned to the oracle by
tests/test_gpu_f_overlay_png.py), the decoded images against the host raster `U.annotate`, small frames against
oracle/png_ref.py::deflate_png_lz file for file.  Stand-in weights (tools.make_weights), half-width detector, 64x64 caption crops.
The host emulation twin: tests/test_annotate_batch_emu_cpu.py."""
import base64
import io
import types

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def models():
    from omniparser_amd.florence import Florence2Captioner
    from omniparser_amd.util.yolov9 import YOLOv9Detector
    from tools.make_weights import ensure_blob, ensure_caption_checkpoint
    det = YOLOv9Detector(model_path=ensure_blob(seed=0, nc=1, width=0.5), device="cuda", precision="f32")
    cap = Florence2Captioner(ensure_caption_checkpoint(0), "cuda", precision="f32", resolution=64)
    return det, cap


def _parser(models, **kw):
    from omniparser_amd.pipeline import ScreenParser
    return ScreenParser(models[0], models[1], box_threshold=0.05, iou_threshold=0.7, nms_iou=0.1, max_det=300, imgsz=640, **kw)


def _batch(seeds, w, h, n_ocr=40):
    from omniparser_amd.synth import synthetic_ocr, synthetic_screenshot
    imgs = [synthetic_screenshot(s, w, h) for s in seeds]
    return imgs, [torch.from_numpy(a).cuda() for a in imgs], [synthetic_ocr(s, w, h, n_ocr) for s in seeds]


def _cxcywh(elems):
    from omniparser_amd.util import utils as U
    return U._box_convert_xyxy_to_cxcywh(torch.tensor([e["bbox"] for e in elems], dtype=torch.float32).reshape(-1, 4))


def _decode(s):
    return np.asarray(Image.open(io.BytesIO(base64.b64decode(s))).convert("RGB"))


def _assert_host_raster(img, elems, marked, w, h):
    """the returned image decodes to the host raster of the frame's elements, and the label coordinates are the host's"""
    from omniparser_amd.util import utils as U
    from omniparser_amd.util.omniparser import overlay_style
    host, coords = U.annotate(img, _cxcywh(elems), None, list(range(len(elems))), **overlay_style((w, h)))
    png, got = marked
    assert np.array_equal(_decode(png), host)
    assert list(got) == list(coords) and all(np.array_equal(got[k], coords[k]) for k in coords)
    assert len(elems) == 0 or not np.array_equal(host, img)


def _ids(ids):
    return [[r.tolist() for r in f] for f in ids]


def test_parse_batch_8_frames_1080p_returns_the_single_frame_pngs(models):
    """8 synthetic 1080p frames with OCR: elements and ids are those of the call without the argument (the crops never saw annotated
    pixels), the frames keep their bytes, every string is what `annotate_encode_device` returns for the frame's elements on a fresh
    copy, decodes to the host raster, and the label coordinates are the host's."""
    from omniparser_amd.util import utils as U
    from omniparser_amd.util.omniparser import overlay_style
    sp = _parser(models)
    W, H = 1920, 1080
    imgs, frames, ocr = _batch(range(8), W, H)
    plain_el, plain_ids = sp.parse_batch(frames, ocr, return_ids=True)
    elems, ids, marked = sp.parse_batch(frames, ocr, return_ids=True, return_image=True)
    torch.cuda.synchronize()
    assert elems == plain_el and _ids(ids) == _ids(plain_ids)
    assert len(marked) == 8 and sum(len(e) for e in elems) > 200
    for f in range(8):
        assert np.array_equal(frames[f].cpu().numpy(), imgs[f]), f
        want, wcoords = U.annotate_encode_device(None, _cxcywh(elems[f]), list(range(len(elems[f]))), "cuda",
                                                 frame_dev=torch.from_numpy(imgs[f].copy()).cuda(), **overlay_style((W, H)))
        assert marked[f][0] == want, f
        assert list(marked[f][1]) == list(wcoords) and all(np.array_equal(marked[f][1][k], wcoords[k]) for k in wcoords), f
        _assert_host_raster(imgs[f], elems[f], marked[f], W, H)
    assert sp.annotate_hbm_bytes() > 8 * 50e6
    sp.release_annotate_scratch()
    assert sp.annotate_hbm_bytes() == 0


def test_batched_deflate_4_frames_270x480_is_the_oracle_file_for_file():
    from oracle import png_ref as PR
    from omniparser_amd.synth import synthetic_screenshot
    from omniparser_amd.util.utils import png_deflate_device_batch
    rng = np.random.default_rng(2)
    frames = [synthetic_screenshot(2, 480, 270), rng.integers(0, 256, (270, 480, 3), dtype=np.uint8), np.full((270, 480, 3), 200, dtype=np.uint8),
              np.ascontiguousarray(synthetic_screenshot(5, 960, 540)[100:370, 200:680])]
    png, b64, meta = png_deflate_device_batch(torch.from_numpy(np.stack(frames)).cuda())
    torch.cuda.synchronize()
    m = meta.cpu()
    for k, frame in enumerate(frames):
        data = png[k, :int(m[k, 1])].cpu().numpy().tobytes()
        assert data == PR.deflate_png_lz(frame), k
        assert b64[k, :int(m[k, 2])].cpu().numpy().tobytes() == base64.b64encode(data), k
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(data)).convert("RGB")), frame), k


def test_parse_stream_three_batches_equal_parse_batch_alone(models):
    """three batches of different content, the last one smaller: batch i + 1's overlay / PNG work is queued before batch i is read
    back (two alternating scratch sets), and every batch's elements, ids and images are those of `parse_batch` on that batch alone"""
    sp = _parser(models)
    W, H = 1280, 800
    groups = [_batch(seeds, W, H, 24) for seeds in ((11, 12, 13), (14, 15, 16), (17, 18))]
    got = list(sp.parse_stream([(fr, ocr) for _, fr, ocr in groups], return_ids=True, pad_to=3, return_image=True))
    assert len(got) == 3
    for (imgs, frames, ocr), (elems, ids, marked) in zip(groups, got):
        a_el, a_ids, a_marked = sp.parse_batch(frames, ocr, return_ids=True, pad_to=3, return_image=True)
        assert elems == a_el and _ids(ids) == _ids(a_ids)
        assert len(marked) == len(frames) == len(a_marked)
        for f in range(len(frames)):
            assert marked[f][0] == a_marked[f][0], f
            assert all(np.array_equal(marked[f][1][k], a_marked[f][1][k]) for k in a_marked[f][1])
            _assert_host_raster(imgs[f], elems[f], marked[f], W, H)
            assert np.array_equal(frames[f].cpu().numpy(), imgs[f])
    assert got[0][2][0][0] != got[1][2][0][0]


def test_tiled_route_frame_returns_the_host_raster(models):
    """a 3840x2160 frame takes the tiled route (above 1952x1112): only capacities change for the tail"""
    sp = _parser(models, tile_large=True)
    W, H = 3840, 2160
    imgs, frames, ocr = _batch((4,), W, H, 60)
    plain = sp.parse_batch(frames, ocr)
    elems, marked = sp.parse_batch(frames, ocr, return_image=True)
    assert elems == plain and len(marked) == 1 and len(elems[0]) > 50
    _assert_host_raster(imgs[0], elems[0], marked[0], W, H)
    assert np.array_equal(frames[0].cpu().numpy(), imgs[0])


def test_parse_many_group_of_three_uses_the_batched_tail(models):
    """`ParseService.parse_many` on 3 equal-sized images: the element lists of `parse_batch` on the same group, and every
    `som_image_base64` decodes to the host raster of its elements"""
    from omniparser_amd import server as S
    from omniparser_amd.synth import synthetic_ocr, synthetic_screenshot
    from omniparser_amd.util import utils as U
    from omniparser_amd.util.omniparser import overlay_style
    sp = _parser(models)
    W, H = 1280, 800
    seeds = (21, 22, 23)
    imgs = [synthetic_screenshot(s, W, H) for s in seeds]
    items = []
    for s, a in zip(seeds, imgs):
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, format="PNG")
        texts, boxes = synthetic_ocr(s, W, H, 24)
        items.append({"base64_image": base64.b64encode(buf.getvalue()).decode("ascii"),
                      "ocr": {"texts": list(texts), "boxes": [list(map(float, b)) for b in boxes]}})
    svc = S.ParseService(types.SimpleNamespace(ocr_provider=None), screen_parser=sp, workers=2)
    res = svc.parse_many(items)["results"]
    before = sp.parse_batch([torch.from_numpy(a).cuda() for a in imgs], [S._ocr_tuple(it["ocr"]) for it in items])
    assert len(res) == 3
    for f in range(3):
        assert set(res[f]) == {"som_image_base64", "parsed_content_list", "latency", "stage_ms"}
        assert res[f]["parsed_content_list"] == before[f] and len(before[f]) > 10
        host, _ = U.annotate(imgs[f], _cxcywh(before[f]), None, list(range(len(before[f]))), **overlay_style((W, H)))
        assert np.array_equal(_decode(res[f]["som_image_base64"]), host)

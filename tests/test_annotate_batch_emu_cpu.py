"""The frame-batched forms of OMNI_OP_OVERLAY and OMNI_OP_PNG_DEFLATE (i5 = 2) and the host code above them, run from the device sources
on the host emulation (tests/emu): every frame of a batch against the host raster `overlay.render` and against
oracle/png_ref.py::deflate_png_lz, byte for byte, and against the single-frame ops.  The `-m gpu` twin: tests/test_gpu_n_annotate_batch.py."""
import base64
import contextlib
import io
import types

import numpy as np
import pytest
import torch
from PIL import Image

from omniparser_amd.util import overlay as OV
from test_overlay_png_emu_cpu import _scene


def _overlay_batch(W, H, counts, seed=20):
    """frames + draw lists with `counts` boxes (3 primitives each; the degenerate boxes of `_scene` wherever there are boxes)"""
    frames, cmds = [], []
    for k, K in enumerate(counts):
        f, c = _scene(seed + k, W, H, max(K, 3))             # `_scene` plants three degenerate boxes; K = 0: the frame alone
        frames.append(f)
        cmds.append(c if K else [])
    return frames, cmds


def test_batched_overlay_equals_host_raster_and_leaves_the_sources(emu):
    """B = 3 at one size: no primitive at all (a plain copy), 39 of them, and 900 (four culling rounds of 256).  Every destination
    frame is `render` of a copy of its source; the sources keep their bytes."""
    frames, cmds = _overlay_batch(333, 97, (0, 13, 300))
    nprim = [OV.raster_primitives(c)[0].shape[0] for c in cmds]
    assert nprim[0] == 0 and 30 <= nprim[1] <= 50 and nprim[2] > 256
    srcs = [torch.from_numpy(f.copy()) for f in frames]
    dst = torch.full((3, 97, 333, 3), 0xAB, dtype=torch.uint8)
    OV.render_device_batch(srcs, dst, cmds)
    for f in range(3):
        assert np.array_equal(dst[f].numpy(), OV.render(frames[f].copy(), cmds[f])), f
        assert np.array_equal(srcs[f].numpy(), frames[f]), f
    assert np.array_equal(dst[0].numpy(), frames[0])
    assert not np.array_equal(dst[1].numpy(), frames[1]) and not np.array_equal(dst[2].numpy(), frames[2])


def _deflate_frames(H=96, W=240):
    """the frame kinds of test_overlay_png_emu_cpu._frames at ONE size whose filtered stream (96 x 721 = 69216 bytes) spans two full
    32 KiB units and a short third one"""
    from omniparser_amd.synth import synthetic_screenshot
    rng = np.random.default_rng(5)
    assert H * (3 * W + 1) >= 2 * 32768
    return [("noise", rng.integers(0, 256, (H, W, 3), dtype=np.uint8)),
            ("flat", np.full((H, W, 3), 77, dtype=np.uint8)),
            ("screenshot", np.ascontiguousarray(synthetic_screenshot(1, 480, 270)[40:40 + H, 100:100 + W])),
            ("pixel runs", np.tile(rng.integers(0, 256, (1, 1, 3), dtype=np.uint8), (H, W, 1)))]      # distance-3 matches across the unit boundaries


def test_batched_deflate_is_the_oracle_stream_per_frame(emu):
    from oracle import png_ref as PR
    from omniparser_amd.util.utils import png_deflate_device, png_deflate_device_batch
    kinds = _deflate_frames()
    batch = torch.from_numpy(np.stack([f for _, f in kinds]))
    png, b64, meta = png_deflate_device_batch(batch)
    assert png.shape[0] == b64.shape[0] == meta.shape[0] == 4
    for k, (name, frame) in enumerate(kinds):
        total, nb64 = int(meta[k, 1]), int(meta[k, 2])
        data = png[k, :total].numpy().tobytes()
        want = PR.deflate_png_lz(frame)
        assert data == want, (name, total, len(want))
        p1, b1, m1 = png_deflate_device(torch.from_numpy(frame), lz=True)
        assert data == p1[:int(m1[1])].numpy().tobytes(), name
        used = 4 + 2 * ((frame.shape[0] * (3 * frame.shape[1] + 1) + 32767) // 32768)      # sizes, then unit sizes and offsets
        assert used == 10 and meta[k, :used].tolist() == m1[:used].tolist(), name
        assert b64[k, :nb64].numpy().tobytes() == base64.b64encode(data) == b1[:int(m1[2])].numpy().tobytes(), name
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(data)).convert("RGB")), frame), name


def test_batch_of_one_is_the_single_frame_op(emu):
    """B = 1 through the batched entries = the existing ops, byte for byte; and the existing entries (ops built without the new
    slots) still draw in place and skip an empty draw list."""
    from omniparser_amd.util.utils import png_deflate_device, png_deflate_device_batch
    (frame,), (cmds,) = _overlay_batch(200, 120, (40,), seed=31)
    src = torch.from_numpy(frame.copy())
    dst = torch.zeros((1, 120, 200, 3), dtype=torch.uint8)
    OV.render_device_batch([src], dst, [cmds])
    inplace = OV.render_device(torch.from_numpy(frame.copy()), cmds)
    assert np.array_equal(dst[0].numpy(), inplace.numpy()) and np.array_equal(src.numpy(), frame)
    untouched = torch.from_numpy(frame.copy())
    assert OV.render_device(untouched, []) is untouched and np.array_equal(untouched.numpy(), frame)
    png, b64, meta = png_deflate_device_batch(dst)
    p1, b1, m1 = png_deflate_device(inplace, lz=True)
    used = 4 + 2 * ((120 * 601 + 32767) // 32768)
    assert meta[0, :used].tolist() == m1[:used].tolist()
    assert png[0, :int(meta[0, 1])].numpy().tobytes() == p1[:int(m1[1])].numpy().tobytes()
    assert b64[0, :int(meta[0, 2])].numpy().tobytes() == b1[:int(m1[2])].numpy().tobytes()


def test_batched_ops_refuse_bad_arguments_and_launch_nothing(emu):
    L = emu
    from omniparser_amd.util.utils import AnnotateScratch
    H, W, B = 20, 30, 2
    frames = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (B, H, W, 3), dtype=np.uint8))
    sc = AnnotateScratch(B, H, W, "cpu")
    outs = (sc.png, sc.filt, sc.slots, sc.meta, sc.part, sc.b64, sc.toks)
    for t in outs:
        t.fill_(0x5A)

    def deflate(over=None):
        i = {0: H, 1: W, 2: sc.cap, 3: sc.meta.shape[1], 4: sc.part.shape[1], 5: 2, 6: B}
        i.update(over or {})
        return L.make_op(L.OP_PNG_DEFLATE, L.F32, p=[frames.data_ptr(), sc.png.data_ptr(), sc.filt.data_ptr(), sc.slots.data_ptr(),
                                                     sc.meta.data_ptr(), sc.part.data_ptr(), sc.b64.data_ptr(), sc.toks.data_ptr()], i=i)
    for bad in ({2: sc.cap - 1}, {3: sc.meta.shape[1] - 1}, {4: sc.part.shape[1] - 1}, {6: 0}, {6: -3}):
        with pytest.raises(L.OmniError):
            L.launch(deflate(bad))
        assert all(bool((t == 0x5A).all()) for t in outs), bad
    L.launch(deflate())                                      # the same op with its capacities in order runs
    assert int(sc.meta[1, 1]) > 57

    srcs = [frames[0].clone(), frames[1].clone()]
    dst = torch.full((B, H, W, 3), 0x5A, dtype=torch.uint8)
    ptrs = torch.tensor([t.data_ptr() for t in srcs], dtype=torch.int64)
    offs = torch.zeros(B + 1, dtype=torch.int32)

    def overlay(p3, p4, nb):
        return L.make_op(L.OP_OVERLAY, L.F32, p=[dst.data_ptr(), None, None, p3, p4], i={0: H, 1: W, 2: 0, 3: nb})
    for bad in ((None, offs.data_ptr(), B), (ptrs.data_ptr(), None, B), (ptrs.data_ptr(), offs.data_ptr(), 0), (None, None, B)):
        with pytest.raises(L.OmniError):
            L.launch(overlay(*bad))
        assert bool((dst == 0x5A).all()), bad
    L.launch(overlay(ptrs.data_ptr(), offs.data_ptr(), B))
    assert np.array_equal(dst.numpy(), frames.numpy())


def test_annotate_encode_device_batch_equals_the_single_frame_call(emu):
    """the host layer: layout per frame, one overlay launch, one deflate chain -> the strings and label coordinates of
    `annotate_encode_device` frame by frame, and frames that were not drawn on"""
    from omniparser_amd.util import utils as U
    rng = np.random.default_rng(3)
    frames = [rng.integers(0, 256, (90, 160, 3), dtype=np.uint8) for _ in range(3)]
    boxes = [torch.tensor([[0.3, 0.4, 0.2, 0.3], [0.7, 0.5, 0.4, 0.6], [0.01, 0.02, 0.02, 0.03]]), torch.zeros(0, 4),
             torch.tensor([[0.5, 0.5, 0.9, 0.9]])]
    phrases = [list(range(len(b))) for b in boxes]
    dev = [torch.from_numpy(f.copy()) for f in frames]
    got = U.annotate_encode_device_batch(dev, boxes, phrases, text_scale=0.4, text_padding=5)
    for f in range(3):
        want = U.annotate_encode_device(frames[f], boxes[f], phrases[f], "cpu", text_scale=0.4, text_padding=5)
        assert got[f][0] == want[0], f
        assert list(got[f][1]) == list(want[1]) and all(np.array_equal(got[f][1][k], want[1][k]) for k in want[1]), f
        assert np.array_equal(dev[f].numpy(), frames[f]), f


class _StubParser:
    """pipeline.ScreenParser on the host hand-off with the two model stages stubbed: everything `return_image` adds is the product's"""

    @staticmethod
    def make(monkeypatch):
        from omniparser_amd.pipeline import ScreenParser

        class P(ScreenParser):
            def detect(self, frames, pad_to=None):
                return [torch.tensor([[10., 12., 60., 40.], [80., 20., 150., 70.], [30., 50., 31., 52.]]) + 3 * k for k in range(len(frames))]

            def caption(self, frames, crops_per_frame, max_new_tokens=20):
                return [[(f"cap{k}", torch.tensor([k])) for k in range(len(c))] for c in crops_per_frame]

        stub = types.SimpleNamespace(_lock=contextlib.nullcontext(), device=torch.device("cpu"), stream=None)
        sp = P(stub, stub, processor=object())
        sp.device_glue = False
        return sp


@pytest.mark.parametrize("mode", ["device", "host", "skip"])
def test_parse_batch_return_image_on_the_emulated_tail(emu, monkeypatch, mode):
    """`parse_batch(return_image=True)` (host hand-off route, stubbed models, real overlay / PNG tail on the emulation): elements and
    ids are those of the call without the argument, the frames keep their bytes, every image decodes to the host raster `U.annotate`
    of the frame's elements, label coordinates are the host's.  OMNI_OVERLAY=host gives Pillow's PNG, OMNI_SKIP_ANNOTATE=1 gives ""."""
    from omniparser_amd.util import utils as U
    from omniparser_amd.util.omniparser import overlay_style
    monkeypatch.setenv("OMNI_OVERLAY", "host" if mode == "host" else "device")
    if mode == "skip":
        monkeypatch.setenv("OMNI_SKIP_ANNOTATE", "1")
    sp = _StubParser.make(monkeypatch)
    rng = np.random.default_rng(8)
    raw = [rng.integers(0, 256, (100, 180, 3), dtype=np.uint8) for _ in range(2)]
    frames = [torch.from_numpy(r.copy()) for r in raw]
    ocr = [(["File"], [[5, 80, 50, 95]]), ([], [])]
    plain = sp.parse_batch(frames, ocr, return_ids=True)
    elems, ids, marked = sp.parse_batch(frames, ocr, return_ids=True, return_image=True)
    assert elems == plain[0] and [[r.tolist() for r in f] for f in ids] == [[r.tolist() for r in f] for f in plain[1]]
    two = sp.parse_batch(frames, ocr, return_image=True)
    assert isinstance(two, tuple) and len(two) == 2 and two[0] == elems
    assert len(marked) == 2
    for f in range(2):
        assert np.array_equal(frames[f].numpy(), raw[f])
        bx = U._box_convert_xyxy_to_cxcywh(torch.tensor([e["bbox"] for e in elems[f]], dtype=torch.float32).reshape(-1, 4))
        host, coords = U.annotate(raw[f], bx, None, list(range(len(elems[f]))), **overlay_style((180, 100)))
        png, got = marked[f]
        assert list(got) == list(coords) and all(np.array_equal(got[k], coords[k]) for k in coords)
        if mode == "skip":
            assert png == ""
            continue
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(base64.b64decode(png))).convert("RGB")), host)
        if mode == "host":
            assert png == U.encode_png_b64(host)
        else:
            assert png == U.annotate_encode_device(raw[f], bx, list(range(len(elems[f]))), "cpu", **overlay_style((180, 100)))[0]

"""bench.py --dump-outputs: the arrays written for the last timed step (bench.dump_outputs), on hand-made step results — e2e element
lists with caption ids, and a detect-mode plan whose output buffers hold scratch past the kept count."""
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

import bench  # noqa: E402
from omniparser_amd import dist as OD  # noqa: E402


def _load(d):
    out = {p.stem: np.load(p) for p in sorted(d.glob("*.npy"))}
    assert all(a.dtype in (np.float32, np.float64) for a in out.values())
    return out


def test_dump_e2e_elements_and_caption_ids(tmp_path):
    elems = [[{"bbox": [0.1, 0.2, 0.3, 0.4], "source": "box_ocr_content_ocr", "interactivity": False, "content": "ok"},
              {"bbox": [0.5, 0.5, 0.6, 0.6], "source": "box_yolo_content_yolo", "interactivity": True, "content": "a"},
              {"bbox": [0.0, 0.0, 0.1, 0.1], "source": "box_yolo_content_ocr", "interactivity": True, "content": "b "},
              {"bbox": [0.7, 0.1, 0.8, 0.2], "source": "box_yolo_content_yolo", "interactivity": True, "content": "c"}],
             []]
    ids = [[torch.tensor([2, 0, 5, 7]), np.array([2, 9])], []]
    names = bench.dump_outputs(tmp_path, SimpleNamespace(batch=2), {"elems": elems, "ids": ids})
    a = _load(tmp_path)
    assert sorted(a) == names == ["boxes", "caption_ids", "count", "interactive", "source"]
    MD, CT = OD.MAX_DET, OD.CAP_TOK
    assert a["count"].tolist() == [4, 0]
    assert a["boxes"].shape == (2, MD, 4) and a["boxes"].dtype == np.float64
    assert a["boxes"][0, :4].tolist() == [e["bbox"] for e in elems[0]] and not a["boxes"][0, 4:].any() and not a["boxes"][1].any()
    assert a["source"][0, :5].tolist() == [0, 2, 1, 2, -1]
    assert a["interactive"][0, :5].tolist() == [0, 1, 1, 1, 0]
    assert a["caption_ids"].shape == (2, MD, CT)
    # the ids rows go to the captioned icons (source box_yolo_content_yolo) in element order
    assert a["caption_ids"][0, 1, :5].tolist() == [2, 0, 5, 7, -1]
    assert a["caption_ids"][0, 3, :3].tolist() == [2, 9, -1]
    assert (a["caption_ids"][0, [0, 2]] == -1).all() and (a["caption_ids"][1] == -1).all()


def test_dump_detect_zeroes_rows_past_the_count(tmp_path):
    B, MD = 2, OD.MAX_DET
    g = torch.Generator().manual_seed(0)
    dp = SimpleNamespace(out_count=torch.tensor([3, 1], dtype=torch.int32), out_boxes=torch.rand(B, MD, 4, generator=g) * 100,
                         out_scores=torch.rand(B, MD, generator=g), out_cls=torch.randint(0, 5, (B, MD), generator=g, dtype=torch.int32))
    bench.dump_outputs(tmp_path, SimpleNamespace(batch=B), {}, dp)
    a = _load(tmp_path)
    assert sorted(a) == ["boxes", "cls", "count", "scores"]
    assert a["count"].tolist() == [3, 1]
    for j, k in enumerate((3, 1)):
        assert np.array_equal(a["boxes"][j, :k], dp.out_boxes[j, :k].numpy()) and not a["boxes"][j, k:].any()
        assert np.array_equal(a["scores"][j, :k], dp.out_scores[j, :k].numpy()) and not a["scores"][j, k:].any()
        assert a["cls"][j, :k].tolist() == dp.out_cls[j, :k].tolist() and not a["cls"][j, k:].any()

"""bench.py without --full: set-up, warm-up, the timed steps, --dump-outputs and the line, nothing else; --full adds `roofline`,
`extra` and `cpu_baseline` after the timed region.  One rank, detect mode at the debug sizes of tests/test_bench_world2_cpu.py, the
product's device path on the host emulation (tests/emu); what --full adds is stubbed here (it times the GPU), only its dispatch is
checked."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

import bench  # noqa: E402

ARGS = ["--gpus", "1", "--steps", "1", "--warmup", "1", "--mode", "detect", "--batch", "1", "--width", "0.25", "--frame", "640x480",
        "--imgsz", "320"]


@pytest.mark.parametrize("full", [False, True], ids=["plain", "full"])
def test_only_full_runs_what_the_headline_does_not_need(full, emu, monkeypatch, capfd, tmp_path):
    from tools.make_weights import ensure_blob
    ensure_blob(seed=0, nc=1, width=0.25)
    ran = []
    for name in ("roofline", "extras", "cpu_baseline", "child_json"):
        monkeypatch.setattr(bench, name, lambda *a, _name=name, **k: ran.append(_name) or {"stub": _name})
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a, **k: None)
    monkeypatch.setattr(torch.cuda, "max_memory_allocated", lambda *a, **k: 0)
    monkeypatch.setattr(bench, "IW", bench.IW)                 # main() sets them from --frame
    monkeypatch.setattr(bench, "IH", bench.IH)
    monkeypatch.setenv("OMNI_WEIGHTS_DIR", "")                 # restored (unset) after the test: bench.py sets it
    monkeypatch.setenv("OMNI_VERIFY_IMPORT", "0")
    monkeypatch.setattr(sys, "argv", ["bench.py", *ARGS, "--dump-outputs", str(tmp_path)] + (["--full"] if full else []))
    bench.main()
    lines = [l for l in capfd.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 1 and d["warmup"] == 1 and d["value"] > 0 and d["unit"] == "screenshots/s"
    assert abs(d["value"] - 1 / (d["ms_per_step"] / 1000.0)) < 1e-3 * d["value"] + 1e-3
    assert np.load(tmp_path / "count.npy").shape == (1,)
    if full:
        assert ran == ["roofline", "extras", "cpu_baseline"]
        assert d["roofline"] == {"stub": "roofline"} and d["extra"] == {"stub": "extras"} and d["cpu_baseline"] == {"stub": "cpu_baseline"}
    else:
        assert ran == [] and not {"roofline", "extra", "cpu_baseline"} & set(d)

"""Cost of beam-search captioning at the benched load: 8 synthetic 1920x1080 screenshots, 768x768 crops, ~345 crops per batch, through
ScreenParser.caption (micro-batched encode + ONE merged decode plan, the bench's caption path) with the captioner's num_beams = 1 and 3.
Prints one JSON line per beam width: caption ms per batch and per screenshot, merged-decode ms (20 steps) and ms per step, HBM held by the
allocator (peak and resident).  MI355X only: `python tools/beam_bench.py [--beams 1,3] [--reps 3]`; run one width per process for HBM
figures that hold nothing of another width's plans."""
import argparse
import gc
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def boxes_for(seed, n, iw=1920, ih=1080):
    rng = np.random.default_rng(1000 + seed)
    out = []
    for _ in range(n):
        s, t = int(rng.integers(18, 96)), int(rng.integers(18, 96))
        x0, y0 = int(rng.integers(0, iw - s)), int(rng.integers(0, ih - t))
        out.append([x0, y0, x0 + s, y0 + t])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--beams", default="1,3")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--crops", type=int, default=345)
    a = ap.parse_args()
    from omniparser_amd.florence import Florence2Captioner
    from omniparser_amd.pipeline import ScreenParser
    from omniparser_amd.synth import synthetic_screenshot
    from tools.make_weights import ensure_caption_checkpoint
    frames = [torch.from_numpy(synthetic_screenshot(s)).cuda() for s in range(a.frames)]
    per = [a.crops // a.frames + (1 if i < a.crops % a.frames else 0) for i in range(a.frames)]
    boxes = [boxes_for(i, n) for i, n in enumerate(per)]
    cap = Florence2Captioner(ensure_caption_checkpoint(0), "cuda", precision="f32", resolution=768)
    sp = ScreenParser(None, cap)
    for k in [int(x) for x in a.beams.split(",")]:
        cap.num_beams = k
        cap.clear_plans()
        gc.collect()                                   # plan objects hold reference cycles
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        sp.caption(frames, boxes)                      # builds and captures the plans
        torch.cuda.synchronize()
        wall, dec = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            sp.caption(frames, boxes)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
            dec.append(sp._ev["cap1"].elapsed_time(sp._ev["cap2"]))
        res = {"num_beams": k, "frames": a.frames, "crops": sum(per), "resolution": 768, "reps": a.reps,
               "caption_ms": round(float(np.median(wall)), 2), "caption_ms_per_screenshot": round(float(np.median(wall)) / a.frames, 2),
               "decode_ms": round(float(np.median(dec)), 2), "decode_step_ms": round(float(np.median(dec)) / 20, 3),
               "hbm_peak_gb": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2),
               "hbm_resident_gb": round(torch.cuda.memory_allocated() / 2 ** 30, 2)}
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()

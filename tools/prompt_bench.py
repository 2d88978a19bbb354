#!/usr/bin/env python
"""What a caption prompt costs on the MI355X: `Florence2Captioner.caption_crops` over 345 crops of one 1920x1080 screenshot at
768x768 with the default prompt (constant block, 585 encoder tokens), a prompt of 11 tokens (text capacity 16: 593 tokens) and one
of 64 tokens (capacity 64: 641 tokens), timed with device events after a warm-up call that builds and captures the plans.
One JSON line per prompt.  Expectation to compare against (not a gate): the encoder tokens grow by 593/585 and 641/585, the
encoder GEMMs linearly and its attention quadratically with that; the vision tower, most of a crop's work, does not change.

    python tools/prompt_bench.py [--crops 345] [--reps 5]"""
import argparse
import gc
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--crops", type=int, default=345)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    from omniparser_amd.florence import PROMPT_IDS, Florence2Captioner, text_capacity
    from omniparser_amd.synth import synthetic_screenshot
    from tools.make_weights import ensure_caption_checkpoint
    rng = np.random.default_rng(7)
    frame = torch.from_numpy(synthetic_screenshot(14)).cuda()
    boxes = []
    for _ in range(a.crops):
        s, t = int(rng.integers(18, 96)), int(rng.integers(18, 96))
        x0, y0 = int(rng.integers(0, 1920 - s)), int(rng.integers(0, 1080 - t))
        boxes.append([x0, y0, x0 + s, y0 + t])
    g = torch.Generator().manual_seed(1234)
    prompts = {"default": None}
    for n in (11, 64):
        prompts[f"{n} tokens"] = [0] + torch.randint(4, 50000, (n - 2,), generator=g).tolist() + [2]
    cap = Florence2Captioner(ensure_caption_checkpoint(0), "cuda", precision="f32", resolution=768)
    base = None
    for name, ids in prompts.items():
        cap.clear_plans()
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        cap.caption_crops(frame, boxes, prompt_ids=ids)          # builds and captures the plans
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            cap.caption_crops(frame, boxes, prompt_ids=ids)      # ends in a read-back of the ids: the work has finished
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        n_txt = len(PROMPT_IDS) if ids is None else text_capacity(len(ids))
        med = float(np.median(ms))
        base = base or med
        print(json.dumps({"prompt": name, "text_capacity": n_txt, "encoder_tokens": 577 + n_txt, "crops": a.crops, "reps": a.reps,
                          "caption_ms": round(med, 2), "min_ms": round(min(ms), 2), "max_ms": round(max(ms), 2),
                          "ratio_to_default": round(med / base, 4), "token_ratio": round((577 + n_txt) / 585, 4)}), flush=True)


if __name__ == "__main__":
    main()

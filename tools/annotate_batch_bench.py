"""Measure the batched overlay + PNG tail (`ScreenParser.parse_batch / parse_stream(return_image=True)`) on 8 synthetic 1920x1080
frames with the elements the pipeline really produces for them:

  tail    (a) the per-frame way: `U.annotate_encode_device` once per frame after `parse_batch` (one stream, 9 launches and one blocking
              read per frame) against (b) the batched tail standalone (`U.annotate_encode_device_batch`: one overlay launch, one deflate
              chain, one read of the sizes), interleaved a, b, a, b ... in one process; the strings of (a) and (b) must be equal.
              Also: PNG file bytes per frame and the HBM the scratch holds.
  stream  (c) milliseconds per step of `parse_stream` without and with `return_image`, interleaved in one process, and the device
              time of the annotate stage from its HIP events (`parse_batch`, `stats["stage_ms"]["annotate"]`).

Without `--step` this is the driver: every step runs in a child process of its own under `timeout`, the output of every child is
appended to `--out` (default profiles/annotate_batch_mi355x.txt), and the first non-zero status ends the run with that status.
`python tools/annotate_batch_bench.py [--width 1.0] [--caption-res 768] [--iters 5] [--rounds 2] [--steps 6]`"""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

STEPS = (("tail", 420), ("stream", 540))          # name, time limit in seconds


def build(a):
    import torch
    from omniparser_amd.florence import Florence2Captioner
    from omniparser_amd.pipeline import ScreenParser
    from omniparser_amd.synth import BENCH_SEEDS, synthetic_ocr, synthetic_screenshot
    from omniparser_amd.util.yolov9 import YOLOv9Detector
    from tools.make_weights import ensure_blob, ensure_caption_checkpoint
    dev = torch.device("cuda", 0)
    det = YOLOv9Detector(model_path=ensure_blob(seed=0, nc=1, width=a.width), device=dev, precision="f32")
    cap = Florence2Captioner(ensure_caption_checkpoint(0), dev, precision="f32", resolution=a.caption_res)
    sp = ScreenParser(det, cap, box_threshold=0.05, iou_threshold=0.7, nms_iou=0.1, max_det=300, imgsz=640)
    W, H = 1920, 1080
    seeds = BENCH_SEEDS[:8]
    frames = [torch.from_numpy(synthetic_screenshot(s, W, H)).to(dev) for s in seeds]
    ocr = [synthetic_ocr(s, W, H, 40) for s in seeds]
    return sp, frames, ocr, dev, W, H


def step_tail(a):
    import torch
    from omniparser_amd.util import utils as U
    from omniparser_amd.util.omniparser import overlay_style
    sp, frames, ocr, dev, W, H = build(a)
    with torch.inference_mode():
        elems = sp.parse_batch(frames, ocr)
        boxes = [U._box_convert_xyxy_to_cxcywh(torch.tensor([e["bbox"] for e in el], dtype=torch.float32).reshape(-1, 4)) for el in elems]
        phrases = [list(range(len(el))) for el in elems]
        style = overlay_style((W, H))
        torch.cuda.synchronize()
        hbm0 = torch.cuda.memory_allocated(dev)
        sc = U.AnnotateScratch(len(frames), H, W, dev)
        hbm1 = torch.cuda.memory_allocated(dev)

        def per_frame(copies):                           # the in-place raster draws on the request's own upload: fresh copies per run
            return [U.annotate_encode_device(None, b, p, dev, frame_dev=c, **style)[0] for b, p, c in zip(boxes, phrases, copies)]

        def batched():
            return [s for s, _ in U.annotate_encode_device_batch(frames, boxes, phrases, scratch=sc, **style)]

        def timed(fn, per_run=None):
            ms = []
            for _ in range(a.iters):
                args = () if per_run is None else (per_run(),)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = fn(*args)
                torch.cuda.synchronize()
                ms.append(1000 * (time.perf_counter() - t0))
            return out, ms

        clones = lambda: [f.clone() for f in frames]
        ref = per_frame(clones())
        got = batched()                                  # warm-up of both, and the check
        out = {"step": "tail", "frames": len(frames), "frame": f"{W}x{H}", "elements_per_frame": [len(e) for e in elems],
               "batched_strings_equal_per_frame_strings": ref == got, "rounds": []}
        for _ in range(a.rounds):
            _, ms_a = timed(per_frame, clones)
            _, ms_b = timed(batched)
            out["rounds"].append({"a_per_frame_loop_ms": [round(v, 2) for v in ms_a], "b_batched_tail_ms": [round(v, 2) for v in ms_b]})
        med = lambda key: sorted(v for r in out["rounds"] for v in r[key])[len(out["rounds"]) * a.iters // 2]
        out["a_per_frame_loop_ms_median"], out["b_batched_tail_ms_median"] = round(med("a_per_frame_loop_ms"), 2), round(med("b_batched_tail_ms"), 2)
        out["b_over_a"] = round(out["b_batched_tail_ms_median"] / out["a_per_frame_loop_ms_median"], 3)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        h = U.annotate_encode_device_batch_launch(frames, boxes, phrases, scratch=sc, **style)
        e1.record()
        U.annotate_encode_device_batch_finish(h)
        out["b_device_ms_overlay_plus_deflate_chain"] = round(e0.elapsed_time(e1), 3)
        out["png_file_bytes_per_frame"] = [int(v) for v in sc.meta[:, 1].cpu().tolist()]
        out["hbm"] = {"allocated_before_scratch_gb": round(hbm0 / 1e9, 3), "allocated_after_scratch_gb": round(hbm1 / 1e9, 3),
                      "scratch_mb_per_frame": round(sc.nbytes() / len(frames) / 1e6, 1)}
    print(json.dumps(out), flush=True)
    return 0 if out["batched_strings_equal_per_frame_strings"] else 1


def step_stream(a):
    import torch
    sp, frames, ocr, dev, W, H = build(a)

    def batches(n):
        for _ in range(n):
            yield frames, ocr

    def run(n, **kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        last = None
        for last in sp.parse_stream(batches(n), **kw):
            pass
        torch.cuda.synchronize()
        return 1000 * (time.perf_counter() - t0) / n, last

    with torch.inference_mode():
        run(4)                                           # the plan sets of the steady state (two encode lanes, two decode plans)
        hbm0 = torch.cuda.memory_allocated(dev)
        _, (elems, marked) = run(4, return_image=True)   # + the two scratch sets
        hbm1 = torch.cuda.memory_allocated(dev)
        out = {"step": "stream", "frames_per_step": len(frames), "frame": f"{W}x{H}", "steps_per_run": a.steps, "rounds": []}
        for _ in range(a.rounds):
            plain, _ = run(a.steps)
            img, _ = run(a.steps, return_image=True)
            out["rounds"].append({"parse_stream_ms_per_step": round(plain, 2), "with_return_image_ms_per_step": round(img, 2)})
        out["c_added_ms_per_step"] = round(sorted(r["with_return_image_ms_per_step"] - r["parse_stream_ms_per_step"] for r in out["rounds"])[a.rounds // 2], 2)
        sp.parse_batch(frames, ocr, return_image=True)
        out["parse_batch_stage_ms"] = sp.stats.get("stage_ms", {})
        out["base64_chars_per_frame"] = [len(s) for s, _ in marked]
        out["hbm"] = {"allocated_before_return_image_gb": round(hbm0 / 1e9, 3), "allocated_after_gb": round(hbm1 / 1e9, 3),
                      "annotate_scratch_gb": round(sp.annotate_hbm_bytes() / 1e9, 3), "peak_allocated_gb": round(torch.cuda.max_memory_allocated(dev) / 1e9, 2)}
    print(json.dumps(out), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=[s for s, _ in STEPS], default=None)
    ap.add_argument("--width", type=float, default=1.0, help="detector channel multiplier (1.0 = YOLOv9-E, what bench.py runs)")
    ap.add_argument("--caption-res", type=int, default=768, choices=[64, 768])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "annotate_batch_mi355x.txt"))
    a = ap.parse_args()
    if a.step is not None:
        return {"tail": step_tail, "stream": step_stream}[a.step](a)
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    with out.open("w") as f:
        for name, limit in STEPS:
            cmd = ["timeout", "-k", "10", str(limit), sys.executable, str(Path(__file__).resolve()), "--step", name, "--width", str(a.width),
                   "--caption-res", str(a.caption_res), "--iters", str(a.iters), "--rounds", str(a.rounds), "--steps", str(a.steps)]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            f.write(r.stdout)
            f.flush()
            sys.stdout.write(r.stdout)
            if r.returncode != 0:                            # a fault, an abort or a time limit: nothing more is started on the GPU
                print(f"step {name} ended with status {r.returncode}: stopping", file=sys.stderr)
                return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())

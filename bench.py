#!/usr/bin/env python
"""bench.py — screenshots/sec of the MI355X screen-parsing hot path (BASELINE.json metric).

Contract: `python bench.py --gpus N --steps K --warmup W` — for N>1 either under torch.distributed.run (one rank per
GPU, the environment it sets is used as is) or plainly, in which case this script spawns its N ranks itself
(`omniparser_amd.dist.self_launch`).  A *step* is one pass of the hot path over one batch of synthetic 1920x1080 screenshots that
are already resident in HBM as RGB bytes:

  --mode e2e (default; BASELINE configs[2]): batch of 8 screenshots -> Pillow-exact Lanczos letterbox ->
      YOLOv9-E -> decode + NMS -> reference glue (overlap removal vs a synthetic OCR fixture) -> crop,
      cv2-bilinear 64x64, Pillow-bicubic to 768x768 (the reference's CPU-path crop size = the parity
      target; --caption-res 64 is its cuda branch) -> Florence-2 (DaViT + BART encoder) -> 20-step greedy
      decode.  Output: parsed element lists (boxes + caption ids).  Annotated-PNG rendering is a caller-side
      visual and is not part of the timed path.
  --mode detect (BASELINE configs[1]): detector stage only, batch 1.

W untimed warm-up steps, exactly K timed steps between barrier+synchronize pairs, MAX over ranks, rank 0
prints ONE JSON line; `value` = screenshots of all ranks / that time.  Screenshots shard across ranks with
no data-path collective; the only exchange is one all_gather of packed element records per job.  A plain run does
that and nothing else (besides --dump-outputs).

--full adds, after the timed region: `roofline` (dominant kernel family = the GEMMs: algorithmic conv/linear FLOPs per
step at the REAL crop count / HIP-event time of exactly those launches timed in sequence, vs the dense f16 MFMA peak),
`extra` (N=1: BASELINE configs[1] detector-only at both network sizes, the 64x64 crop size, configs[4] tiled 4K, and
unless --no-ab the child-process lines), `cpu_baseline` (the reference-equivalent CPU path from oracle/, timed on rank 0
at N=1 on a bounded sample) and `config.parity_scan` (the committed record of the GPU-vs-oracle scan, quoted while it
still describes this tree).  --no-extra and --no-cpu-baseline trim a --full run.
Weights are seeded-random (tools/make_weights.py); data is synthetic (omniparser_amd/synth.py).

--dump-outputs DIR: after the timed steps, rank 0 writes what the timed path returned in its last step as DIR/<name>.npy (float32 /
float64; see dump_outputs), so that two builds run with the same arguments can be compared output for output.
"""
import argparse
import json
import os
import re
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=None)
    ap.add_argument("--mode", default="e2e", choices=["e2e", "detect"])
    ap.add_argument("--batch", type=int, default=None, help="screenshots per step (e2e default 8, detect default 1)")
    ap.add_argument("--precision", default=os.environ.get("OMNI_PRECISION", "f32"), choices=["f32", "f16"])
    ap.add_argument("--caption-res", type=int, default=768, choices=[64, 768])
    ap.add_argument("--imgsz", default="640", help="'640' (reference default) or 'native' (1088x1920 network input)")
    ap.add_argument("--full", action="store_true", help="after the timed steps, also measure and check what the headline figure does not need: "
                    "`roofline`, `extra`, `cpu_baseline`, `config.parity_scan`")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip `cpu_baseline`")
    ap.add_argument("--micro-batch", type=int, default=int(os.environ.get("OMNI_CAPTION_MICRO_BATCH", "128")), choices=[32, 64, 96, 128],
                    help="crops per caption micro-batch (plan capacity; the reference's batch_size = 128, ref:util/utils.py:89)")
    ap.add_argument("--no-extra", action="store_true", help="with --full: skip the `extra` object (configs[1], 64x64 crops, tiled 4K)")
    ap.add_argument("--no-pipeline", dest="pipeline", action="store_false",
                    help="time K synchronous parse_batch calls instead of the K steps through ScreenParser.parse_stream (the default: "
                         "detector of step i+1, two encode lanes and the decode of step i overlap; same kernels, same results)")
    ap.add_argument("--pipeline", dest="pipeline", action="store_true", help=argparse.SUPPRESS)
    ap.set_defaults(pipeline=True)
    ap.add_argument("--lanes", type=int, default=2, choices=[1, 2, 3, 4], help="with --pipeline: caption micro-batches in flight at once (HIP streams); "
                    "3 / 4: experiments (each lane holds its own 128-row encode plans, ~25 GB each at 768x768 crops)")
    ap.add_argument("--no-ab", action="store_true", help="with --full: skip the child-process measurements (`extra.e2e_r64_f16_reference_cuda_branch`, `extra.annotate_tail`, `extra.stream_*`)")
    ap.add_argument("--width", type=float, default=1.0, help="debug only: detector channel multiplier (1.0 = YOLOv9-E)")
    ap.add_argument("--frame", default="1920x1080", help="debug only: synthetic frame size WxH (the metric is quoted on 1920x1080; the CPU test "
                    "of the N > 1 path runs a small frame on the host emulation)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the timed path returned in its last step (rank 0) as DIR/<name>.npy (float32 / float64)")
    a = ap.parse_args()
    if a.batch is None:
        a.batch = 8 if a.mode == "e2e" else 1
    if a.steps is None:
        a.steps = 3 if (a.mode == "e2e" and a.caption_res == 768) else (10 if a.mode == "e2e" else 200)
    if a.warmup is None:
        a.warmup = 1 if a.mode == "e2e" else 20
    return a


IW, IH = 1920, 1080
CONF, NMS_IOU, OVERLAP_IOU, MAX_DET = 0.05, 0.1, 0.7, 300   # ref:util/omniparser.py:30, ref:util/utils.py:431


_T0 = time.perf_counter()


def note(msg):
    """progress line on stderr (the JSON line on stdout stays the only stdout output)"""
    print(f"[bench {time.perf_counter() - _T0:7.1f}s] {msg}", file=sys.stderr, flush=True)


def main():
    args = parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` with no launcher: this process spawns the N ranks itself (one per GPU, RCCL rendezvous on 127.0.0.1) and
        # relays rank 0's JSON line; under `python -m torch.distributed.run` the environment is already there and nothing is spawned
        from omniparser_amd.dist import self_launch
        sys.exit(self_launch(args.gpus))
    import faulthandler
    faulthandler.dump_traceback_later(int(os.environ.get("OMNI_BENCH_WATCHDOG", "240")), repeat=True, file=sys.stderr)   # where is it, if it stalls
    import torch
    import torch.distributed as dist
    from omniparser_amd import _lib as L
    from omniparser_amd import dist as OD
    from omniparser_amd.synth import BENCH_SEEDS, synthetic_ocr, synthetic_screenshot
    from omniparser_amd.util.yolov9 import YOLOv9Detector

    rank, world, local_rank = OD.init_from_env()
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"
    if world > 1:
        # N processes share the host: without a cap every rank's CPU-side torch ops (hand-off tables, record packing, tokenizer glue)
        # spawn one worker per core of the whole box and the ranks thrash each other
        torch.set_num_threads(max(1, (os.cpu_count() or world) // world))
    load_native()
    dev = L.require_device(torch.device("cuda", local_rank), "bench.py")       # the MI355X or nothing (no CPU fallback)
    torch.cuda.set_device(local_rank)
    global IW, IH
    IW, IH = (int(v) for v in args.frame.split("x"))
    imgsz = int(args.imgsz) if args.imgsz.isdigit() else (IH, IW)
    # stand-in checkpoints are INPUT FILES (the reference downloads its weights): generated once, in a separate
    # process, by tools/make_weights.py — this process never imports oracle/ outside cpu_baseline()
    blob, cap_dir = standin_checkpoints(args, rank, world)
    assert blob.exists(), blob
    note("stand-in checkpoints ready")
    det = YOLOv9Detector(model_path=blob, device=dev, precision=args.precision)
    note("detector loaded (blob imported and verified against itself)")
    B = args.batch
    frames = [torch.from_numpy(synthetic_screenshot(s, IW, IH)).to(dev) for s in BENCH_SEEDS]
    ocr = [synthetic_ocr(s, IW, IH, 40) for s in BENCH_SEEDS]
    n_items = args.steps * B * world
    my_items = OD.shard_indices(args.steps * world, rank, world)      # step-granular round robin
    assert len(my_items) == args.steps

    parser = None
    if args.mode == "e2e":
        from omniparser_amd.florence import Florence2Captioner
        from omniparser_amd.pipeline import ScreenParser
        cap = Florence2Captioner(cap_dir, dev, precision=args.precision, resolution=args.caption_res)
        parser = ScreenParser(det, cap, box_threshold=CONF, iou_threshold=OVERLAP_IOU, nms_iou=NMS_IOU, max_det=MAX_DET, imgsz=imgsz,
                              batch_size=args.micro_batch)
        parser.encode_lanes = args.lanes
    else:
        dp = det.get_plan(IW, IH, imgsz, CONF, NMS_IOU, MAX_DET, batch=B)

    recs = torch.zeros(args.steps * B, OD.REC_W, dtype=torch.int32, device=dev)
    crop_counts = []
    last = {}                            # what the timed path returned in its most recent step (e2e: elements + caption ids)

    @torch.inference_mode()
    def step(step_id, li=None):
        idx = [(step_id * B + j) % 8 for j in range(B)]
        if args.mode == "detect":
            with torch.cuda.stream(det.stream):
                for j, f in enumerate(idx):
                    dp.img[j].copy_(frames[f], non_blocking=True)
                dp.launch(det)
                if li is not None:
                    for j in range(B):
                        r = recs[li * B + j]
                        r[0] = step_id * B + j
                        r[1:2] = dp.out_count[j:j + 1]
                        r[2:2 + 4 * MAX_DET] = dp.out_boxes[j].view(torch.int32).flatten()
                        r[2 + 4 * OD.MAX_DET:2 + 5 * OD.MAX_DET] = dp.out_scores[j].view(torch.int32)
                        r[2 + 5 * OD.MAX_DET:2 + 6 * OD.MAX_DET] = dp.out_cls[j]
            return
        elems, ids = parser.parse_batch([frames[f] for f in idx], [ocr[f] for f in idx], return_ids=True)
        pack(step_id, li, elems, ids)

    step_done = []                       # host clock when each step's results were in hand (diagnostic: a cold first process shows here)

    def pack(step_id, li, elems, ids):
        step_done.append(time.perf_counter())
        crop_counts.append(sum(parser.stats["crops"]))
        last["elems"], last["ids"] = elems, ids
        if li is not None:
            pack_records(recs, B, dev, step_id, li, elems, ids)

    def sync_all():
        det.stream.synchronize()
        torch.cuda.synchronize(dev)
        if world > 1:
            dist.barrier()

    if args.pipeline and args.mode == "e2e":
        # warm-up through the same pipeline (its second-lane encode plans and second decode plan are built here, not in the timed region)
        def warm_batches():
            # (at least 4: the plan sets of the steady state exist after the second lane has seen the step's remainder micro-batch twice —
            # two 128-row plan sets, their exact-row twins (florence.py::_CaptionPlans.rows_for), two decode plans; the driver passes 5)
            for w in range(max(args.warmup, 4)):
                idx = [(w * B + j) % 8 for j in range(B)]
                yield [frames[f] for f in idx], [ocr[f] for f in idx]
        with torch.inference_mode():
            for w, _ in enumerate(parser.parse_stream(warm_batches(), return_ids=True)):
                note(f"warm-up step {w} done (pipelined)")
    else:
        for w in range(args.warmup):
            step(w)
            note(f"warm-up step {w} done")
    sync_all()
    crop_counts.clear()
    step_done.clear()
    import gc
    gc_mode = os.environ.get("OMNI_BENCH_GC", "on")          # diagnostic for the one-step-in-twenty +40 ms outlier: off | freeze | on
    if gc_mode == "off":
        gc.disable()
    elif gc_mode == "freeze":
        gc.collect(); gc.freeze()
    gc_before = [g["collections"] for g in gc.get_stats()]
    t0 = time.perf_counter()
    if args.pipeline and args.mode == "e2e":
        # the same K steps as a software pipeline over batches (ScreenParser.parse_stream): detector + hand-off of step i+1 overlap
        # the captions of step i, the caption work of step i+1 is queued before step i is read back
        def batches():
            for item in my_items:
                idx = [(item * B + j) % 8 for j in range(B)]
                yield [frames[f] for f in idx], [ocr[f] for f in idx]
        with torch.inference_mode():
            for li, (elems, ids) in enumerate(parser.parse_stream(batches(), return_ids=True)):
                pack(my_items[li], li, elems, ids)
    else:
        for li, item in enumerate(my_items):
            step(item, li)
    with torch.cuda.stream(det.stream):
        allr = OD.gather_records(recs, n_items, rank, world)
    sync_all()
    elapsed = time.perf_counter() - t0
    gc_runs = [g["collections"] - b for g, b in zip(gc.get_stats(), gc_before)]
    if gc_mode == "off":
        gc.enable()
    note(f"timed region done: {elapsed:.2f} s for {args.steps} steps (gc {gc_mode}: collections per generation {gc_runs})")
    if args.dump_outputs and rank == 0:
        # outside the timed region, before anything else runs on the plans whose output buffers hold the last step's results
        names = dump_outputs(Path(args.dump_outputs), args, last, dp if args.mode == "detect" else None)
        note(f"outputs of the last timed step written to {args.dump_outputs}: {names}")
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    value = n_items / elapsed
    kept = allr[:, 1].float().mean().item()

    workload = ("BASELINE configs[2]: full detect -> crop -> Florence-2 caption, batch=%d screenshots, greedy decode, caption crops %dx%d"
                % (B, args.caption_res, args.caption_res)) if args.mode == "e2e" else \
        "BASELINE configs[1]: YOLOv9-E icon_detect only, batch=%d, 1920x1080 (letterbox+network+decode+NMS)" % B
    out = {
        "metric": "screenshots/sec end-to-end (detect+caption) @1920x1080",
        "value": round(value, 4), "unit": "screenshots/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(1000.0 * elapsed / args.steps, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        # what the path computes in: f32 storage, accumulation and statistics; the GEMMs multiply on the f16 matrix cores with every f32
        # operand split into two f16 halves and three products per MAC (f32-class accuracy, measured < 2e-6 relative; NOT IEEE f32 products)
        "dtype": "f32 (split-f16x3 MFMA)" if (args.precision == "f32" and os.environ.get("OMNI_CONV_SPLIT", "1") == "1") else args.precision,
        "data": "synthetic 1920x1080 GUI-like screenshots (seeds %s) + synthetic OCR boxes; seeded random-weight YOLOv9-E blob " % (list(BENCH_SEEDS),) +
                "and Florence-2-base-shaped checkpoint",
        "config": {
            "workload": workload, "screenshots_per_step": B,
            "network_input": f"{imgsz}x{imgsz}" if isinstance(imgsz, int) else "1088x1920",
            "conf": CONF, "nms_iou": NMS_IOU, "overlap_iou": OVERLAP_IOU, "max_det": MAX_DET,
            "parallelism": f"replicas x{world}, round-robin shards of steps, 1 all_gather/job",
            "hipgraph": det.use_graph, "mean_elements_per_screenshot": round(kept, 2),
            "gemm_tile_order": "xcd row blocks + N partition (L2-resident weight slabs)",
            "gemm_path": ("split-f16 x3 MFMA (f32-class accuracy): pre-split LDS-DMA GEMM for the captioner's linear layers, "
                          "register-staged split kernel for convs / decoder steps" if args.precision == "f32" and
                          os.environ.get("OMNI_CONV_SPLIT", "1") == "1" else
                          ("exact f32 MFMA" if args.precision == "f32" else "f16 MFMA")),
        },
    }
    if args.mode == "e2e":
        out["config"]["mean_crops_per_screenshot"] = round(sum(crop_counts) / max(len(crop_counts), 1) / B, 2)
        out["config"]["caption_micro_batch"] = args.micro_batch
        from omniparser_amd.florence import _BUCKETS
        out["config"]["caption_plan_capacities"] = list(_BUCKETS)
        out["config"]["caption_remainder"] = ("exact rows: a second hipGraph over the first n rows of the lane's full-capacity plan set "
                                              "(florence.py::_CaptionPlans.encode_rows)" if parser.cap.exact_rows else "padded to the next plan capacity")
        out["config"]["steps_pipelined"] = bool(args.pipeline)
        out["config"]["warmup_steps_run"] = max(args.warmup, 4) if args.pipeline else args.warmup     # pipelined: >= 4 untimed steps (plan sets of the steady state)
        # wall time between consecutive steps' results inside the timed region (pipelined: step i's results arrive while step i+1 runs)
        out["config"]["step_wall_ms"] = [round(1000.0 * (b - a), 1) for a, b in zip([t0] + step_done[:-1], step_done)][:40]
        out["config"]["hw_queues"] = os.environ.get("GPU_MAX_HW_QUEUES", "HIP runtime default (4)")
        out["config"]["python_gc"] = {"mode": gc_mode, "collections_in_timed_region": gc_runs}
        if args.pipeline:
            out["config"]["pipeline"] = ("parse_stream: detector + hand-off graph of step i+1 on the detector's stream, caption micro-batches alternating "
                                         "over %d encode stream(s), the 20 decode steps of step i on their own stream (two decode plans)" % args.lanes)
        out["config"]["decode"] = ("one 20-step decode over all crops of the batch (cross-attention K/V of every micro-batch copied into one plan)"
                                   if os.environ.get("OMNI_MERGED_DECODE", "1") != "0" else "per micro-batch")
        out["config"]["text"] = "caption ids -> strings (tokenizers batch_decode + strip, ref:util/utils.py:128-130) inside the timed region (pipeline.py::caption_finish)"
        out["config"]["frames"] = "8 device-resident frames reused every step (inputs in HBM when the timed region starts); --full's extra.e2e_pcie_inclusive uploads them per step"
        out["config"]["hand_off"] = "device (detector + hand-off ops in one hipGraph)" if getattr(parser, "device_glue", False) else "host"
    # parity of the benched composition on frames the stand-in's calibration never saw — quoted from the committed record of the measured
    # scan (tools/scan_gpu_vs_oracle.py: the oracle's final lists computed in the CPU container, the detector + hand-off on the MI355X), not
    # measured by this run; the benched frames themselves are asserted element for element in tests/test_gpu_z_bench_path.py
    # The citation is dropped unless the scan's recorded provenance still describes this tree: same conv tuning table (it decides the
    # order in which 84 conv shapes sum their K partials) and same kernel sources (round 5 quoted a scan measured before
    # the tuning table existed).
    scans = sorted((ROOT / "profiles").glob("r*_scan_gpu_vs_oracle.json"), key=lambda p: [int(t) if t.isdigit() else t for t in re.split(r"(\d+)", p.name)])
    if args.full and args.mode == "e2e" and scans:
        try:
            import hashlib
            scan = scans[-1]
            sc = json.loads(scan.read_text())
            tune = ROOT / "omniparser_amd" / "conv_tuning_gfx950.json"
            cur = {"conv_tuning_sha16": hashlib.sha256(tune.read_bytes()).hexdigest()[:16] if tune.exists() else None,
                   "conv_tuning_applied": os.environ.get("OMNI_CONV_TUNING", "1") != "0",
                   "kernel_sources_sha16": hashlib.sha256(b"".join(p.read_bytes() for p in sorted((ROOT / "omniparser_amd" / "csrc").glob("*.h*")))).hexdigest()[:16]}
            prov = sc.get("provenance") or {}
            if all(prov.get(k) == v for k, v in cur.items()):
                out["config"]["parity_scan"] = {"frames": sc["frames"], "final_boxes_identical": sc["final_boxes_identical"],
                                                "elements_and_crops_identical": sc["elements_and_crops_identical"],
                                                "oracle_tie_free_frames": sc["oracle_tie_free_frames"], "tie_free_and_identical": sc["tie_free_and_identical"],
                                                "held_out": "seeds 8..109 (102 of the 110 frames): the stand-in's calibration batch holds seeds 0..7 and its "
                                                            "threshold is placed on that batch alone", "source": "profiles/" + scan.name,
                                                "measured_at": prov.get("git_rev")}
            else:
                out["config"]["parity_scan"] = {"source": None, "note": f"profiles/{scan.name} was measured with other kernel sources / tuning table "
                                                                        "than this tree: not quoted (re-run tools/scan_gpu_vs_oracle.py device)"}
        except Exception:                                   # noqa: BLE001 — an optional citation
            pass
    if args.frame != "1920x1080" or args.width != 1.0:
        out["config"]["debug"] = {"frame": args.frame, "width": args.width, "note": "NOT the metric's workload (debug / CPU-test sizes)"}
    out["config"]["hbm_peak_allocated_gb"] = round(torch.cuda.max_memory_allocated(dev) / 1e9, 2)   # plans + weights of this process (torch allocator)

    if rank == 0:
        # the timed result above is final: nothing below may keep the JSON line from being printed
        def guarded(name, fn):
            try:
                with torch.inference_mode():
                    out[name] = fn()
                note(f"{name} done")
            except Exception as e:      # noqa: BLE001 — reported in the line itself
                import traceback
                traceback.print_exc(file=sys.stderr)
                out[name] = {"error": f"{type(e).__name__}: {e}"[:400]}
        if args.full:
            dp_obj = dp if args.mode == "detect" else None
            guarded("roofline", lambda: roofline(args, det, parser, dp_obj, crop_counts, B))
        if args.full and world == 1 and not args.no_extra:
            guarded("extra", lambda: extras(args, det, parser, frames, ocr, dev, cap_dir))
        if world == 1 and not args.no_extra and not args.no_ab and args.mode == "e2e" and isinstance(out.get("extra"), dict):
            # this process is done with the GPU: give its activation pools back before the children build their own plans
            try:
                import gc
                parser.cap.clear_plans(); det._plans.clear()
                gc.collect(); torch.cuda.empty_cache()
            except Exception:      # noqa: BLE001
                pass
            # the reference's OWN cuda branch as a labelled line (ref:util/utils.py:120-121: 64x64 crops, do_resize=False, fp16): same
            # pipeline, f16 plans.  Not the parity mode: its parity class is a token-match RATE against the fp32 oracle
            # (tests/test_gpu_b_caption_model.py::test_captioner_f16_token_match_rate_r64), not exactness.  Own process, hard limit.
            out["extra"]["e2e_r64_f16_reference_cuda_branch"] = child_json(
                [sys.executable, os.path.abspath(__file__), "--steps", "5", "--warmup", "2", "--full", "--no-extra", "--no-cpu-baseline",
                 "--caption-res", "64", "--precision", "f16"], {}, 150,
                keep=("value", "ms_per_step", "steps", "dtype", ("config", "workload"), ("config", "mean_crops_per_screenshot"),
                      ("roofline", "gemm_ms_per_step"), ("roofline", "achieved")))
            note("e2e_r64_f16 done")
            out["extra"]["annotate_tail"] = child_json([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools",
                                                                                     "annotate_bench.py")], {}, 120)
            note("annotate_tail done")
            # BASELINE configs[3] stand-in on this one GPU: mixed-resolution eval stream (tools/stream_bench.py), 64x64 crops
            keep = ("metric", "value", "unit", "items", "seconds", "caption_res", "device_batch", "rank0_batches", "mean_elements",
                    "resolution_counts", "data")
            out["extra"]["stream_mixed_resolution_r64"] = child_json(
                [sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools", "stream_bench.py"), "--items", "48",
                 "--caption-res", "64"], {}, 150, keep=keep)
            note("stream_mixed_resolution_r64 done")
            # the same stream at the parity resolution (768x768 crops): the real kernels of configs[3] on one GPU
            out["extra"]["stream_mixed_resolution_r768"] = child_json(
                [sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools", "stream_bench.py"), "--items", "24",
                 "--caption-res", "768"], {}, 240, keep=keep)
            note("stream_mixed_resolution_r768 done")
        if args.full and world == 1 and not args.no_cpu_baseline:
            guarded("cpu_baseline", lambda: cpu_baseline(args, blob, imgsz, out["config"].get("mean_crops_per_screenshot", 0)))
        faulthandler.cancel_dump_traceback_later()
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def load_native():
    """Bind the library build() made.  The benchmark may run in a checkout that was built and then made read-only, and it is also run
    over earlier trees of the project to compare their outputs with --dump-outputs; the loader of those takes the build lock (a file
    opened for writing in the tree) even when nothing is stale.  When that open is refused, a library whose stamp matches the sources
    is bound directly; a stale or missing one is still an error."""
    from omniparser_amd import _lib as L
    try:
        return L.lib()
    except OSError:
        from omniparser_amd import build as BD
        hdrs = list(BD.CSRC.glob("*.h")) + [BD.PKG.parent / "include" / "omni_amd.h"]
        if not BD.LIB.exists() or BD._stale(BD.LIB, BD.sources() + hdrs):
            raise
        import torch  # noqa: F401  (torch's HIP runtime first, as L.lib() does)
        L._lib = L.bind(BD.LIB)
        return L._lib


# run in a child process: the stand-in checkpoint of one kind under argv[2] (a directory named `weights`).  Setting ROOT also serves a
# make_weights.py that predates OMNI_WEIGHTS_DIR (earlier trees of the project: their checkpoints live at <ROOT>/weights/...)
_GENERATE = ("import sys; from pathlib import Path; sys.path.insert(0, sys.argv[1]); import tools.make_weights as M; "
             "M.ROOT = Path(sys.argv[2]).parent; "
             "print(M.ensure_blob(0, 1, float(sys.argv[4])) if sys.argv[3] == 'detector' else M.ensure_caption_checkpoint(0))")


def standin_checkpoints(args, rank, world):
    """(detector blob, caption checkpoint dir) of the seeded stand-ins, generated on first use by rank 0 in child processes.  They live
    in <repo>/weights when that directory already holds them or can be written; in a read-only checkout, in a per-user cache
    ($XDG_CACHE_HOME or ~/.cache, else the temp directory).  Same seeds and committed calibration: the same weights either way.
    OMNI_WEIGHTS_DIR is set to the choice for the child processes of this script."""
    import subprocess
    import tempfile
    import tools.make_weights as MW
    det_rel = Path(*MW.default_path(0, 1, args.width).parts[-3:])        # icon_detect_v3_<tag>/icon_detect_v3/model.pt
    cap_rel = Path(MW.caption_dir(0).name)
    kinds = {"detector": det_rel}
    if args.mode == "e2e":
        kinds["caption"] = cap_rel / "model.safetensors"
    wdir = ROOT / "weights"
    if not (all((wdir / m).exists() for m in kinds.values()) or os.access(wdir if wdir.exists() else ROOT, os.W_OK | os.X_OK)):
        cache = Path(os.environ.get("XDG_CACHE_HOME") or Path.home() / ".cache") / "omniparser_amd" / "weights"
        for wdir in (cache, Path(tempfile.gettempdir()) / f"omniparser_amd-{os.getuid()}" / "weights"):
            try:
                wdir.mkdir(parents=True, exist_ok=True)
            except OSError:
                continue
            if os.access(wdir, os.W_OK | os.X_OK):
                break
        else:
            raise RuntimeError("no writable directory for the stand-in checkpoints")
    os.environ["OMNI_WEIGHTS_DIR"] = str(wdir)
    if rank == 0:
        # one child per missing kind, side by side: seeded initialisation is serial work, so a first run waits for the slower
        # child instead of both; every child has ended before any failure is raised
        procs = {kind: subprocess.Popen([sys.executable, "-c", _GENERATE, str(Path(MW.__file__).resolve().parents[1]), str(wdir), kind,
                                         str(args.width)], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
                 for kind, marker in kinds.items() if not (wdir / marker).exists()}
        errs = {kind: p.communicate()[1] for kind, p in procs.items()}
        for kind, p in procs.items():
            if p.returncode != 0 or not (wdir / kinds[kind]).exists():
                raise RuntimeError(f"stand-in {kind} generation failed in {wdir}:\n{errs[kind][-2000:]}")
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
    return wdir / det_rel, wdir / cap_rel


def pack_records(recs, B, dev, step_id, li, elems, ids):
    """the parsed elements of one step's B screenshots -> rows li*B .. li*B+B-1 of the job's record table (what the all_gather moves):
    boxes in ratio coordinates, caption ids on the rows of the icons that were captioned, in element order.  Same layout as
    `dist.pack_record` (the tests unpack it with `dist.unpack_record`), assembled in ONE host array and ONE upload per step: round 5
    built 8 records with ~50 small torch ops each and uploaded them one by one — 15 ms of host time per step, in the open after the
    last step of a pipelined run (K = 3: 2 % of the line)."""
    import numpy as np
    import torch
    from omniparser_amd import dist as OD
    MD, CT = OD.MAX_DET, OD.CAP_TOK
    host = np.zeros((B, OD.REC_W), dtype=np.int32)
    for j in range(B):
        el = elems[j][:MD]
        k = len(el)
        r = host[j]
        r[0], r[1] = step_id * B + j, k
        if k:
            r[2:2 + 4 * k] = np.asarray([e["bbox"] for e in el], dtype=np.float32).reshape(-1).view(np.int32)
            r[2 + 4 * MD:2 + 4 * MD + k] = np.ones(k, dtype=np.float32).view(np.int32)
        # cls stays 0; caption ids on the rows of the captioned icons
        cap = r[2 + 6 * MD:].reshape(MD, CT)
        ic = [i for i, e in enumerate(elems[j]) if e["source"] == "box_yolo_content_yolo"][:len(ids[j])]
        for row, i in zip(ids[j], ic):
            if i < k:
                v = row.numpy() if hasattr(row, "numpy") else np.asarray(row)
                cap[i, :min(len(v), CT)] = v[:CT]
    recs[li * B:li * B + B].copy_(torch.from_numpy(host), non_blocking=True)


def dump_outputs(d, args, last, dp=None):
    """--dump-outputs: the arrays a caller of the timed path received in the last timed step, one DIR/<name>.npy each, float32 / float64
    only (integers as float, exact below 2**24), padded to MAX_DET rows per screenshot; `count` says how many rows of each are real.
    e2e: the parsed elements of the B screenshots (ratio xyxy boxes, source kind, interactivity, caption ids with -1 padding);
    detect: the detector's kept boxes (pixels), scores and classes.  A few hundred KB at the default sizes."""
    import numpy as np
    from omniparser_amd import dist as OD
    MD, CT, B = OD.MAX_DET, OD.CAP_TOK, args.batch
    d.mkdir(parents=True, exist_ok=True)
    arrs = {}
    if dp is not None:
        cnt = dp.out_count[:B].cpu().numpy()
        real = np.arange(MD)[None, :] < cnt[:, None]           # rows past the count are scratch of the plan: written as 0
        arrs["count"] = cnt.astype(np.float64)
        arrs["boxes"] = np.where(real[..., None], dp.out_boxes[:B].cpu().numpy(), 0).astype(np.float32)
        arrs["scores"] = np.where(real, dp.out_scores[:B].cpu().numpy(), 0).astype(np.float32)
        arrs["cls"] = np.where(real, dp.out_cls[:B].cpu().numpy(), 0).astype(np.float32)
    else:
        elems, ids = last["elems"], last["ids"]
        kinds = {"box_ocr_content_ocr": 0, "box_yolo_content_ocr": 1, "box_yolo_content_yolo": 2}
        count = np.zeros(B, dtype=np.float64)
        boxes = np.zeros((B, MD, 4), dtype=np.float64)
        source = np.full((B, MD), -1.0, dtype=np.float32)
        interactive = np.zeros((B, MD), dtype=np.float32)
        caption_ids = np.full((B, MD, CT), -1.0, dtype=np.float32)
        for j in range(B):
            el = elems[j][:MD]
            count[j] = len(el)
            for i, e in enumerate(el):
                boxes[j, i] = np.asarray(e["bbox"], dtype=np.float64)
                source[j, i] = kinds[e["source"]]
                interactive[j, i] = float(bool(e["interactivity"]))
            # caption ids belong to the captioned icons, in element order (the pairing pack_records uses)
            ic = [i for i, e in enumerate(elems[j]) if e["source"] == "box_yolo_content_yolo"][:len(ids[j])]
            for row, i in zip(ids[j], ic):
                if i < MD:
                    v = np.asarray(row.numpy() if hasattr(row, "numpy") else row).reshape(-1)[:CT]
                    caption_ids[j, i, :len(v)] = v
        arrs.update(count=count, boxes=boxes, source=source, interactive=interactive, caption_ids=caption_ids)
    total = sum(a.nbytes for a in arrs.values())
    assert total <= 64 << 20, f"--dump-outputs: {total} bytes exceeds 64 MB"
    for k, a in arrs.items():
        np.save(d / f"{k}.npy", a)
    return sorted(arrs)


def child_json(cmd, env, limit_s, keep=None):
    """run `cmd` with `env` added, at most `limit_s` seconds, and return the JSON object of its last stdout line (or what went wrong)."""
    import subprocess
    e = dict(os.environ, **env)
    e.pop("OMNI_BENCH_WATCHDOG", None)
    try:
        r = subprocess.run(cmd, env=e, capture_output=True, text=True, timeout=limit_s)
    except subprocess.TimeoutExpired:
        return {"env": env, "error": f"no result within {limit_s} s"}
    lines = [l for l in r.stdout.strip().splitlines() if l.startswith("{")]
    if r.returncode != 0 or not lines:
        return {"env": env, "error": f"exit {r.returncode}: {r.stderr.strip()[-300:]}"}
    try:
        d = json.loads(lines[-1])
    except ValueError as ex:
        return {"env": env, "error": f"unparsable line: {ex}"}
    if keep:
        sel = {}
        for k in keep:
            if isinstance(k, tuple):
                v = d
                for part in k:
                    v = v.get(part) if isinstance(v, dict) else None
                sel[".".join(k)] = v
            else:
                sel[k] = d.get(k)
        d = sel
    d["env"] = env
    return d


GEMM_KINDS = (1, 24)        # OMNI_OP_CONV (conv / linear) and OMNI_OP_MLP_FUSED (fc1 + GELU + fc2 in one kernel): the MFMA-bound family


def gemm_of(by_kind):
    return sum(by_kind.get(k, 0.0) for k in GEMM_KINDS)


KIND_NAMES = {1: "gemm (conv / linear)", 2: "avgpool", 3: "maxpool", 4: "resize_nearest", 5: "letterbox", 6: "detect_decode", 7: "nms",
              8: "dwconv3", 9: "layernorm", 10: "attention (window / mha)", 11: "channel_attention", 12: "proj_prep", 13: "assemble",
              14: "embed_step", 15: "attn_decode", 16: "greedy_step", 17: "crop_resize", 18: "dwconv3+ln", 19: "split_convert", 20: "hand-off",
              21: "overlay", 22: "png_pack", 23: "png_deflate", 24: "mlp_fused (fc1+GELU+fc2, GEMM family)"}


def profile_plan(plan, stream, repeat=1, per_kernel=None, times=1.0, work_scale=1.0):
    """per-op-kind device ms of `repeat` eager replays (HIP events around every op, in sequence: omni_plan_profile).  `per_kernel`
    (dict) collects launches / ms / algorithmic FLOPs and bytes per (kernel, shape), weighted by `times` (how often the step runs this
    plan); `work_scale` = real rows / plan capacity (bucket padding is wasted time, not work)."""
    from omniparser_amd.opwork import op_kernel, op_shape, op_work
    by_kind, n_gemm = {}, 0
    for _ in range(repeat):
        ms = plan.profile(stream)
        for op, t in zip(plan.ops, ms):
            by_kind[op.kind] = by_kind.get(op.kind, 0.0) + t
            if per_kernel is not None:
                f, b = op_work(op)
                a = per_kernel.setdefault((op_kernel(op), op_shape(op), op.kind), [0.0, 0.0, 0.0, 0.0])
                a[0] += times; a[1] += t * times; a[2] += f * times * work_scale; a[3] += b * times * work_scale
        n_gemm += sum(1 for op in plan.ops if op.kind in GEMM_KINDS)
    return by_kind, n_gemm


def per_kernel_rows(per_kernel, top=8):
    """the step's `top` most expensive (kernel, shape) groups: launches, ms per step, achieved rate on ALGORITHMIC work and its
    fraction of the roof that bounds it (dense f16 MFMA 2500 TF/s for the GEMM / attention kernels, HBM 8 TB/s otherwise)."""
    from omniparser_amd.opwork import MFMA_KINDS
    rows = []
    for (name, shape, kind), (n, ms, f, b) in sorted(per_kernel.items(), key=lambda kv: -kv[1][1])[:top]:
        r = {"kernel": name, "shape_rows_n_k": list(shape), "launches": int(round(n)), "ms": round(ms, 3)}
        if kind in MFMA_KINDS and f > 0:
            tf = f / (ms * 1e-3) / 1e12
            r.update(bound="mfma", achieved=round(tf, 1), unit="TFLOP/s", frac=round(tf / 2500.0, 4))
        else:
            tb = b / (ms * 1e-3) / 1e12
            r.update(bound="hbm", achieved=round(tb, 3), unit="TB/s", frac=round(tb / 8.0, 4))
        rows.append(r)
    return rows


def roofline(args, det, parser, dp, crop_counts, B):
    """Dominant kernel family = the GEMMs (conv / linear).  `achieved` = ALGORITHMIC GEMM FLOPs of one step (real crop count,
    not the bucket-padded one) / device time of exactly those launches, each timed in its real sequence by HIP events during
    an instrumented eager replay of the step's plans right after the timed region (same inputs, same buffers; every other
    kernel of the step runs in between, so caches are in the state the timed steps leave them).  The same replay yields the
    per-kernel-family split of a step; `rocprofv3 --kernel-trace --stats` of this command is committed under profiles/."""
    from omniparser_amd import _lib as L
    fam, parts, pk = {}, {}, {}
    gemm_ms = 0.0
    launches = 0

    def add(by_kind, times=1.0):
        for k, t in by_kind.items():
            fam[k] = fam.get(k, 0.0) + t * times

    if args.mode == "detect":
        bk, n = profile_plan(dp.plan, det.stream, per_kernel=pk)
        add(bk)
        flops, gemm_ms, launches = dp.net_flops, bk.get(1, 0.0), n
        parts["detector_batch%d" % B] = {"gemm_ms": round(gemm_ms, 4), "gflop": round(dp.net_flops / 1e9, 2)}
        crops = 0
    else:
        cap = parser.cap
        ddp = next(p for p in det._plans.values() if p.batch == B)
        bk, n = profile_plan(ddp.plan, det.stream, per_kernel=pk)
        add(bk)
        flops, gemm_ms, launches = float(ddp.net_flops), bk.get(1, 0.0), n
        parts["detector_batch%d" % B] = {"gemm_ms": round(bk.get(1, 0.0), 4), "gflop": round(ddp.net_flops / 1e9, 2)}
        crops = int(round(sum(crop_counts) / max(len(crop_counts), 1)))
        merged = crops > 128 and os.environ.get("OMNI_MERGED_DECODE", "1") != "0"      # one decode over all crops (florence.py::_DecodePlans)
        exact = merged and cap.exact_rows and crops % 128       # the remainder micro-batch: an exact-row graph in a 128-row plan's buffers
        mbs = [128] * (crops // 128) + ([crops % 128 if exact else cap.bucket(crops % 128)] if crops % 128 else [])
        per_crop = 0.0
        import torch
        for bucket in sorted(set(mbs)):
            cp = cap._plans.get((bucket, cap.resolution, 20))
            if cp is None and exact and bucket == crops % 128:
                owners = [p for k, p in cap._plans.items() if k[0] == 128 and k[1] == cap.resolution and bucket in getattr(p, "_row_plans", {})]
                cp = owners[0]._row_plans[bucket] if owners else None
                if cp is None:          # no exact twin (yet): the remainder ran the twin of the next ladder capacity, or the full plan
                    b2 = cap.bucket(bucket)
                    owners = [p for k, p in cap._plans.items() if k[0] == 128 and k[1] == cap.resolution and b2 in getattr(p, "_row_plans", {})]
                    if not owners:
                        mbs[-1] = 128   # counted with the full micro-batches below (their real rows include the remainder's)
                        continue
                    cp = owners[0]._row_plans[b2]
                    mbs[-1] = bucket = b2
            if cp is None:
                continue
            cnt = mbs.count(bucket)
            if cp.arena is None:
                with torch.inference_mode(), torch_stream(cap.stream):
                    cp.reset()
            real_rows = sum(min(128, crops - 128 * j) for j, mb in enumerate(mbs) if mb == bucket)
            be, ne = profile_plan(cp.encode_plan, cap.stream, per_kernel=pk, times=cnt, work_scale=real_rows / float(cnt * bucket))
            add(be, cnt)
            gemm_ms += cnt * gemm_of(be)
            launches += cnt * ne
            part = {"encode_gemm_ms": round(gemm_of(be), 3), "encode_gflop_per_crop": round(cp.encode_flops / cp.B / 1e9, 2),
                    "encode_gemm_bytes_per_crop": int(cp.pb.bytes / cp.B)}
            if cp.arena is None:
                part["step_gflop_per_crop"] = round(cp.step_flops / cp.B / 1e9, 4)
                step_flops_per_crop = cp.step_flops / cp.B
            else:
                part["exact_rows_in_plan_of"] = cp.arena.B
            if not merged:
                bs, ns = profile_plan(cp.step_plan, cap.stream, repeat=20, per_kernel=pk, times=cnt, work_scale=real_rows / float(cnt * bucket))
                add(bs, cnt)
                gemm_ms += cnt * bs.get(1, 0.0)
                launches += cnt * ns
                part["decode20_gemm_ms"] = round(bs.get(1, 0.0), 3)
            parts["caption_mb%d_x%d" % (bucket, cnt)] = part
            if cp.arena is None:
                per_crop = cp.encode_flops / cp.B + 20 * cp.step_flops / cp.B
        if merged:
            dec = cap._plans.get(("dec", cap.decode_bucket(crops), cap.resolution, 20))
            if dec is not None:
                with torch.inference_mode(), torch_stream(cap.stream):
                    dec.reset()
                bs, ns = profile_plan(dec.step_plan, cap.stream, repeat=20, per_kernel=pk, work_scale=crops / float(dec.B))
                add(bs)
                gemm_ms += bs.get(1, 0.0)
                launches += ns
                parts["decode_rows%d" % dec.B] = {"decode20_gemm_ms": round(bs.get(1, 0.0), 3), "decode20_all_ms": round(sum(bs.values()), 3)}
        flops += crops * per_crop          # ALGORITHMIC: real crops (bucket padding is wasted time, not work)
    achieved = flops / (gemm_ms * 1e-3) / 1e12
    split = args.precision == "f32" and os.environ.get("OMNI_CONV_SPLIT", "1") == "1"
    peak = 2500.0 if (split or args.precision == "f16") else 157.3
    total = sum(fam.values())
    out = {"bound": "mfma",
           "kernel": ("gemm_dma_kernel (pre-split LDS-DMA GEMM, split-f16 x3 MFMA, f32 accumulate) + mlp_fused_kernel (DaViT stage-0 FFN) + conv_split_kernel (convs, decoder steps)"
                      if split else "conv_igemm_kernel<T,BM,BN,RB,ALIGNED,PW>") + " + splitk_reduce_kernel",
           "achieved": round(achieved, 3), "peak": peak, "unit": "TFLOP/s", "frac": round(achieved / peak, 4), "traffic": None}
    if split:
        # every algorithmic MAC issues 3 f16 MFMA products (hi*hi + hi*lo + lo*hi): the matrix pipe is busy 3 * achieved / peak
        out.update(mfma_products_per_mac=3, matrix_pipe_utilisation=round(3 * achieved / peak, 4), vs_f32_mfma_peak=round(achieved / 157.3, 3))
    tfile = next((f for f in (ROOT / "profiles" / "r6_pmc_traffic.json", ROOT / "profiles" / "r5_pmc_traffic.json", ROOT / "profiles" / "r4_pmc_traffic.json",
                              ROOT / "profiles" / "r3_pmc_traffic.json")
                  if f.exists()), None)
    if split and args.mode == "e2e" and args.caption_res == 768 and tfile is not None:
        t = json.loads(tfile.read_text())
        out["traffic"] = t.get("gemm_bytes_per_launch")
        out["traffic_source"] = f"profiles/{tfile.name}: PMC passes of a separate rocprofv3 session over the same kernels (not of this run)"
        out["traffic_detail"] = {k: t[k] for k in ("gemm_fetch_bytes_per_crop", "gemm_write_bytes_per_crop", "algorithmic_gemm_bytes_per_crop",
                                                   "ratio", "source") if k in t}
    out.update({
        "flops_per_step": flops, "crops_per_step": crops, "gemm_launches_per_step": launches, "gemm_ms_per_step": round(gemm_ms, 3),
        "avg_gemm_launch_us": round(1000 * gemm_ms / max(launches, 1), 3), "profiled_step_ms": round(total, 3),
        "non_gemm_share": round(1.0 - gemm_ms / max(total, 1e-9), 4),
        "kernel_family_ms_per_step": {KIND_NAMES.get(k, str(k)): round(v, 3) for k, v in sorted(fam.items(), key=lambda kv: -kv[1])},
        "parts": parts,
        # the step's most expensive (kernel, shape) groups with their OWN roofline fraction (the family figure above averages over them)
        "per_kernel": per_kernel_rows(pk),
        "method": "HIP events around every op of an eager replay of the step's plans (omni_plan_profile), after the timed region"})
    return out


def torch_stream(stream):
    import torch
    return torch.cuda.stream(stream)


def extras(args, det, parser, frames, ocr, dev, cap_dir):
    """BASELINE configs[1], the 64x64 (reference cuda-branch) crop size, configs[4] — small runs beside the headline line.
    `value` of the JSON line stays configs[2] at 768x768."""
    import torch
    from omniparser_amd.florence import Florence2Captioner
    from omniparser_amd.pipeline import ScreenParser
    from omniparser_amd.synth import synthetic_ocr, synthetic_screenshot
    ex = {}

    def time_region(fn, iters, warm=1):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) / iters

    # configs[1]: detector only (letterbox + network + decode + NMS, HBM-resident input), batch 1 / 8, both network sizes
    for tag, imgsz, batch, iters in (("detector_b1_640", 640, 1, 100), ("detector_b8_640", 640, 8, 20), ("detector_b1_1088x1920", (IH, IW), 1, 30)):
        dp = det.get_plan(IW, IH, imgsz, CONF, NMS_IOU, MAX_DET, batch=batch)
        with torch.cuda.stream(det.stream):
            for j in range(batch):
                dp.img[j].copy_(frames[j % 8])
        det.stream.synchronize()

        def run(dp=dp):
            dp.launch(det)
            det.stream.synchronize()
        sec = time_region(run, iters, warm=2)
        bk, n = profile_plan(dp.plan, det.stream)
        g = bk.get(1, 1e-9)
        ex[tag] = {"value": round(batch / sec, 2), "unit": "screenshots/s", "ms_per_step": round(1000 * sec, 3),
                   "workload": "BASELINE configs[1]: detector only, batch %d, network input %s" % (batch, "640x640" if imgsz == 640 else "1088x1920"),
                   "roofline": {"bound": "mfma", "achieved": round(dp.net_flops / g / 1e9, 2), "peak": 2500.0, "unit": "TFLOP/s",
                                "frac": round(dp.net_flops / g / 1e9 / 2500.0, 4), "gemm_ms": round(g, 3),
                                "gflop": round(dp.net_flops / 1e9, 1), "non_gemm_ms": round(sum(bk.values()) - g, 3)}}
    if args.mode != "e2e":
        return ex
    # the boundary (get_som_labeled_img / parse) hands over HOST images: the same pipelined stream with every batch's 8 frames uploaded
    # from pinned host memory inside the timed loop (8 x 6.2 MB per step) — the PCIe-inclusive rate; it is never `value`
    host = [f.cpu().pin_memory() for f in frames]

    def h2d_batches(n):
        for k in range(n):
            with torch.cuda.stream(det.stream):      # the detector's stream reads the frames first; every later reader is ordered behind it
                up = [host[j].to(dev, non_blocking=True) for j in range(8)]
            yield up, list(ocr)
    with torch.inference_mode():
        for _ in parser.parse_stream(h2d_batches(2)):
            pass
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in parser.parse_stream(h2d_batches(3)):
            pass
        torch.cuda.synchronize(dev)
    sec = (time.perf_counter() - t0) / 3
    ex["e2e_pcie_inclusive"] = {"value": round(8 / sec, 3), "unit": "screenshots/s", "ms_per_step": round(1000 * sec, 2), "steps": 3,
                                "workload": "configs[2] as timed above, plus the upload of every step's 8 frames from pinned host memory "
                                            "(49.8 MB per step) inside the loop"}
    del host
    # the reference's cuda branch feeds 64x64 crops (ref:util/utils.py:120-121): same pipeline at that crop size
    cap64 = Florence2Captioner(cap_dir, dev, precision=args.precision, resolution=64)
    p64 = ScreenParser(det, cap64, box_threshold=CONF, iou_threshold=OVERLAP_IOU, nms_iou=NMS_IOU, max_det=MAX_DET, imgsz=640)
    sec = time_region(lambda: p64.parse_batch(frames, ocr), 3)
    ex["e2e_r64_batch8"] = {"value": round(8 / sec, 2), "unit": "screenshots/s", "ms_per_step": round(1000 * sec, 2),
                            "workload": "configs[2] pipeline with 64x64 crops (the reference's cuda-branch crop size), batch 8"}
    del p64, cap64
    torch.cuda.empty_cache()
    # configs[4]: 3840x2160 frames, 2x2 overlapping tiles + global NMS (policy is ours), 64-crop caption micro-batches at 768x768
    ptile = ScreenParser(det, parser.cap, box_threshold=CONF, iou_threshold=OVERLAP_IOU, nms_iou=NMS_IOU, max_det=MAX_DET, imgsz=640,
                         batch_size=64, tile_large=True)
    f4k = [torch.from_numpy(synthetic_screenshot(100 + s, 3840, 2160)).to(dev) for s in range(2)]
    o4k = [synthetic_ocr(100 + s, 3840, 2160, 40) for s in range(2)]
    ptile.parse_batch(f4k, o4k)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    ptile.parse_batch(f4k, o4k)
    torch.cuda.synchronize(dev)
    sec = time.perf_counter() - t0
    ex["tiled_4k_r768"] = {"value": round(2 / sec, 3), "unit": "screenshots/s", "ms_per_step": round(1000 * sec, 1),
                           "workload": "BASELINE configs[4] on one GPU: 2 frames of 3840x2160, 2x2 tiles of 1952x1112 (64 px overlap) -> global NMS, "
                                       "64-crop caption micro-batches at 768x768",
                           "crops_per_frame": ptile.stats["crops"], "boxes_per_frame": ptile.stats["boxes"]}
    return ex


def cpu_baseline(args, blob, imgsz, mean_crops):
    """Reference-equivalent CPU path on the host cores (oracle/: torch.jit blob + PIL letterbox + restated
    batched_nms; transformers Florence-2 fp32 on 768x768 crops), bounded sample."""
    import numpy as np
    import torch
    from PIL import Image
    from oracle import detector_ref as D
    from omniparser_amd.synth import synthetic_screenshot
    model = torch.jit.load(str(blob), map_location="cpu").eval()
    imgs = [Image.fromarray(synthetic_screenshot(s)) for s in range(2)]
    D.predict(model, imgs[0], conf=CONF, imgsz=imgsz, iou=NMS_IOU, max_det=MAX_DET)
    t0 = time.perf_counter()
    for im in imgs:
        D.predict(model, im, conf=CONF, imgsz=imgsz, iou=NMS_IOU, max_det=MAX_DET)
    t_det = (time.perf_counter() - t0) / len(imgs)
    res = {"unit": "screenshots/s", "cores": torch.get_num_threads(), "kind": "port"}
    if args.mode == "detect":
        res.update(value=round(1.0 / t_det, 4), sample="2 screenshots, detector stage (PIL letterbox + TorchScript YOLOv9-E fp32 + decode + "
                   "batched_nms), 1 warm-up")
        return res
    from oracle import preprocess_ref as PR
    from omniparser_amd.florence import CLIP_MEAN, CLIP_STD, PROMPT_IDS
    from tools.make_weights import build_random_captioner
    cap = build_random_captioner(0)
    R = args.caption_res
    # ONE WHOLE SCREENSHOT, measured: detector pass + every caption crop of the frame (the mean crop count of the timed steps, crop
    # rectangles = the oracle detector's first boxes on that frame) through crop / cv2-bilinear 64x64 / bicubic RxR / Florence-2
    # `generate` in ONE batch — how the reference runs it (ref:util/utils.py:101-125: batch_size 128, all crops of an image at once).
    # `value` is 1 / that measured time; nothing is composed from per-crop figures (rounds 1-4 quoted t_det + crops x t_crop from an
    # 8-crop batch, which over-stated the CPU's cost per crop by ~1.6x against a whole measured pass).
    n = max(1, int(round(mean_crops))) if not os.environ.get("OMNI_CPU_BASELINE_CROPS") else int(os.environ["OMNI_CPU_BASELINE_CROPS"])
    img = synthetic_screenshot(0)
    t0 = time.perf_counter()
    res0 = D.predict(model, Image.fromarray(img), conf=CONF, imgsz=imgsz, iou=NMS_IOU, max_det=MAX_DET)
    t_det1 = time.perf_counter() - t0
    bx = np.asarray(res0[0], dtype=np.float64).reshape(-1, 4)
    boxes = []
    for b in bx:                                             # integer rectangles inside the frame with a positive area (the hand-off drops the rest)
        x0, y0, x1, y1 = max(int(b[0]), 0), max(int(b[1]), 0), min(int(b[2]), IW), min(int(b[3]), IH)
        if x1 - x0 >= 2 and y1 - y0 >= 2 and len(boxes) < n:
            boxes.append((x0, y0, x1, y1))
    rng = np.random.default_rng(0)
    while len(boxes) < n:                                    # a frame with fewer detections than the mean: fill with icon-sized rectangles
        x, y = int(rng.integers(0, IW - 64)), int(rng.integers(0, IH - 64))
        boxes.append((x, y, x + 60, y + 48))
    t1 = time.perf_counter()
    pv = np.stack([PR.caption_pixel_values(img, b, R, CLIP_MEAN, CLIP_STD) for b in boxes])
    pix = torch.from_numpy(pv).permute(0, 3, 1, 2).contiguous()
    ids = torch.tensor([[cap.config.image_token_id] * ((R // 32) ** 2 + 1) + PROMPT_IDS] * n)
    with torch.inference_mode():
        cap.generate(input_ids=ids, pixel_values=pix, max_new_tokens=20, num_beams=1, do_sample=False)
    t_cap = time.perf_counter() - t1
    whole = t_det1 + t_cap
    c0 = next((f for f in (ROOT / "profiles" / "r5_s3_configs0.json", ROOT / "profiles" / "r4_s4_configs0.json") if f.exists()), ROOT / "profiles" / "r5_s3_configs0.json")
    if c0.exists():
        # BASELINE configs[0] measured WHOLE in a separate session (tools/configs0.py: the reference's demo_image.jpg, ONE full CPU pass of
        # every crop at 768x768 vs Omniparser.parse on the MI355X) — quoted from the committed record, not measured by this run
        try:
            d0 = json.loads(c0.read_text())
            res["configs0_measured_separately"] = {"cpu_seconds_per_image": d0["cpu_reference_equivalent"]["seconds_per_image"],
                                                   "mi355x_seconds_per_image": d0["mi355x"]["seconds_per_image"], "image": d0["image"],
                                                   "size": d0["size"], "captions_identical": d0["agreement"]["captions_identical"],
                                                   "source": "profiles/" + c0.name}
        except Exception:                                   # noqa: BLE001 — an optional citation
            pass
    res.update(value=round(1.0 / whole, 5), seconds_per_screenshot=round(whole, 2),
               sample=f"ONE whole 1920x1080 screenshot, measured (not composed): detector pass {t_det1:.2f} s (warm: {t_det:.2f} s) + crop / resize / "
                      f"Florence-2 generate over all {n} crops of the frame at {R}x{R} in one batch {t_cap:.1f} s ({t_cap / n:.2f} s per crop); "
                      "hand-off glue (milliseconds) excluded")
    return res


if __name__ == "__main__":
    main()

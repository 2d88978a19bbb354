"""What the built-in OCR costs on the device, in ONE process.
(a) OMNI_OP_REGION_OCR mode 0 alone: 6 tiles of 768 x 768 cut from a 1920x1080 frame (the grid of `read_regions` at overlap 128) and
    128 tiles of 64 x 64, f32 and f16 plan inputs; HIP events around the op of an eager replay (omni_plan_profile), median (min) of
    10 after a warm-up replay, and the HBM rate the algorithmic bytes of opwork.op_work imply.
(b) mode 1 alone: 6 and 128 rows of T = 1025 tokens, every region slot used (113 regions per row) and no region at all.
(c) `util.utils.read_text_regions` on a synthetic 1920x1080 frame at R = 768, f32 plans, stand-in checkpoint with the synthetic
    tokenizer + location tokens, generation restricted to the location tokens and 40 text tokens so that the answer has regions:
    wall time of a synchronised call at 64 and at 256 new tokens per tile, median (min) of 3 after a warm-up call.
usage: python tools/region_ocr_bench.py [out.txt]   -> a table on stdout (and into out.txt)"""
import statistics
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def profile(L, op, reps=10):
    import torch
    plan = L.Plan([op])
    s = torch.cuda.Stream()
    ts = []
    with torch.cuda.stream(s):
        plan.run(s)
        s.synchronize()
        for _ in range(reps):
            ts.append(plan.profile(s)[0])
    s.synchronize()
    return ts


def bench_cut(lines):
    import numpy as np
    import torch
    from omniparser_amd import _lib as L
    from omniparser_amd import opwork
    from omniparser_amd.florence import tile_cut_op
    from omniparser_amd.pipeline import ScreenParser
    from omniparser_amd.synth import synthetic_screenshot
    frame = torch.from_numpy(synthetic_screenshot(5)).cuda()
    H, W = frame.shape[:2]
    lut = torch.from_numpy((np.arange(256).astype(np.float64) * (1 / 255)).astype(np.float32)).cuda()
    lines.append("(a) mode 0, tiles cut from a 1920x1080 frame; microseconds median (min) of 10; GB/s = algorithmic bytes / median")
    for R, origins in ((768, ScreenParser.tile_origins(W, H, 768, 768, 128)[0]), (64, [(13 * k, 7 * k) for k in range(128)])):
        org = torch.tensor(origins, dtype=torch.int32).cuda()
        for name, dt, tdt, ldo in (("f32", L.F32, torch.float32, 4), ("f16", L.F16, torch.float16, 8)):
            y = torch.empty((len(origins), R, R, ldo), dtype=tdt, device="cuda")
            op = tile_cut_op(dt, frame.data_ptr(), org.data_ptr(), y.data_ptr(), lut.data_ptr(), len(origins), H, W, R, ldo)
            ts = profile(L, op)
            nb = opwork.op_work(op, y.element_size())[1]
            med = statistics.median(ts)
            lines.append(f"  {len(origins):>3} tiles of {R:>3}x{R:<3} {name} (pitch {ldo}){1e3 * med:10.1f} ({1e3 * min(ts):.1f}) us   {nb / 1e6:8.2f} MB -> {nb / (med * 1e-3) / 1e9:7.1f} GB/s")


def bench_parse(lines):
    import numpy as np
    import torch
    import region_checks as RC
    from omniparser_amd import _lib as L
    from omniparser_amd.florence import ocr_slots, region_parse_op
    T, R = 1025, 768
    M = ocr_slots(T)
    table = np.full((51289,), RC.TEXT, np.uint16)
    table[:3] = RC.STRIP
    table[RC.LOC0:RC.LOC0 + 1000] = np.arange(1000)
    tab = torch.from_numpy(table.astype(np.int16)).cuda()
    lines += ["", f"(b) mode 1, rows of T = {T} tokens with log-probabilities; microseconds median (min) of 10"]
    full = [RC.START] + ([RC.A] + RC.QUAD_A) * M + RC.QUAD_B[:(T - 1) % 9]
    none = [RC.START] + [RC.A] * (T - 2) + [RC.EOS]
    for n in (6, 128):
        for name, row in (("113 regions per row", full), ("no region", none)):
            ids = torch.tensor([row] * n, dtype=torch.int32).cuda()
            logp = -torch.rand((n, T - 1)).cuda()
            cells = torch.tensor([[0, 0, -2 ** 31, 2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1]] * n, dtype=torch.int32).cuda()
            rec = torch.empty((n, M, 16), dtype=torch.int32, device="cuda")
            sums, rows = torch.empty((n, M), device="cuda"), torch.empty((n, 4), dtype=torch.int32, device="cuda")
            ts = profile(L, region_parse_op(ids.data_ptr(), tab.data_ptr(), logp.data_ptr(), cells.data_ptr(), rec.data_ptr(), sums.data_ptr(),
                                            rows.data_ptr(), n, T, tab.numel(), R, RC.EOS))
            assert rows[:, 0].tolist() == [M if row is full else 0] * n
            lines.append(f"  {n:>3} rows, {name:<20}{1e3 * statistics.median(ts):10.1f} ({1e3 * min(ts):.1f}) us")


def bench_call(lines):
    import torch
    import region_checks as RC
    from omniparser_amd.florence import Florence2Captioner
    from omniparser_amd.synth import synthetic_screenshot
    from omniparser_amd.util import utils as U
    tmp = tempfile.mkdtemp()
    ckpt = RC.caption_dir_with_tokenizer(tmp)
    cap = Florence2Captioner(ckpt, "cuda", precision="f32", resolution=768)
    proc = U.FlorenceProcessor(ckpt, image_token_id=cap.w.cfg.get("image_token_id", 51289), special_ids=(cap.w.bos, cap.w.pad, cap.w.eos, 3))
    cmp_ = {"model": cap, "processor": proc}
    frame = synthetic_screenshot(5)
    gen = {"suppress_tokens": RC.ocr_suppress(cap.w.vocab, keep=(RC.BOS, RC.EOS))}
    lines += ["", "(c) read_text_regions, 1920x1080 frame, R = 768 (6 tiles, overlap 128), f32 plans; ms per synchronised call, median (min) of 3"]
    for max_new in (64, 256):
        fn = lambda: U.read_text_regions(frame, cmp_, max_new_tokens=max_new, generation=gen, return_stats=True)
        regions, stats = fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(1e3 * (time.perf_counter() - t0))
        lines.append(f"  max_new_tokens = {max_new:>4}: {statistics.median(ts):9.1f} ({min(ts):.1f}) ms   {cap.last_steps} steps, "
                     f"{sum(s['found'] for s in stats)} regions found, {len(regions)} returned")


def main():
    lines = []
    bench_cut(lines)
    bench_parse(lines)
    bench_call(lines)
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 1:
        Path(sys.argv[1]).parent.mkdir(parents=True, exist_ok=True)
        Path(sys.argv[1]).write_text(text + "\n")


if __name__ == "__main__":
    main()

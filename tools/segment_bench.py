"""What segmentation costs on the device, in ONE process.
(a) OMNI_OP_REGION_OCR mode 5 alone: 8 rows of T = 65 tokens holding one polygon of 32 vertices (what the stand-in checkpoint answers)
    and two <poly> instances of two polygons each; then mode 6 alone on mode 5's outputs for those rows, 4 instance slots, R = 768,
    a 1920x1080 frame.  HIP events around the op of an eager replay (omni_plan_profile), median (min) of 10 after a warm-up replay.
(b) `util.utils.segment` for 8 regions of a synthetic 1920x1080 frame at R = 768 against `util.utils.describe_regions` for the same
    boxes at the same max_new_tokens (64), f32 plans, stand-in checkpoint with the synthetic tokenizer + location and polygon tokens,
    generation restricted to the location tokens, <sep>, <poly>, </poly> and EOS in both: HIP events on the captioner's stream around
    the call (and the wall time of the synchronised call), median (min) of 5 after a warm-up call.  The events bracket the whole
    call, host work included; `Florence2Captioner.segment_regions` with the rows `segment` hands it is timed the same way, so that
    segment - segment_regions is what `segment` does on the host behind the read-back.  The share of the two launches is an ESTIMATE:
    the times of (a), a separate run on synthetic rows, over the time of the call.
usage: python tools/segment_bench.py [out.txt]   -> a table on stdout (and into out.txt)"""
import statistics
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from tools.region_ocr_bench import profile      # noqa: E402

N, T, I, R = 8, 65, 4, 768


def bench_ops(lines):
    import numpy as np
    import torch
    import poly_checks as PC
    import region_checks as RC
    from omniparser_amd import _lib as L
    from omniparser_amd.florence import poly_mask_op, poly_parse_op, poly_slots
    P, V = poly_slots(T)
    table = np.full((51289,), RC.TEXT, np.uint16)
    table[:3] = RC.STRIP
    table[RC.LOC0:RC.LOC0 + 1000] = np.arange(1000)
    table[[PC.SEP, PC.POLY, PC.PEND]] = [PC.C_SEP, PC.C_POLY, PC.C_PEND]
    tab = torch.from_numpy(table.astype(np.int16)).cuda()
    rng = np.random.default_rng(0)
    ring = lambda k, cx, cy, rad: [v for q in range(k) for v in (int(cx + rad * np.cos(6.2832 * q / k)), int(cy + rad * np.sin(6.2832 * q / k)))]   # noqa: E731
    one = [RC.START] + RC.loc(*ring(32, 500, 500, 400))
    inst = lambda cx, cy: [PC.POLY] + RC.loc(*ring(6, cx, cy, 200)) + [PC.SEP] + RC.loc(*ring(5, cx, cy, 100)) + [PC.PEND]                            # noqa: E731
    two = ([RC.START] + inst(300, 300) + inst(700, 600) + [RC.EOS] + [RC.PAD] * T)[:T]
    lines.append(f"(a) modes 5 and 6 alone, {N} rows of T = {T} tokens, {I} instance slots, R = {R}, 1920x1080 frame; microseconds median (min) of 10")
    out = {}
    for name, row in (("one polygon of 32 vertices", one), ("2 instances x 2 polygons", two)):
        ids = torch.tensor([row] * N, dtype=torch.int32).cuda()
        logp = -torch.from_numpy(rng.random((N, T - 1), dtype=np.float32)).cuda()
        cells = torch.tensor([[100 * r, 40 * r, -2 ** 31, 2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1] for r in range(N)], dtype=torch.int32).cuda()
        verts = torch.empty((N, V, 2), dtype=torch.int32, device="cuda")
        rec = torch.empty((N, P, 16), dtype=torch.int32, device="cuda")
        sums, rows = torch.empty((N, P), device="cuda"), torch.empty((N, 4), dtype=torch.int32, device="cuda")
        mask = torch.empty((N, I, R, (R + 31) // 32), dtype=torch.int32, device="cuda")
        cnt = torch.empty((N, I, R), dtype=torch.int32, device="cuda")
        t5 = profile(L, poly_parse_op(ids.data_ptr(), tab.data_ptr(), logp.data_ptr(), cells.data_ptr(), verts.data_ptr(), rec.data_ptr(), sums.data_ptr(),
                                      rows.data_ptr(), N, T, tab.numel(), R, RC.EOS))
        t6 = profile(L, poly_mask_op(rec.data_ptr(), rows.data_ptr(), verts.data_ptr(), cells.data_ptr(), mask.data_ptr(), cnt.data_ptr(), N, T, I, 1080, 1920, R))
        assert rows[:, 1].tolist() == [1 if row is one else 2] * N and int(cnt.sum()) > 0
        out[name] = (statistics.median(t5), statistics.median(t6))
        lines.append(f"  {name:<28} mode 5 {1e3 * out[name][0]:8.1f} ({1e3 * min(t5):.1f}) us   mode 6 {1e3 * out[name][1]:8.1f} ({1e3 * min(t6):.1f}) us   "
                     f"{int(cnt.sum())} pixels set")
    return out


def bench_calls(lines, ops):
    import torch
    import poly_checks as PC
    import region_checks as RC
    from omniparser_amd.florence import Florence2Captioner
    from omniparser_amd.synth import synthetic_screenshot
    from omniparser_amd.util import utils as U
    ckpt = PC.caption_dir_with_poly_tokenizer(tempfile.mkdtemp())
    cap = Florence2Captioner(ckpt, "cuda", precision="f32", resolution=R)
    proc = U.FlorenceProcessor(ckpt, image_token_id=cap.w.cfg.get("image_token_id", 51289), special_ids=(cap.w.bos, cap.w.pad, cap.w.eos, 3))
    cmp_ = {"model": cap, "processor": proc}
    frame = synthetic_screenshot(5)
    boxes = [[100 + 220 * k, 80 + 110 * k, 260 + 220 * k, 200 + 110 * k] for k in range(N)]
    gen = {"suppress_tokens": PC.poly_suppress(cap.w.vocab, keep=(RC.BOS, RC.EOS))}
    max_new = T - 1
    lines += ["", f"(b) {N} regions of a 1920x1080 frame, R = {R}, {max_new} new tokens, f32 plans; ms per call on the captioner's stream "
                  "(HIP events; wall time of the synchronised call beside it), median (min) of 5"]
    res, seen = {}, []
    real = cap.segment_regions

    def spy(image_u8, origins, prompts, class_table, **kw):
        seen[:] = [(image_u8, origins, prompts, class_table, kw)]
        return real(image_u8, origins, prompts, class_table, **kw)
    cap.segment_regions = spy
    U.segment(frame, cmp_, regions=boxes, max_new_tokens=max_new, instances=I, generation=gen)
    del cap.segment_regions
    img, origins, prompts, table, skw = seen[0]
    for name, fn in (("describe_regions", lambda: U.describe_regions(frame, boxes, cmp_, task="<REGION_TO_DESCRIPTION>", max_new_tokens=max_new, generation=gen)),
                     ("segment_regions", lambda: real(img, origins, prompts, table, **skw)),
                     ("segment", lambda: U.segment(frame, cmp_, regions=boxes, max_new_tokens=max_new, instances=I, generation=gen))):
        got = fn()
        torch.cuda.synchronize()
        ev, wall = [], []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(cap.stream)
            t0 = time.perf_counter()
            fn()
            b.record(cap.stream)
            torch.cuda.synchronize()
            wall.append(1e3 * (time.perf_counter() - t0))
            ev.append(a.elapsed_time(b))
        res[name] = statistics.median(ev)
        extra = (f"{len(got)} instances, {sum(g['area'] for g in got)} pixels set" if name == "segment" else
                 f"{len(got)} texts" if name == "describe_regions" else f"{int(got.rows[:, 3].sum())} instances kept")
        lines.append(f"  {name:<18}{statistics.median(ev):9.2f} ({min(ev):.2f}) ms   wall {statistics.median(wall):9.2f} ({min(wall):.2f}) ms   {cap.last_steps} steps, {extra}")
    t5, t6 = ops["one polygon of 32 vertices"]
    lines.append(f"  segment - describe_regions = {res['segment'] - res['describe_regions']:.2f} ms, of which segment - segment_regions = "
                 f"{res['segment'] - res['segment_regions']:.2f} ms is host work behind the read-back")
    lines.append(f"  estimate from the separate run (a): a mode-5 + a mode-6 launch, {1e3 * (t5 + t6):.1f} us, would be "
                 f"{100 * (t5 + t6) / res['segment']:.3f} % of a segment call")


def main():
    lines = []
    ops = bench_ops(lines)
    bench_calls(lines, ops)
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 1:
        Path(sys.argv[1]).parent.mkdir(parents=True, exist_ok=True)
        Path(sys.argv[1]).write_text(text + "\n")


if __name__ == "__main__":
    main()

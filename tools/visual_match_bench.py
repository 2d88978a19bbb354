"""What a visual embedding and an exemplar match cost on the device, in ONE process.
(a) `Florence2Captioner.embed_crops` (the DaViT tower and the projector, then OMNI_OP_VISUAL_MATCH mode 0) beside `caption_crops`
    (the same, plus the BART encoder, the cross-K/V GEMMs and 20 decode steps) on the same 128 crops of a synthetic screenshot, at
    768x768 and at 64x64 crops: wall time of a synchronised call, median (min) of 5 after a warm-up call.  `caption_crops` is called
    as the commit before the embeddings called it, so the same file measures that commit (the embed column is then left out).
(b) OMNI_OP_VISUAL_MATCH modes 1 + 2 at D = 768, k = 5 for (queries, gallery rows) = (300, 300), (300, 65536), (4096, 65536): HIP events
    around both ops of an eager replay (omni_plan_profile), median (min) of 10 after a warm-up replay, and the HBM rate the
    algorithmic bytes of opwork.op_work imply (queries and gallery read once, partials written once).
usage: python tools/visual_match_bench.py [out.txt] [crops=128]   -> a table on stdout (and into out.txt)"""
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def bench_calls(lines, n_crops):
    import torch
    import gpu_checks as G
    from omniparser_amd.florence import Florence2Captioner
    from omniparser_amd.synth import synthetic_screenshot
    from tools.make_weights import ensure_caption_checkpoint
    frame = torch.from_numpy(synthetic_screenshot(5)).cuda()
    boxes = G.real_crop_boxes(5, n_crops)
    lines.append(f"(a) {n_crops} crops of a 1920x1080 synthetic screenshot, f32 plans, stand-in checkpoint; ms per synchronised call, median (min) of 5")
    for R in (768, 64):
        cap = Florence2Captioner(ensure_caption_checkpoint(0), "cuda", precision="f32", resolution=R)
        calls = {"caption_crops": lambda: cap.caption_crops(frame, boxes)}
        if hasattr(cap, "embed_crops"):
            calls["embed_crops"] = lambda: cap.embed_crops(frame, boxes)
            calls["caption_crops(return_embeddings=True)"] = lambda: cap.caption_crops(frame, boxes, return_embeddings=True)
        for name, fn in calls.items():
            fn()
            torch.cuda.synchronize()
            ts = []
            for _ in range(5):
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts.append(1e3 * (time.perf_counter() - t0))
            lines.append(f"  {R:>3}x{R:<3} {name:<40}{statistics.median(ts):9.2f} ({min(ts):.2f})")
        torch.cuda.synchronize()
        cap.clear_plans()
        del cap
        torch.cuda.empty_cache()


def bench_match(lines):
    import torch
    from omniparser_amd import _lib as L
    from omniparser_amd import opwork
    from omniparser_amd.florence import match_geometry, match_ops
    D, k = 768, 5
    lines += ["", f"(b) OMNI_OP_VISUAL_MATCH modes 1 + 2, D = {D}, k = {k}: omni_plan_profile of [partial top-k, merge], 10 replays after a warm-up; "
              "microseconds median (min); GB/s = algorithmic bytes of the launch / its median time"]
    g = torch.Generator().manual_seed(0)
    for m, n in ((300, 300), (300, 65536), (4096, 65536)):
        q = torch.nn.functional.normalize(torch.randn(m, D, generator=g), dim=1).cuda()
        gal = torch.nn.functional.normalize(torch.randn(n, D, generator=g), dim=1).cuda()
        groups, length, splits, nbytes = match_geometry(m, n, D, k)
        part = torch.empty(nbytes // 4, dtype=torch.int32, device="cuda")
        idx = torch.empty((m, k), dtype=torch.int32, device="cuda")
        score = torch.empty((m, k), dtype=torch.float32, device="cuda")
        ops = list(match_ops(q.data_ptr(), gal.data_ptr(), part.data_ptr(), idx.data_ptr(), score.data_ptr(), m, n, D, k, 0, nbytes))
        torch.cuda.synchronize()
        plan = L.Plan(ops)
        s = torch.cuda.Stream()
        times = [[], []]
        with torch.cuda.stream(s):
            plan.run(s)
            s.synchronize()
            for _ in range(10):
                t = plan.profile(s)
                times[0].append(t[0])
                times[1].append(t[1])
        s.synchronize()
        want = (q @ gal.T).topk(k, dim=1).indices
        agree = float((idx.long() == want).float().mean())
        ops[0].i[5] = length                                 # the launcher's split, for the byte count of the partials
        ops[1].i[5] = length
        lines.append(f"  m = {m:>4}, n = {n:>5}: {groups} query groups x {splits} slices of {length} rows; top-{k} agrees with torch.topk of the f32 GEMM in {100 * agree:.2f} % of positions")
        for name, op, ts in (("partial top-k", ops[0], times[0]), ("merge", ops[1], times[1])):
            flops, nb = opwork.op_work(op)
            med = statistics.median(ts)
            lines.append(f"    {name:<14}{1e3 * med:10.1f} ({1e3 * min(ts):.1f}) us   {nb / 1e6:9.2f} MB -> {nb / (med * 1e-3) / 1e9:8.1f} GB/s"
                         + (f"   {flops / (med * 1e-3) / 1e12:6.2f} TFLOP/s" if flops else ""))


def main():
    lines = []
    bench_calls(lines, int(sys.argv[2]) if len(sys.argv) > 2 else 128)
    bench_match(lines)
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 1:
        Path(sys.argv[1]).parent.mkdir(parents=True, exist_ok=True)
        Path(sys.argv[1]).write_text(text + "\n")


if __name__ == "__main__":
    main()

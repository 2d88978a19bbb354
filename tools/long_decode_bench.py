"""One decode step of the captioner over a LONG history: median device time of the captured step graph of a 128-row plan at 64x64
crops with 20, 128, 512 and 1024 new tokens, the step counter parked two positions before the end (max_new - 1 keys in the
self-attention, an unforced position for the greedy op, seeded token history), and the per-kernel time of the six self-attention
ops and of the greedy op from the per-op profiler (HIP events around every op of an eager run: omni_plan_profile).  It uses only
`Florence2Captioner.plans`, so the same file measures any commit of this repository; compare two commits only from runs on the same
device in the same session.
usage: python tools/long_decode_bench.py [out.json] [rows=128]   -> JSON on stdout (and into out.json)"""
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

LENGTHS = (20, 128, 512, 1024)
WARMUP, REPEATS, PROFILES = 10, 41, 9


def main():
    import torch
    from omniparser_amd import _lib as L
    from omniparser_amd.florence import Florence2Captioner
    from tools.make_weights import caption_dir, ensure_via_subprocess
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    rows = int(sys.argv[2]) if len(sys.argv) > 2 else 128
    R = 64
    ensure_via_subprocess("caption", seed=0)
    cap = Florence2Captioner(caption_dir(0), "cuda", precision="f32", resolution=R)
    out = {"rows": rows, "R": R, "vocab": cap.w.vocab, "device": torch.cuda.get_device_name(0),
           "method": f"step: one hipGraph replay between two events, step counter rewritten before each, {WARMUP} warm-up replays, "
                     f"median of {REPEATS}; ops: omni_plan_profile of an eager run, median of {PROFILES}",
           "lengths": {}}
    g = torch.Generator().manual_seed(0)
    for max_new in LENGTHS:
        cp = cap.plans(rows, R, max_new)
        st = max_new - 2
        ops = cp.step_plan.ops
        self_ops = [j for j, op in enumerate(ops) if op.kind == L.OP_ATTN_DECODE and op.i[7] <= 0]
        greedy = [j for j, op in enumerate(ops) if op.kind == L.OP_GREEDY_STEP]
        assert len(self_ops) == cap.w.dec_layers and len(greedy) == 1
        with torch.inference_mode(), torch.cuda.stream(cap.stream):
            cp.reset()
            ids = torch.randint(3, cap.w.vocab, tuple(cp.ids.shape), generator=g, dtype=torch.int32)
            ids[:, 0] = cp.start_token
            cp.ids.copy_(ids)
            for c in cp.cross_kv:
                c.t.zero_()
            for c in cp.self_k + cp.self_v:
                c.t.zero_()
            park = torch.tensor([st], dtype=torch.int32, device=cap.device)
            for _ in range(WARMUP):
                cp.step.copy_(park)
                cp.step_plan.replay(cap.stream)
            step_ms = []
            for _ in range(REPEATS):
                cp.step.copy_(park)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(cap.stream)
                cp.step_plan.replay(cap.stream)
                b.record(cap.stream)
                cap.stream.synchronize()
                step_ms.append(a.elapsed_time(b))
            attn_ms, greedy_ms = [], []
            for _ in range(PROFILES):
                cp.step.copy_(park)
                t = cp.step_plan.profile(cap.stream)
                attn_ms.append(sum(t[j] for j in self_ops)); greedy_ms.append(t[greedy[0]])
            cap.stream.synchronize()
        out["lengths"][str(max_new)] = {
            "max_new_tokens": max_new, "self_attention_keys": st + 1, "ops": len(ops),
            "self_kv_MB": round(2 * cap.w.dec_layers * rows * (max_new + 1) * cap.w.d_model * 4 / 1e6, 1),
            "graph_step_ms": round(statistics.median(step_ms), 4), "graph_step_ms_min": round(min(step_ms), 4),
            "graph_step_ms_p90": round(sorted(step_ms)[int(0.9 * (len(step_ms) - 1))], 4),
            "self_attention_6_ops_ms": round(statistics.median(attn_ms), 4), "greedy_op_ms": round(statistics.median(greedy_ms), 4)}
        cap.clear_plans()
        del cp
        torch.cuda.empty_cache()
    text = json.dumps(out, indent=1)
    print(text)
    if out_path:
        Path(out_path).parent.mkdir(parents=True, exist_ok=True)
        Path(out_path).write_text(text + "\n")


if __name__ == "__main__":
    main()

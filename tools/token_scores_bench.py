"""Cost of the token log-probabilities of greedy decoding (OMNI_OP_GREEDY_STEP p4) on the merged decode plan: device time of the
greedy op (HIP events around every op of an eager replay: omni_plan_profile) and of one whole decode step (graph replays between two
events), scores off and scores on, in ONE process on plans of the same shape.
usage: python tools/token_scores_bench.py [rows=384] [R=768] [out.json]   -> JSON on stdout (and into out.json)"""
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def main():
    import torch
    from omniparser_amd import _lib as L
    from omniparser_amd.florence import Florence2Captioner
    from tools.make_weights import caption_dir, ensure_via_subprocess
    rows = int(sys.argv[1]) if len(sys.argv) > 1 else 384
    R = int(sys.argv[2]) if len(sys.argv) > 2 else 768
    ensure_via_subprocess("caption", seed=0)
    cap = Florence2Captioner(caption_dir(0), "cuda", precision="f32", resolution=R)
    max_new = 20
    out = {"rows": rows, "R": R, "max_new_tokens": max_new, "vocab": cap.w.vocab, "logits_MB": round(rows * cap.w.vocab * 4 / 1e6, 1),
           "method": "greedy op: omni_plan_profile (HIP events around every op of an eager replay), mean over 20 steps x 3 passes; "
                     "step: 20 hipGraph replays between two events / 20, median of 7"}
    g = torch.Generator().manual_seed(0)
    kv = None
    for name, scores in (("scores_off", False), ("scores_on", True), ("scores_off_again", False)):
        dec = cap.decode_plans(rows, R, max_new, scores=scores)
        with torch.inference_mode(), torch.cuda.stream(cap.stream):
            if kv is None:                           # the same (random, finite) cross-attention K / V for both plans
                kv = [torch.randn(tuple(c.t.shape), generator=g).to(cap.device).to(c.t.dtype) for c in dec.cross_kv[:1]]
            for c in dec.cross_kv:
                c.t.copy_(kv[0])
            greedy = [j for j, op in enumerate(dec.step_plan.ops) if op.kind == L.OP_GREEDY_STEP]
            assert len(greedy) == 1 and (dec.step_plan.ops[greedy[0]].p[4] is not None) == scores
            op_ms, eager_ms = [], []
            for _ in range(3):
                dec.reset()
                for _ in range(max_new):
                    t = dec.step_plan.profile(cap.stream)
                    op_ms.append(t[greedy[0]]); eager_ms.append(sum(t))
            step_ms = []
            for _ in range(7):
                dec.reset()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(cap.stream)
                for _ in range(max_new):
                    dec.step_plan.replay(cap.stream)
                b.record(cap.stream)
                cap.stream.synchronize()
                step_ms.append(a.elapsed_time(b) / max_new)
        out[name] = {"greedy_op_ms": round(statistics.mean(op_ms), 4), "greedy_op_ms_min": round(min(op_ms), 4),
                     "eager_step_ms_sum_of_ops": round(statistics.mean(eager_ms), 3), "graph_step_ms": round(statistics.median(step_ms), 4),
                     "graph_step_ms_all": [round(v, 4) for v in step_ms], "ops": len(dec.step_plan.ops)}
    off, on = out["scores_off"], out["scores_on"]
    out["scores_on_cost"] = {"greedy_op_ms": round(on["greedy_op_ms"] - off["greedy_op_ms"], 4),
                             "graph_step_ms": round(on["graph_step_ms"] - off["graph_step_ms"], 4),
                             "graph_step_pct": round(100.0 * (on["graph_step_ms"] / off["graph_step_ms"] - 1.0), 2)}
    text = json.dumps(out, indent=1)
    print(text)
    if len(sys.argv) > 3:
        Path(sys.argv[3]).parent.mkdir(parents=True, exist_ok=True)
        Path(sys.argv[3]).write_text(text + "\n")


if __name__ == "__main__":
    main()

"""Device time of the target-score form of OMNI_OP_GREEDY_STEP (p5: one pass over the row, online max / sum / arg-max) beside the
scores instantiation of the generating form (p4: arg-max pass + sum pass) on the same logits, in ONE process: HIP events around every
op of an eager replay (omni_plan_profile), the two ops alternating in one plan.
usage: python tools/target_scores_bench.py [rows=1024] [vocab=51289] [out.json]   -> JSON on stdout (and into out.json)"""
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def main():
    import torch
    from omniparser_amd import _lib as L
    rows = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    V = int(sys.argv[2]) if len(sys.argv) > 2 else 51289
    T = 21
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(0)
    out = {"rows": rows, "vocab": V, "method": "omni_plan_profile of a plan [generate+scores, target-score] x 4, 10 replays, step pinned at 3"}
    for name, tdt, dt in (("f32", torch.float32, L.F32), ("f16", torch.float16, L.F16)):
        logits = (torch.randn(rows, V, generator=g) * 3).to(tdt).to(dev)
        bias = (torch.randn(V, generator=g) * 0.5).to(dev)
        ids = torch.randint(0, V, (rows, T), generator=g, dtype=torch.int32).to(dev)
        ids2 = ids.clone()
        fin = torch.zeros(rows, dtype=torch.int32, device=dev)
        step = torch.full((1,), 3, dtype=torch.int32, device=dev)
        logp, logp2 = torch.zeros(rows, T, device=dev), torch.zeros(rows, T, device=dev)
        top1 = torch.zeros(rows, T, dtype=torch.int32, device=dev)
        tlen = torch.full((rows,), T - 1, dtype=torch.int32, device=dev)
        common = {0: rows, 1: V, 2: V, 3: T, 4: T - 1, 6: 0, 7: 2, 8: 1, 9: -1, 10: -1, 11: 0}
        gen = L.make_op(L.OP_GREEDY_STEP, dt, p=[logits.data_ptr(), bias.data_ptr(), ids2.data_ptr(), fin.data_ptr(), logp2.data_ptr(), None,
                                                 step.data_ptr()], i={**common, 5: 0})
        tgt = L.make_op(L.OP_GREEDY_STEP, dt, p=[logits.data_ptr(), bias.data_ptr(), ids.data_ptr(), None, logp.data_ptr(), tlen.data_ptr(),
                                                 step.data_ptr(), top1.data_ptr()], i=common)
        plan = L.Plan([gen, tgt] * 4)
        st = torch.cuda.Stream()
        torch.cuda.synchronize()                                # the uploads above ran on the current stream
        t_gen, t_tgt = [], []
        with torch.cuda.stream(st):
            plan.run(st)
            st.synchronize()
            for _ in range(10):
                fin.zero_()
                t = plan.profile(st)
                t_gen += t[0::2]; t_tgt += t[1::2]
        st.synchronize()
        mb = rows * V * logits.element_size() / 1e6
        out[name] = {"logits_MB": round(mb, 1), "generate_with_scores_ms": round(statistics.median(t_gen), 4),
                     "target_score_ms": round(statistics.median(t_tgt), 4), "generate_with_scores_ms_min": round(min(t_gen), 4),
                     "target_score_ms_min": round(min(t_tgt), 4), "target_score_GBps": round(mb / statistics.median(t_tgt), 1),
                     "generate_with_scores_GBps_of_two_reads": round(2 * mb / statistics.median(t_gen), 1)}
    text = json.dumps(out, indent=1)
    print(text)
    if len(sys.argv) > 3:
        Path(sys.argv[3]).parent.mkdir(parents=True, exist_ok=True)
        Path(sys.argv[3]).write_text(text + "\n")


if __name__ == "__main__":
    main()

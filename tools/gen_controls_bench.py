"""Device time of OMNI_OP_GREEDY_CTRL_STEP beside OMNI_OP_GREEDY_STEP's bitmap (long-history) form on the same operands, in ONE
process: HIP events around every op of an eager replay (omni_plan_profile), the ops alternating in one plan.  The history is
long_checks' (122 tokens with repeated 3-grams in rows 0 and 3 of every four), the step is pinned (i11 = 0).
usage: python tools/gen_controls_bench.py [rows=128] [vocab=51289] [out.txt]   -> a table on stdout (and into out.txt)"""
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import torch
    import long_checks as LC
    from omniparser_amd import _lib as L
    from omniparser_amd.florence import GenerationControls, gen_ctrl_words
    rows = int(sys.argv[1]) if len(sys.argv) > 1 else 128
    V = int(sys.argv[2]) if len(sys.argv) > 2 else 51289
    T, max_new, st = LC.GT, LC.GMAX_NEW, LC.GSTEP
    dev = torch.device("cuda")
    settings = {"neutral block": GenerationControls(),
                "penalty 1.3": GenerationControls(repetition_penalty=1.3),
                "every control": GenerationControls(repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=max_new,
                                                    suppress_tokens=list(range(5, 400, 7)), begin_suppress_tokens=[9, 10],
                                                    bad_words_ids=[[220, 221, 600 + k] for k in range(64)])}
    lines = [f"OMNI_OP_GREEDY_CTRL_STEP beside OMNI_OP_GREEDY_STEP (bitmap form: max_new {max_new}, n-gram 3), B = {rows}, V = {V}, T = {T}, "
             f"step {st}", "omni_plan_profile (HIP events around every op of an eager replay) of a plan [greedy_step, ctrl_step x 3 settings] x 4, "
             "10 replays after a warm-up replay; median (min) microseconds per launch", ""]
    for name, tdt, dt in (("f32", torch.float32, L.F32), ("f16", torch.float16, L.F16)):
        ids4, logits4, bias, fin4, _ = LC.long_greedy_inputs(V, tdt)
        rep = (rows + 3) // 4
        ids = ids4.repeat(rep, 1)[:rows].contiguous().to(dev)
        logits = logits4.repeat(rep, 1)[:rows].contiguous().to(dev)
        fin = torch.zeros(rows, dtype=torch.int32, device=dev)
        bias = bias.to(dev)
        step = torch.full((1,), st, dtype=torch.int32, device=dev)
        for scores in (False, True):
            logp = torch.zeros(rows, T, device=dev) if scores else None
            common = {0: rows, 1: V, 2: V, 3: T, 4: max_new, 5: 3, 6: 0, 7: 2, 8: 1, 9: 0, 10: 2, 11: 0}
            ptrs = [logits.data_ptr(), bias.data_ptr(), ids.data_ptr(), fin.data_ptr(), logp.data_ptr() if scores else None, None, step.data_ptr()]
            ops = [L.make_op(L.OP_GREEDY_STEP, dt, p=ptrs, i=common)]
            blocks = []
            for gc in settings.values():
                buf = torch.zeros(gen_ctrl_words(V), dtype=torch.int32)
                w = gc.pack(V, 0)
                buf[:w.numel()] = w
                blocks.append(buf.to(dev))
                ops.append(L.make_op(L.OP_GREEDY_CTRL_STEP, dt, p=ptrs + [blocks[-1].data_ptr()], i={**common, 12: buf.numel() * 4}))
            torch.cuda.synchronize()                            # the uploads ran on the current stream; plan creation reads the headers
            plan = L.Plan(ops * 4)
            s = torch.cuda.Stream()
            times = [[] for _ in ops]
            with torch.cuda.stream(s):
                plan.run(s)
                s.synchronize()
                for _ in range(10):
                    fin.zero_()
                    t = plan.profile(s)
                    for k in range(len(ops)):
                        times[k] += t[k::len(ops)]
            s.synchronize()
            fmt = lambda v: f"{1e3 * statistics.median(v):8.1f} ({1e3 * min(v):.1f})"
            lines.append(f"{name} logits, p4 {'set' if scores else 'NULL'}:")
            lines.append(f"  greedy_step_long_kernel                  {fmt(times[0])}")
            for k, label in enumerate(settings):
                lines.append(f"  greedy_ctrl_step_kernel, {label:<15} {fmt(times[k + 1])}")
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 3:
        Path(sys.argv[3]).parent.mkdir(parents=True, exist_ok=True)
        Path(sys.argv[3]).write_text(text + "\n")


if __name__ == "__main__":
    main()

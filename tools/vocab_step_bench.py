"""Device time of OMNI_OP_GREEDY_VOCAB_STEP beside OMNI_OP_GREEDY_STEP on the same operands, in ONE process: HIP events around every
op of an eager replay (omni_plan_profile), the ops alternating in one plan.  Two settings of the rows' trie nodes: every row at a
root-heavy node with ~5000 children, and every row at a typical node with 1..16 children.  The history is the first 14 tokens of
long_checks' (rows 0 and 3 of every four end in a repeated 2-gram, so the 3-gram ban is live), max_new_tokens = 20 (the captions'
default: OMNI_OP_GREEDY_STEP runs its list form), the step is pinned (i11 = 0) and every row is finished, so that no launch moves a
node: a finished row costs what any row costs (the flag is read by one thread behind the arg-max).
usage: python tools/vocab_step_bench.py [rows=128] [vocab=51289] [out.txt]   -> a table on stdout (and into out.txt)"""
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

WIDE, TYPICAL = 5000, 128          # children of the root-heavy node; typical nodes (node k has k % 16 + 1 children)


def bench_vocabulary(V):
    from omniparser_amd.florence import CaptionVocabulary
    firsts = list(range(1000, 1000 + WIDE))
    labels = [[0, c, 2] for c in firsts[TYPICAL:]]
    for k, c in enumerate(firsts[:TYPICAL]):
        labels += [[0, c, 20000 + 97 * k + 7 * j, 2] for j in range(k % 16 + 1)]
    v = CaptionVocabulary(labels).check(V, 20, 2, 0, 2, 3, 2)
    return v, v.walk([0]), [v.walk([0, c]) for c in firsts[:TYPICAL]]


def main():
    import torch
    import long_checks as LC
    from omniparser_amd import _lib as L
    from omniparser_amd.florence import vocab_trie_words
    rows = int(sys.argv[1]) if len(sys.argv) > 1 else 128
    V = int(sys.argv[2]) if len(sys.argv) > 2 else 51289
    T, max_new, st = 21, 20, 13
    dev = torch.device("cuda")
    vocab, wide, typical = bench_vocabulary(V)
    assert len(vocab.children(wide)) == WIDE and all(1 <= len(vocab.children(n)) <= 16 for n in typical)
    buf = torch.zeros(vocab_trie_words(), dtype=torch.int32)
    block = vocab.pack()
    buf[:block.numel()] = block
    trie = buf.to(dev)
    nodes = {f"node with {WIDE} children": torch.full((rows,), wide, dtype=torch.int32).to(dev),
             "nodes with 1..16 children": torch.tensor([typical[r % TYPICAL] for r in range(rows)], dtype=torch.int32).to(dev)}
    lines = [f"OMNI_OP_GREEDY_VOCAB_STEP beside OMNI_OP_GREEDY_STEP (list form: max_new {max_new}, n-gram 3), B = {rows}, V = {V}, T = {T}, "
             f"step {st}; trie of {vocab.n_nodes} nodes ({block.numel() * 4} bytes) in a buffer of {buf.numel() * 4} bytes",
             "omni_plan_profile (HIP events around every op of an eager replay) of a plan [greedy_step, vocab_step x 2 settings] x 4, "
             "10 replays after a warm-up replay; median (min) microseconds per launch", ""]
    for name, tdt, dt in (("f32", torch.float32, L.F32), ("f16", torch.float16, L.F16)):
        ids4, logits4, bias, fin4, _ = LC.long_greedy_inputs(V, tdt)
        rep = (rows + 3) // 4
        ids = ids4[:, :T].repeat(rep, 1)[:rows].contiguous().to(dev)
        logits = logits4.repeat(rep, 1)[:rows].contiguous().to(dev)
        fin = torch.ones(rows, dtype=torch.int32, device=dev)
        bias = bias.to(dev)
        step = torch.full((1,), st, dtype=torch.int32, device=dev)
        for scores in (False, True):
            logp = torch.zeros(rows, T, device=dev) if scores else None
            common = {0: rows, 1: V, 2: V, 3: T, 4: max_new, 5: 3, 6: 0, 7: 2, 8: 1, 9: 0, 10: 2, 11: 0}
            ptrs = [logits.data_ptr(), bias.data_ptr(), ids.data_ptr(), fin.data_ptr(), logp.data_ptr() if scores else None]
            ops = [L.make_op(L.OP_GREEDY_STEP, dt, p=ptrs + [None, step.data_ptr()], i=common)]
            for nd in nodes.values():
                ops.append(L.make_op(L.OP_GREEDY_VOCAB_STEP, dt, p=ptrs + [nd.data_ptr(), step.data_ptr(), trie.data_ptr()],
                                     i={**common, 12: buf.numel() * 4}))
            torch.cuda.synchronize()                            # the uploads ran on the current stream; plan creation reads the header
            plan = L.Plan(ops * 4)
            s = torch.cuda.Stream()
            times = [[] for _ in ops]
            with torch.cuda.stream(s):
                plan.run(s)
                s.synchronize()
                for _ in range(10):
                    t = plan.profile(s)
                    for k in range(len(ops)):
                        times[k] += t[k::len(ops)]
            s.synchronize()
            assert all(int(nd.min()) == int(nd.max()) or nd.tolist() == [typical[r % TYPICAL] for r in range(rows)] for nd in nodes.values())
            fmt = lambda v: f"{1e3 * statistics.median(v):8.1f} ({1e3 * min(v):.1f})"
            lines.append(f"{name} logits, p4 {'set' if scores else 'NULL'}:")
            lines.append(f"  greedy_step_kernel                                  {fmt(times[0])}")
            for k, label in enumerate(nodes):
                lines.append(f"  greedy_vocab_step_kernel, {label:<26}{fmt(times[k + 1])}")
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 3:
        Path(sys.argv[3]).parent.mkdir(parents=True, exist_ok=True)
        Path(sys.argv[3]).write_text(text + "\n")


if __name__ == "__main__":
    main()

"""Per-stage device time of the DaViT channel blocks' attention part in a caption encode plan: the qkv linear (one launch, or the
q|k + v pair of a folded block, reported separately as well), OMNI_OP_CHAN_ATTN (scores + softmax + apply, scores + softmax + fold +
pack, or — behind the scores epilogue of the q|k launch — softmax + fold + pack) and the projection GEMM — HIP events around every op
of an eager replay (omni_plan_profile), one line per stage and repeat.
usage: python tools/chan_fold_profile.py [capacity=128] [R=768] [repeats=3] [fold=1|0] [root] [scores_in_gemm=1|0]
`root`: import omniparser_amd from another checkout (an A/B against a tree without a switch: the table has the same rows; "." = this
tree).  `scores_in_gemm`: Florence2Captioner.chan_scores_in_gemm where the checkout has it."""
import json
import sys
from pathlib import Path


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 128
    R = int(sys.argv[2]) if len(sys.argv) > 2 else 768
    rep = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    fold = (sys.argv[4] != "0") if len(sys.argv) > 4 else True
    root = Path(sys.argv[5]).resolve() if len(sys.argv) > 5 and sys.argv[5] != "." else Path(__file__).resolve().parents[1]
    scores = (sys.argv[6] != "0") if len(sys.argv) > 6 else True
    sys.path.insert(0, str(root))
    import torch
    from omniparser_amd import _lib as L
    from omniparser_amd.florence import Florence2Captioner
    from tools.make_weights import caption_dir, ensure_via_subprocess
    if hasattr(Florence2Captioner, "fold_chan_proj"):
        Florence2Captioner.fold_chan_proj = fold
    if hasattr(Florence2Captioner, "chan_scores_in_gemm"):
        Florence2Captioner.chan_scores_in_gemm = scores
    ensure_via_subprocess("caption", seed=0)
    cap = Florence2Captioner(caption_dir(0), "cuda", precision="f32", resolution=R)
    cap.use_graph = False
    cp = cap.plans(B, R, 20)
    g = torch.Generator().manual_seed(0)
    with torch.inference_mode(), torch.cuda.stream(cap.stream):
        low = torch.randn(B, 8, 8, 3, generator=g).permute(0, 3, 1, 2)
        x = torch.nn.functional.interpolate(low, size=(R, R), mode="bicubic").permute(0, 2, 3, 1).contiguous()
        cp.x_in.t[:, :, :, :3] = x.to(cap.device)
        cp.reset()
        cp.encode_plan.run(cap.stream)
        cap.stream.synchronize()
    ops = cp.encode_plan.ops
    blocks = []                                    # (C, folded, indices of the qkv launch(es), index of chan_attn, index of the projection)
    for j, op in enumerate(ops):
        if op.kind == L.OP_CHAN_ATTN:
            folded = op.i[8] == 1
            blocks.append((op.i[3], folded, [j - 2, j - 1] if folded else [j - 1], j, j + 1))
    out = {"capacity": B, "R": R, "root": str(root), "fold_stages": list(getattr(cp, "fold_stages", [])),
           "chan_scores_in_gemm": bool(getattr(Florence2Captioner, "chan_scores_in_gemm", False)) and scores,
           "scores_epilogue_launches": sum(1 for op in ops if op.kind == L.OP_CONV and op.i[20] == 2 and op.i[28] == 1),
           "hbm_peak_allocated_gb": None, "repeats": []}
    with torch.inference_mode():
        for r in range(rep):
            ms = cp.encode_plan.profile(cap.stream)
            row = {"encode_ms": round(sum(ms), 3), "stages": {}}
            for C, folded, qi, ci, pi in blocks:
                s = row["stages"].setdefault(C, {"folded": folded, "blocks": 0, "qkv": 0.0, "qk": 0.0, "v": 0.0, "chan_attn": 0.0, "proj": 0.0})
                s["blocks"] += 1
                s["qkv"] += sum(ms[k] for k in qi); s["chan_attn"] += ms[ci]; s["proj"] += ms[pi]
                if folded:
                    s["qk"] += ms[qi[0]]; s["v"] += ms[qi[1]]
            for C, s in row["stages"].items():
                s["sum"] = s["qkv"] + s["chan_attn"] + s["proj"]
                s["attn_sum"] = s["qkv"] + s["chan_attn"]                 # q|k launch + v launch + chan_attn op: what the scores epilogue moves
                print("repeat %d  C=%-4d %-8s blocks %d  qkv %7.3f (q|k %7.3f  v %7.3f)  chan_attn %7.3f  proj %7.3f  qkv+chan %7.3f  sum %7.3f ms   (encode %.2f ms)"
                      % (r, C, "folded" if s["folded"] else "unfolded", s["blocks"], s["qkv"], s["qk"], s["v"], s["chan_attn"], s["proj"],
                         s["attn_sum"], s["sum"], row["encode_ms"]))
            out["repeats"].append(row)
    out["hbm_peak_allocated_gb"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

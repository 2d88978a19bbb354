"""Per-stage device time of the DaViT channel blocks' attention part in a caption encode plan: the qkv linear (one launch, or the
q|k + v pair of a folded block, reported separately as well), OMNI_OP_CHAN_ATTN (scores + softmax + apply, scores + softmax + fold +
pack, or — behind the scores epilogue of the q|k launch — softmax + fold + pack) and the projection GEMM — HIP events around every op
of an eager replay (omni_plan_profile), one line per stage and repeat.  A block with Wv folded in as well (Florence2Captioner.fold_chan_v)
has no v launch; its chan_attn column includes the per-image bias kernel, and the fold GEMM W' . Wv and the re-pack behind it are columns
of their own: sum = q|k + chan_attn + fold GEMM + re-pack + proj.
usage: python tools/chan_fold_profile.py [capacity=128] [R=768] [repeats=3] [fold=1|0] [root] [scores_in_gemm=1|0] [fold_v=1|0]
`root`: import omniparser_amd from another checkout (an A/B against a tree without a switch: the table has the same rows; "." = this
tree).  `scores_in_gemm` / `fold_v`: Florence2Captioner.chan_scores_in_gemm / fold_chan_v where the checkout has them."""
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
    fold_v = (sys.argv[7] != "0") if len(sys.argv) > 7 else True
    sys.path.insert(0, str(root))
    import torch
    from omniparser_amd import _lib as L
    from omniparser_amd.florence import Florence2Captioner
    from tools.make_weights import caption_dir, ensure_via_subprocess
    if hasattr(Florence2Captioner, "fold_chan_proj"):
        Florence2Captioner.fold_chan_proj = fold
    if hasattr(Florence2Captioner, "chan_scores_in_gemm"):
        Florence2Captioner.chan_scores_in_gemm = scores
    if hasattr(Florence2Captioner, "fold_chan_v"):
        Florence2Captioner.fold_chan_v = fold_v
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
    # (C, folded, indices of the qkv launch(es), index of chan_attn, index of the projection, indices of the fold GEMM and the re-pack or None)
    blocks = []
    for j, op in enumerate(ops):
        if op.kind == L.OP_CHAN_ATTN and op.i[11] == 1:          # Wv folded in: q|k, chan_attn, fold GEMM, re-pack, projection
            blocks.append((op.i[3], True, [j - 1], j, j + 3, (j + 1, j + 2)))
        elif op.kind == L.OP_CHAN_ATTN and op.i[11] == 0:
            folded = op.i[8] == 1
            blocks.append((op.i[3], folded, [j - 2, j - 1] if folded else [j - 1], j, j + 1, None))
    out = {"capacity": B, "R": R, "root": str(root), "fold_stages": list(getattr(cp, "fold_stages", [])),
           "chan_scores_in_gemm": bool(getattr(Florence2Captioner, "chan_scores_in_gemm", False)) and scores,
           "fold_chan_v": bool(getattr(Florence2Captioner, "fold_chan_v", False)) and fold_v,
           "fold_gemm_launches": sum(1 for op in ops if op.kind == L.OP_CONV and op.i[20] == 2 and op.i[26] > 0 and op.i[27] == 0 and op.i[28] == 0),
           "scores_epilogue_launches": sum(1 for op in ops if op.kind == L.OP_CONV and op.i[20] == 2 and op.i[28] == 1),
           "hbm_peak_allocated_gb": None, "repeats": []}
    with torch.inference_mode():
        for r in range(rep):
            ms = cp.encode_plan.profile(cap.stream)
            row = {"encode_ms": round(sum(ms), 3), "stages": {}}
            for C, folded, qi, ci, pi, vf in blocks:
                s = row["stages"].setdefault(C, {"folded": folded, "fold_v": vf is not None, "blocks": 0, "qkv": 0.0, "qk": 0.0, "v": 0.0,
                                                 "chan_attn": 0.0, "fold_gemm": 0.0, "repack": 0.0, "proj": 0.0})
                s["blocks"] += 1
                s["qkv"] += sum(ms[k] for k in qi); s["chan_attn"] += ms[ci]; s["proj"] += ms[pi]
                if folded:
                    s["qk"] += ms[qi[0]]; s["v"] += ms[qi[1]] if len(qi) > 1 else 0.0
                if vf is not None:
                    s["fold_gemm"] += ms[vf[0]]; s["repack"] += ms[vf[1]]
            for C, s in row["stages"].items():
                s["sum"] = s["qkv"] + s["chan_attn"] + s["fold_gemm"] + s["repack"] + s["proj"]
                s["attn_sum"] = s["qkv"] + s["chan_attn"]                 # q|k launch + v launch + chan_attn op: what the scores epilogue moves
                print("repeat %d  C=%-4d %-8s blocks %d  qkv %7.3f (q|k %7.3f  v %7.3f)  chan_attn %7.3f  fold_gemm %7.3f  repack %7.3f  proj %7.3f  qkv+chan %7.3f  sum %7.3f ms   (encode %.2f ms)"
                      % (r, C, ("folded+v" if s["fold_v"] else "folded") if s["folded"] else "unfolded", s["blocks"], s["qkv"], s["qk"], s["v"],
                         s["chan_attn"], s["fold_gemm"], s["repack"], s["proj"], s["attn_sum"], s["sum"], row["encode_ms"]))
            out["repeats"].append(row)
    out["hbm_peak_allocated_gb"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""Static VALU census of the gfx950 GEMM kernels (csrc/gemm_dma.hip): per `gemm_dma_kernel` / `mlp_fused_kernel` instantiation the
VALU instructions by class (packed f32, conversions, compare / select, transcendental, other), the `s_nop` count, how much of the
kernel lies after its last MFMA (= the epilogue of `gemm_dma_kernel`), registers and LDS.  Needs only hipcc, no GPU:
    python tools/gemm_epilogue_isa.py [filter] [-DNAME=VALUE ...]
The epilogues run with the matrix pipe idle (both waves of a SIMD reach them together), so their VALU issue slots are wall time:
profiles/gemm_epilogue_isa.txt records this report before and after the epilogue was trimmed."""
import re
import subprocess
import sys
import tempfile
from collections import Counter
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from omniparser_amd.build import FLAGS, HIPCC  # noqa: E402
from tools.isa_report import demangle, waves_per_simd  # noqa: E402

TRANS = ("v_exp", "v_log", "v_rcp", "v_rsq", "v_sqrt", "v_sin", "v_cos")
CLASSES = ("pk_f32", "cvt", "cmp_sel", "trans", "other")


def valu_class(op: str):
    """class of a VALU opcode, None for anything that is not VALU (MFMA and accumulator moves included)"""
    if not op.startswith("v_") or op.startswith("v_mfma") or op.startswith("v_accvgpr"):
        return None
    if op.startswith("v_pk_") and op.split("_e")[0].endswith("_f32"):
        return "pk_f32"
    if op.startswith("v_cvt"):
        return "cvt"
    if op.startswith("v_cmp") or op.startswith("v_cndmask"):
        return "cmp_sel"
    if op.startswith(TRANS):
        return "trans"
    return "other"


def census(body):
    ops = []
    for l in body:
        t = l.split(";")[0].strip().split()
        if t and not t[0].endswith(":") and not t[0].startswith("."):
            ops.append(t[0])
    last = max((i for i, o in enumerate(ops) if o.startswith("v_mfma")), default=-1)
    whole, tail = Counter(), Counter()
    for i, o in enumerate(ops):
        c = valu_class(o)
        for cnt in (whole,) + ((tail,) if i > last else ()):
            cnt["insts"] += 1
            if c:
                cnt["valu"] += 1
                cnt[c] += 1
            if o == "s_nop":
                cnt["s_nop"] += 1
            if o.startswith(("buffer_store", "global_store", "flat_store")):
                cnt["vstore"] += 1
            if o.startswith("s_and_saveexec") or o.startswith("s_or_saveexec"):
                cnt["saveexec"] += 1
    return whole, tail


def report(flt="", defines=()):
    src = ROOT / "omniparser_amd" / "csrc" / "gemm_dma.hip"
    with tempfile.TemporaryDirectory() as td:
        subprocess.run([HIPCC, *FLAGS, *defines, "--save-temps", "-c", str(src), "-o", str(Path(td) / "o.o")], cwd=td, check=True,
                       capture_output=True)
        asm = next(Path(td).glob("*gfx950*.s")).read_text().split("\n")
    rows = []
    for st in (i for i, l in enumerate(asm) if re.match(r"^_Z\w+:", l)):
        en = next((i for i in range(st, len(asm)) if ".end_amdhsa_kernel" in asm[i]), None)
        if en is None:
            continue
        body = asm[st:en]
        meta = {m.group(1): int(m.group(2)) for l in body
                if (m := re.match(r"\s*\.amdhsa_(next_free_vgpr|group_segment_fixed_size|private_segment_fixed_size)\s+(\d+)", l))}
        rows.append((asm[st].split(":")[0], meta, census(body)))
    out = []
    for (name, meta, (whole, tail)), dn in zip(rows, demangle([r[0] for r in rows])):
        short = re.sub(r"\(anonymous namespace\)::", "", dn).split("(")[0].replace("void ", "")
        if not ("gemm_dma_kernel" in short or "mlp_fused_kernel" in short) or (flt and flt not in short):
            continue
        regs = meta.get("next_free_vgpr", 0)
        out.append(f"{short}\n    regs {regs} (waves/SIMD {waves_per_simd(regs)})  scratch {meta.get('private_segment_fixed_size', 0)} B  "
                   f"LDS {meta.get('group_segment_fixed_size', 0)} B")
        for tag, c in (("whole kernel   ", whole), ("after last MFMA", tail)):
            out.append(f"    {tag}: insts {c['insts']:5d}  VALU {c['valu']:5d} = " + "  ".join(f"{k} {c[k]}" for k in CLASSES) +
                       f"  | s_nop {c['s_nop']}  vector stores {c['vstore']}  saveexec {c['saveexec']}")
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    defs = [a for a in args if a.startswith("-D")]
    rest = [a for a in args if not a.startswith("-D")]
    for line in report(rest[0] if rest else "", defs):
        print(line)

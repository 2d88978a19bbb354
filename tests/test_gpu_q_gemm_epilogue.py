"""`-m gpu`: the epilogues of csrc/gemm_dma.hip (`gemm_epilogue`, the chunk epilogue of `mlp_fused_kernel`) after their instruction
count was cut: bias as one fma, one-branch packed GELU, format-B low half by a mixed fma, and stores / residual loads through
tile-relative buffer descriptors whose range check replaces the per-row compare.  Small shapes on every tile configuration: a full
tile plus a 44-row tail (M = 300), a tile that is all tail (M = 37), one and sixteen K slices, channel slices of wider buffers (a
descriptor that is too long would overwrite the 7.0 guard columns `check_gemm_dma` asserts), all five epilogue variants; the
criterion is that check's own 2e-6 against the f64 product of the decoded operands."""
import ctypes
import math
import os

import pytest
import torch

from omniparser_amd import _lib as L

pytestmark = pytest.mark.gpu

TILES = ("256x256", "256x128", "128x128")
# (residual, activation, format-B output)
VARIANTS = {
    "none": (False, L.ACT_NONE, False),
    "residual": (True, L.ACT_NONE, False),
    "split": (False, L.ACT_NONE, True),
    "gelu_split": (False, L.ACT_GELU, True),
    "gelu": (False, L.ACT_GELU, False),
}


def _cases(variant):
    res, act, osplit = VARIANTS[variant]
    out = []
    for M in (300, 37):
        for K in (64, 512):
            for N in (256, 512):
                for sliced in (False, True):
                    # M, K, N, in_ld, in_off, out_ld, out_off, res, act, out_split
                    out.append((M, K, N, K + 32, 16, N + 48, 16, res, act, osplit) if sliced else (M, K, N, K, 0, N, 0, res, act, osplit))
    return out


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_gemm_dma_epilogue_variants(variant):
    import gpu_checks as G
    r = G.check_gemm_dma(cases=_cases(variant), tiles=TILES)
    print(variant, "worst rel err %.3e over %d launches" % (r["worst_rel_err"], r["cases"]))
    assert r["cases"] == 16 * len(TILES) and r["worst_rel_err"] < 2e-6, r


def test_mlp_fused_tails():
    import gpu_checks as G
    r = G.check_mlp_fused()
    print("mlp_fused worst rel err %.3e, vs two launches %.3e" % (r["worst_rel_err"], r["worst_vs_two_launches"]))
    assert r["cases"] == 4, r


class _HipBuffer:
    """a HIP allocation of its own (not the caching allocator's segment): the byte after it belongs to nobody"""

    def __init__(self, nbytes):
        self.hip = ctypes.CDLL("libamdhip64.so")
        self.hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
        self.hip.hipFree.argtypes = [ctypes.c_void_p]
        self.hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        p = ctypes.c_void_p()
        assert self.hip.hipMalloc(ctypes.byref(p), nbytes) == 0
        self.ptr, self.nbytes = p.value, nbytes

    def write(self, t):          # device tensor -> the whole allocation
        assert t.numel() * t.element_size() == self.nbytes
        assert self.hip.hipMemcpy(self.ptr, t.data_ptr(), self.nbytes, 3) == 0

    def read(self):
        t = torch.empty(self.nbytes, dtype=torch.uint8, device="cuda")
        assert self.hip.hipMemcpy(t.data_ptr(), self.ptr, self.nbytes, 3) == 0
        return t.cpu()

    def free(self):
        self.hip.hipFree(self.ptr)


def _clone_op(op, **kw):
    c = L.OmniOp()
    ctypes.memmove(ctypes.byref(c), ctypes.byref(op), ctypes.sizeof(c))
    for k, v in kw.items():
        c.p[int(k[1:])] = v
    return c


def test_output_ending_with_its_allocation():
    """The rows of a tile beyond M are not written: (a) guard ROWS behind the output keep their fill, then (b) the same ops with the
    output's last row ending exactly where a HIP allocation ends — the pointer validation accepts them and the bytes equal those of
    (a).  GEMM (plain, GELU + format B, in-place residual) on a forced 256x256 tile with a 44-row tail and on an all-tail 128x128
    tile, and the fused FFN with a 33-row block."""
    from omniparser_amd.planner import PlanBuilder, View
    g = torch.Generator().manual_seed(3)
    GUARD = 256
    jobs = []
    for M, tile in ((300, "256x256"), (37, None)):
        for name in ("none", "gelu_split", "residual"):
            jobs.append(("gemm", M, tile, name))
    jobs.append(("mlp", 33, None, None))
    for kind, M, tile, name in jobs:
        pb = PlanBuilder("cuda", L.F32)
        if kind == "gemm":
            K, N = 64, 256
            use_res, act, osplit = VARIANTS[name]
            x = torch.randn(M, K, generator=g)
            xv = View(x.view(1, M, 1, K).to("cuda"), 0, K)
            pb.split_convert(xv)
            init = torch.randn(M, N, generator=g) if use_res else torch.full((M, N), 7.0)
            w = pb.pack_weight_dma(torch.randn(N, K, generator=g) / math.sqrt(K))
            b = torch.randn(N, generator=g)
            big = torch.cat([init, torch.full((GUARD, N), 7.0)]).to("cuda")          # M rows of output + guard rows
            ov = View(big[:M].view(1, M, 1, N), 0, N)
            pb.conv(xv, w, b, ov, 1, act=act, res=ov if use_res else None, out_split=osplit)
        else:
            K, N = 128, 128
            x = torch.randn(M, K, generator=g)
            xv = View(x.view(1, M, 1, K).to("cuda"), 0, K)
            pb.split_convert(xv)
            init = torch.randn(M, N, generator=g)
            big = torch.cat([init, torch.full((GUARD, N), 7.0)]).to("cuda")
            ov = View(big[:M].view(1, M, 1, N), 0, N)
            w1, w2 = pb.pack_weight_dma(torch.randn(512, K, generator=g) / math.sqrt(K)), pb.pack_weight_dma(torch.randn(N, 512, generator=g) / 22.0, kperm=True)
            pb.mlp_fused(xv, w1, pb.upload(torch.randn(512, generator=g) * 0.5), w2, pb.upload(torch.randn(N, generator=g)), ov, ov)
        op = pb.ops[-1]
        if tile:
            os.environ["OMNI_GEMM_TILE"] = tile
        try:
            L.launch(pb.ops[0])
            L.launch(op)
            torch.cuda.synchronize()
            got = big.cpu()
            assert (got[M:] == 7.0).all(), f"{kind} {name} M={M} tile {tile}: rows beyond M were written"
            assert not (got[:M] == init).all(), "the op did not write its output"
            # (b) the output (and the in-place residual) at the very end of an allocation of its own
            nbytes = M * N * 4
            buf = _HipBuffer((4 << 20))
            try:
                pre = torch.full(((4 << 20) // 4,), 7.0)
                pre[-M * N:] = init.flatten()
                buf.write(pre.to("cuda"))
                end = buf.ptr + buf.nbytes - nbytes
                uses_res = kind == "mlp" or VARIANTS[name][0]
                L.launch(_clone_op(op, p4=end, **({"p3": end} if uses_res else {})))      # raises OmniError if the validation refuses it
                torch.cuda.synchronize()
                back = buf.read()
            finally:
                buf.free()
        finally:
            os.environ.pop("OMNI_GEMM_TILE", None)
        assert torch.equal(back[-nbytes:], got[:M].contiguous().view(torch.uint8).flatten()), f"{kind} {name} M={M}: output at the end of an allocation differs"
        assert (back[:-nbytes].view(torch.float32) == 7.0).all(), f"{kind} {name} M={M}: bytes in front of the output were written"

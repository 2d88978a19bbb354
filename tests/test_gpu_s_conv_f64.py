"""`-m gpu`: every instantiation of the convolution kernels (csrc/conv_igemm.hip) inside guard bands against a float64 convolution,
per output pixel (tests/conv_f64.py).  Forced-tile cases of a few hundred rows reach every (BM, BN, RB, loader) the launcher can pick —
each case asserts through omni_debug_conv_cfg that it lands where it says, and the union over a family's cases must equal the reach of
the launcher's heuristic over the debug query's sweep.  One large unforced case per 128-row tile keeps the heuristic's own path
exercised, plus the detector's first layer (3x3 over 4 stored channels) on the 128x64 generic-loader kernel it runs at the benched
input.  Under the OMNI_EMU=1 rehearsal the large cases are beyond the host emulation and skip by their own size guard."""
import pytest

import conv_f64 as C

pytestmark = pytest.mark.gpu
LAUNCHES = {"f32": 57, "f16": 57, "split": 36}


@pytest.mark.parametrize("fam", ["f32", "f16", "split"])
def test_every_conv_instantiation_inside_guard_bands(fam):
    cases = C.split_cases() if fam == "split" else C.typed_cases(fam)
    r = C.run_cases(cases)
    for key, cout in (("worst", 40), ("worst_one", 1)):
        print(f"MEASURED {fam} {key}: pixel error {r[key][0]:.3e} [{r[key][1]} at {r[key][2]}]; bound {C.bound(fam, cout):.1e}")
    assert r["launched"] == len(cases) == LAUNCHES[fam]
    reachable = C.sweep(fam)
    print(f"{fam}: reachable {sorted(reachable)}\n{fam}: launched  {sorted(r['instantiations'])}")
    assert r["instantiations"] == reachable, (sorted(reachable - r["instantiations"]), sorted(r["instantiations"] - reachable))
    assert r["reduce"] == ({"none", "reduce_launch", "in_launch_combine"} if fam == "split" else {"none", "reduce_launch"})


@pytest.mark.parametrize("fam,n", [("f32", 0), ("f32", 1), ("f32", 2), ("f16", 0), ("f16", 1), ("split", 0), ("split", 1)])
def test_unforced_heuristic_large_case(fam, n):
    import gpu_checks as G
    c = C.large_cases(fam)[n]
    if G.DEV == "cpu" and C.case_cost(c) > C.EMU_LIMIT:
        pytest.skip("beyond the host emulation (rehearsal): runs on the MI355X")
    e, loc, whole, cfg = C.run_case(c, seed=100 + n)
    print(f"MEASURED {fam} large case {n}: pixel error {e:.3e} at {loc}, whole-tensor {whole:.3e}, {cfg}")
    assert cfg["splits"] == 1

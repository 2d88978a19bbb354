"""tests/conv_f64.py on the host emulation of the kernels (tests/emu): the forced-tile small shapes of every conv instantiation inside
guard bands against the float64 convolution, per output pixel.  The same functions run on the MI355X in tests/test_gpu_s_conv_f64.py,
which adds the large unforced cases; this module prints the worst pixel error per family as the emulation measures it."""
import pytest

import conv_f64 as C

LAUNCHES = {"f32": 57, "f16": 57, "split": 36}


@pytest.mark.parametrize("fam", ["f32", "f16", "split"])
def test_every_conv_instantiation_inside_guard_bands(emu, fam):
    cases = C.split_cases() if fam == "split" else C.typed_cases(fam)
    r = C.run_cases(cases)
    for key, cout in (("worst", 40), ("worst_one", 1)):
        print(f"MEASURED (host emulation) {fam} {key}: pixel error {r[key][0]:.3e} [{r[key][1]} at {r[key][2]}]; bound {C.bound(fam, cout):.1e}")
    assert r["launched"] == len(cases) == LAUNCHES[fam]
    reachable = C.sweep(fam)
    print(f"{fam}: launched {sorted(r['instantiations'])}")
    assert r["instantiations"] == reachable, (sorted(reachable - r["instantiations"]), sorted(r["instantiations"] - reachable))
    assert r["reduce"] == ({"none", "reduce_launch", "in_launch_combine"} if fam == "split" else {"none", "reduce_launch"})

"""The resident-weights form of conv_spq_kernel (conv_spq.hip, RES = 1) keeps 128 registers of weights per lane at two
waves per SIMD: 256 registers in all.  It fits only because its epilogue re-reads the affine per accumulator tile
(`aff_of_tile`, an offset the compiler cannot see through); a compiler that keeps those values live again puts the form
into scratch, which no result would show.  This compiles the unit for gfx950 with hipcc's resource remarks
(tools/kernel_resources.py, no GPU) and holds the form to what the issue set: no scratch at __launch_bounds__(256, 2)."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_resident_form_has_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    rows = {re.sub(r"\(anonymous namespace\)::|\(.*$|void ", "", name): f for name, f in kernel_resources.resources("conv_spq")}
    res = [f for name, f in rows.items() if re.fullmatch(r"conv_spq_kernel<32, 0, 0, 0, 1>", name)]
    assert len(res) == 1, sorted(rows)
    f = res[0]
    print("conv_spq_kernel<32, 0, 0, 0, 1>:", {k: f.get(k) for k in ("VGPRs", "AGPRs", "VGPRs Spill", "ScratchSize [bytes/lane]",
                                                                     "Occupancy [waves/SIMD]")})
    assert int(f["ScratchSize [bytes/lane]"]) == 0 and int(f["VGPRs Spill"]) == 0, f
    assert int(f["VGPRs"]) + int(f["AGPRs"]) <= 256 and int(f["Occupancy [waves/SIMD]"]) >= 2, f

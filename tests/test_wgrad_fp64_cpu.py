"""tests/wgrad_fp64.py on the CPU: the faithful emulation of the weight-gradient kernels passes the bound on every case,
every mutant fails it on the cases meant to catch it, the yardstick table is what `python -m tests.wgrad_fp64` measures,
and every case's claimed plan is what the library's own make_plan / make_plan_sp give (dn_conv_wgrad_plan: host only)."""
import pytest

from tests import wgrad_fp64 as W

RUN = [c for c in W.CASES if not c.refuse]


@pytest.mark.parametrize("case", RUN, ids=lambda c: c.name)
def test_emulation_passes_and_mutants_fail(case):
    ref, c = W.reference(case), W.c_of(case)
    r = W.worst(W.emulate(case), ref, c)
    assert r <= 1.0, (r, W.breakdown(W.emulate(case), ref, c, case.c0))
    # the emulation of the kernels' own chain needs no yardstick beyond the float32 one (no E32 here)
    assert W.worst(W.emulate(case), ref, 1.0) <= W.MARGIN * W.YARD[W.family_of(case)] + (W.P24 if case.accumulate else 0.0) or \
        case.vals == "zero"
    for mutant in W.MUTANTS:
        if W.targets(mutant, case):
            r = W.worst(W.emulate(case, mutant), ref, c)
            assert r > 1.0, (mutant, r)


def test_every_mutant_has_cases_on_every_engine_it_applies_to():
    for mutant in W.MUTANTS:
        engines = {c.eng for c in RUN if W.targets(mutant, c)}
        want = {"sp"} if mutant in ("drop_lo_hi", "drop_hi_lo", "scale_dz_only") else {"f32", "sp"}
        assert engines == want, (mutant, engines)


@pytest.mark.parametrize("family", sorted(W.YARD))
def test_yardstick_table_is_what_the_module_measures(family):
    got = W.measure_yard(family)
    assert W.YARD[family] / 2 <= got <= W.YARD[family] * 2, (family, got)


def _plan(case):
    from disconet_amd import ops, train_ops
    return train_ops.conv_wgrad_plan(W.desc_of(case, ops.conv_desc), sp=case.eng == "sp")


@pytest.mark.parametrize("case", W.CASES, ids=lambda c: c.name)
def test_claimed_plan_is_the_librarys(case):
    plan = _plan(case)
    claim = case.plan_claim()
    assert {k: plan[k] for k in claim} == claim
    assert plan["tiles_x"] * plan["tiles_y"] * case.n == plan["n_tiles"] and (plan["tiles_x"], plan["tiles_y"]) == W.tiles_of(case)
    assert plan["n_cot"] == -(-case.c_out // case.ct) and plan["n_cit"] == -(-case.c0 // case.ct) + -(-case.c1 // case.ct)
    if case.lens is not None:
        assert W.slice_lengths(plan["n_tiles"], plan["n_slices"]) == case.lens


def test_the_case_list_reaches_every_form_and_every_residue_of_the_reduction():
    assert {c.form for c in RUN} == set(W.FORMS)
    for form in ("F32-3x3s1", "F64"):
        assert {c.n_slices % 8 for c in RUN if c.form == form} == set(range(8))
    for form in ("SP32s1", "SP64s1"):
        assert {1, 2, 3, 5, 7, 8, 16} <= {c.n_slices for c in RUN if c.form == form}
    # one case per engine where 512 / blocks, not n_tiles / 4, sets the slice count
    for eng in ("f32", "sp"):
        assert any(c.n_tiles // 4 > c.n_slices == 512 // (-(-c.c_out // c.ct) * -(-c.c0 // c.ct)) for c in RUN if c.eng == eng)


def test_refused_cases_are_refused_for_their_layout_not_for_a_null_pointer():
    refused = [c for c in W.CASES if c.refuse]
    assert refused
    for c in refused:
        spec = W.arg_spec(c)
        assert all(given for name, (given, _) in spec.items() if name != "src1") and spec["src1"][0] == (c.c1 > 0)
        assert sum(1 for given, off in spec.values() if given and off) == 1          # exactly one operand off 16 bytes
        assert all(ld % 4 == 0 for ld, ch in zip(c.ld, (c.c0, c.c1, c.c_out)) if ch)   # rows of 4 k floats: only the base is off

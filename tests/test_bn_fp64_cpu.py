"""tests/bn_fp64.py on the CPU: the faithful emulation of the BatchNorm training kernels passes the bound on every case, every
mutant fails it on the cases that name it and is named by a case, the reference's own mask bits stay within the cap of free
bits, a case's claimed kernel class is what the library's shape rule gives (dn_bn_train_form_supported: host only), every
kernel of the unit's BatchNorm half -- read from train_ops.hip -- is named by a case, and the yardstick table is what the
module measures."""
import pytest

from tests import bn_fp64 as B

RUN = [k for k in B.CASES if not k.refuse]


@pytest.mark.parametrize("case", RUN, ids=lambda k: k.name)
def test_emulation_passes_and_mutants_fail(case):
    outs = B.emulate(case)
    r = B.judge(case, outs)
    assert r and max(r.values()) <= 1.0, r
    if case.kind == "stats":
        assert float(outs["var"].min()) >= 0.0
    if case.kind == "apply" and case.mask:
        assert B.mask_free_share(case) <= B.MASK_FREE_CAP
    if case.vals == "gate" and case.kind == "bwd":
        assert not bool(outs["dz"][..., :3].any()) and not bool(B.reference(case)["dz"].y[..., :3].any())
    if case.heavy:
        return
    for mutant in case.catches:
        r = B.judge(case, B.emulate(case, mutant))
        assert max(r.values()) > 1.0, (mutant, r)


def test_every_mutant_is_named_by_a_case():
    named = {m for k in RUN for m in k.catches}
    assert named == set(B.MUTANTS), set(B.MUTANTS) ^ named
    # the reductions' mutants on both reductions, on the scalar and on the float4 kernels
    for mutant in ("last_chunk", "group0"):
        assert {(k.kind, k.V) for k in RUN if mutant in k.catches} >= {("stats", 1), ("stats", 4), ("bwd", 1), ("bwd", 4)}, mutant
    assert {k.kind for k in RUN if "u_tail" in k.catches} == {"stats", "bwd"}
    assert {k.kind for k in RUN if "mask_bits" in k.catches} == {"apply", "bwd"}


def test_the_sq32_mutant_is_the_parents_rule_and_misses_the_bound_by_orders_of_magnitude():
    for k in RUN:
        if "sq32" in k.catches:
            assert B.judge(k, B.emulate(k, "sq32"))["var"] > 10.0
            assert B.judge(k, B.emulate(k))["var"] <= 1.0


def test_every_kernel_of_the_batchnorm_half_is_named_by_a_case():
    assert {n.split("<")[0] for n in B.BN_KERNELS} == B.kernels_in_source()
    named = {n for k in RUN for n in k.kernels()}
    assert named <= set(B.BN_KERNELS)
    assert set(B.BN_KERNELS) - named == set(B.LEGACY_KERNELS)


def test_claimed_class_is_the_librarys_shape_rule():
    from disconet_amd import train_ops
    lib = train_ops._lib.load()
    for k in B.CASES:
        if k.kind == "running":
            continue
        fast = bool(lib.dn_bn_train_form_supported(train_ops.BN_FORM_BIAS, k.groups, k.rpg, k.c))
        assert (k.cls == "fast") == (fast and k.aligned), k.name
        if k.sp and k.kind == "apply":
            assert lib.dn_bn_train_form_supported(train_ops.BN_FORM_SP_APPLY, k.groups, k.rpg, k.c) == 1
        if not k.want_dz:
            assert lib.dn_bn_train_form_supported(train_ops.BN_FORM_DZ_NULL, k.groups, k.rpg, k.c) == 1
        if k.bias:
            assert k.cls == "fast"
        if k.cls != "fast":
            assert k.cls == ("vec4" if k.c % 4 == 0 and k.aligned else "general")


def test_the_case_list_reaches_the_edges_it_claims():
    by = {k.name: k for k in B.CASES}
    s7 = by["stats:S7-trailing-wg-owns-no-rows"]
    chunk = -(-s7.rpg // s7.nblk)
    assert (s7.nblk, chunk) == (128, 65) and (s7.nblk - 1) * chunk >= s7.rpg and s7.rpg - (s7.nblk - 2) * chunk == 3
    assert by["stats:S8a-576-partials"].nblk == 576 and by["stats:S8b-1024-partials"].nblk == 1024
    assert by["stats:S5-ty4-chunk65"].nblk == 5 and by["stats:S4-float4-10wg"].nblk == 10
    assert by["stats:S6-cvn65"].c // 4 == 65
    assert by["stats:S3-c16-misaligned"].cls == "general" and by["bwd:c16-misaligned-dy_a-mask"].cls == "general"
    assert by["bwd:sp-vec4-c48"].cls == "vec4" and by["bwd:sp-vec4-c48"].kernels()[-1] == "bn_bwd_apply_v4_kernel<true>"
    wrap = by["apply:fast-grid-wrap"]
    assert wrap.total // 4 > 8192 * 256 and wrap.heavy
    bw = by["bwd:bias-grid-wrap"]
    assert bw.total // 4 > 1024 * 256
    assert {k.shape[0] for k in B.CASES if k.kind == "running" and not k.order} >= {1, 7, 8, 9, 17}
    assert {k.groups for k in B.CASES if k.kind == "bwd"} >= {1, 9, 16}
    assert len(B.fold_jobs_inputs()) + 1 > 32


def test_yardstick_table_is_what_the_module_measures():
    got = B.measure_yard()
    assert set(got) == set(B.YARD)
    for fam, v in got.items():
        assert abs(v - B.YARD[fam]) <= 1e-3 * B.YARD[fam], (fam, v, B.YARD[fam])

"""First fit strands a partition whose id goes through the caller's id list (part_id_off >= 0): the record names the id, in
every workgroup that runs first fit — inside the fill workgroup, kas_p4_kernel, the second wavefront of
kas_p4_order_kernel, kas_spread_p4_kernel.  Emulator and GPU over the same batches (tests/first_fit_batches.py)."""
import pytest

from kafka_assigner_amd import abi
from first_fit_batches import solved
from parity_util import assert_same_outputs

SPREAD = abi.KAS_PLAN_SPREAD_FILL
FORMS = {"A": (abi.KAS_PLAN_FILL_WITH_P4, abi.KAS_PLAN_SPLIT_P4, abi.KAS_PLAN_P4_WITH_ORDER, SPREAD),
         "B": (abi.KAS_PLAN_FILL_WITH_P4, abi.KAS_PLAN_SPLIT_P4, abi.KAS_PLAN_P4_WITH_ORDER)}   # (the spread fill: single-topic scenarios)


@pytest.mark.parametrize("name", ["A", "B"])
def test_emu_first_fit_reports_stranded_partitions_under_the_callers_ids(name):
    from emu_lib import emu_solve, last_p4_order, last_split_p4, last_spread
    fb, want = solved(name)
    for flags in FORMS[name]:
        assert_same_outputs(fb, want, emu_solve(fb, flags=flags), f"emu, sparse partition ids, batch {name}, plan flags {flags:#x}")
        ran = (last_split_p4(), last_p4_order(), last_spread())    # kas_p4_kernel, kas_p4_order_kernel, scenarios the spread fill solved
        if flags == abi.KAS_PLAN_FILL_WITH_P4:
            assert ran == (0, 0, 0), ran
        elif flags == abi.KAS_PLAN_SPLIT_P4:
            assert ran == (1, 0, 0), ran
        elif flags == abi.KAS_PLAN_P4_WITH_ORDER:
            assert ran[1:] == (1, 0), ran
        else:
            assert ran[2] == fb.n_scenarios, ran


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "B"])
def test_hip_first_fit_reports_stranded_partitions_under_the_callers_ids(name):
    from kafka_assigner_amd import native
    fb, want = solved(name)
    ctx = native.default_context()
    for flags in FORMS[name]:
        plan = native.Plan(ctx, fb)
        plan.set_flags(flags)
        what = plan.describe()
        plan.close()
        if flags == abi.KAS_PLAN_FILL_WITH_P4:
            assert "kas_p4_kernel" not in what and "kas_p4_order_kernel" not in what and "kas_spread_" not in what, what
        else:
            needle = {abi.KAS_PLAN_SPLIT_P4: "+ kas_p4_kernel<3>", abi.KAS_PLAN_P4_WITH_ORDER: "kas_p4_order_kernel<3>", SPREAD: "kas_spread_{a,q,b,p4}_kernel<3>"}[flags]
            assert needle in what, (hex(flags), what)
        assert_same_outputs(fb, want, native.solve_host_with_flags(fb, flags, ctx), f"hip, sparse partition ids, batch {name}, plan flags {flags:#x}")

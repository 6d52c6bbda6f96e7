"""The plan's change points (tests/plan_edges.py), on the CPU: the pinned table against the planner, and the kernel source on the
emulator against the oracle at both sides of every edge and at every ceiling — the broker counts at which a packed field, a 16-bit
LDS offset or an LDS carve-up holds its last valid value.  tests/test_hip_plan_edges.py runs the same cases on the MI355X."""
import re

import pytest

import emu_lib
import plan_edges as pe
from kafka_assigner_amd import abi
from parity_util import assert_same_outputs

FAMILY_NAMES = list(pe.FAMILIES)
EDGE_CASES = [(f, n) for f in FAMILY_NAMES for n in pe.EDGES[f][0]]


@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_the_planner_changes_its_description_exactly_at_the_pinned_broker_counts(family):
    """a threshold of kas_plan_math.h / kas_launch_plan.h that moves shows here, and becomes a deliberate edit of plan_edges.EDGES"""
    assert pe.find_edges(family) == pe.EDGES[family]


@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_the_cases_of_a_family_count_what_they_claim(family):
    """From the oracle's solve and the planner alone, before any kernel runs: every case has a scenario that solves and moves
    replicas, the family has a scenario that fails first fit, and a case's plan is the probe's at its broker count (so the two
    cases of an edge are solved by the two plans the edge lies between)."""
    f = pe.FAMILIES[family]
    for n in pe.sides(family):
        pe.assert_case_counts(family, n)
        rc, text = emu_lib.describe(pe.case(family, n), f.flags, f.cells16)
        assert (rc, pe.normalised(text)) == pe.probe(family, n), (family, n, text)
    assert pe.first_fit_failures(family) >= 1, family
    for n in pe.EDGES[family][0]:
        assert pe.probe(family, n) != pe.probe(family, n + 1), (family, n)


def _emu(family, n):
    f = pe.FAMILIES[family]
    solve = emu_lib.emu_solve16 if f.cells16 else emu_lib.emu_solve
    return solve(pe.case(family, n), flags=f.flags, p4_by_batch_size=True)      # (first fit where the product runs it for two scenarios)


@pytest.mark.parametrize("family,n", EDGE_CASES, ids=[f"{f}-{n}" for f, n in EDGE_CASES])
def test_emu_equals_oracle_on_both_sides_of_an_edge(family, n):
    for m in (n, n + 1):
        fb = pe.case(family, m)
        assert_same_outputs(fb, pe.reference(family, m), _emu(family, m), f"emu {family}, {m} brokers")


@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_emu_equals_oracle_at_the_ceiling_and_refuses_one_broker_more(family):
    """at the ceiling the last node's block ends on the last byte of the LDS allocation (or 16 bytes before it); one broker more is
    refused when the plan is made — by kas_shape_batch, whose text names the LDS, and by the solve with the same code"""
    f = pe.FAMILIES[family]
    ceiling = pe.EDGES[family][1]
    fb = pe.case(family, ceiling)
    rc, text = emu_lib.describe(fb, f.flags, f.cells16)
    assert rc == 0, text
    if not f.ctx:                                            # (with a Context the stand-by round form is what fills the LDS; the text does not size it)
        assert max(int(v) for v in re.findall(r"lds=(\d+)", text)) in (163840, 163824), text
    assert_same_outputs(fb, pe.reference(family, ceiling), _emu(family, ceiling), f"emu {family}, ceiling of {ceiling} brokers")
    over = pe.case(family, ceiling + 1)
    rc, _, err = emu_lib.plan_shape(over)
    assert rc == abi.KAS_E_UNSUPPORTED and "LDS" in err, (rc, err)
    assert emu_lib.describe(over, f.flags, f.cells16)[0] == abi.KAS_E_UNSUPPORTED
    with pytest.raises(RuntimeError, match=r"rc=%d: .*LDS" % abi.KAS_E_UNSUPPORTED):
        _emu(family, ceiling + 1)


def test_three_ceilings_are_launches_that_end_on_the_last_bytes_of_the_allocation():
    """the fill kernel at RF 3, the wide ticket form at RF 5 and the round form at RF 8 are what fills the LDS at its family's ceiling"""
    want = {"rf3": ("kas_fill_kernel<3,1>[sweeps]", 163840), "rf5": ("kas_order_wide_kernel<5>", 163824),
            "rf8": ("kas_order_round_kernel<8>", 163824)}
    for family, (kernel, lds) in want.items():
        rc, text = emu_lib.describe(pe.probe_batch(family, pe.EDGES[family][1]))
        assert rc == 0 and re.search(re.escape(kernel) + r" grid=\d+x\d+ lds=%d\b" % lds, text), text
    assert all(pe.EDGES[f][1] < pe.N_LIMIT for f in FAMILY_NAMES)

"""Packed rounds on the GPU over crafted move lists (tests/crafted_cases.py: three tiles and a narrower topic, exactly as many
rounds as KAS_ROUND_WINDOW holds and one more, twice that and one more, round words whose `used` bits are all ones at 16 and 17
round bits, the node limit and the plan's broker ceilings), through kas_rounds_device / 16 over tables the test wrote itself
(tests/crafted_device.py), against the checker (tests/rounds_ref.py).  tests/test_rounds_cpu.py runs the same cases on the emulator.
"""
import pytest

import crafted_cases as CC
import crafted_device as CD
from kafka_assigner_amd import native
from rounds_ref import assert_same_rounds, check_invariants

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return native.DeviceContext(0)


@pytest.mark.parametrize("run", CC.runs(CC.ROUND_CASES), ids=CC.run_id)
def test_crafted_rounds(ctx, run):
    """every case under each of its caps and strides on one plan: the records and round_of against the checker's, the guard
    records behind the arrays untouched, a second call the same bytes; a shape no plan takes is refused as the case table says"""
    name, cells16 = run
    case = CC.rounds_case(name)
    why = CC.plan_refusal(name, case, cells16)
    if why:
        CD.assert_plan_refuses(ctx, case, cells16, why, run)
        return
    wants = case.wants(cells16)
    d = CD.device_tables(ctx, case, cells16)
    try:
        for caps, w in zip(case.caps, wants):
            want = case.listed(w)
            check_invariants(w, caps, what=(run, caps))
            for rs, ms in case.strides_for(w):
                scen, recs, rof = CD.run_rounds(d, caps, case.select, rs, ms, (run, caps, rs, ms))
                assert_same_rounds(want, scen, recs, rs, rof, ms, fill=CD.FILL, what=(run, caps, rs, ms))
    finally:
        d.plan.close()

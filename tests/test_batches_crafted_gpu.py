"""Execution batches on the GPU over crafted move lists (tests/crafted_cases.py: groups of KAS_BATCH_GROUP moves and their replay,
the queue's remainder behind a tile, a cap exceeded only by a lane of wavefront 1, 2 or 3, many closes in one group, max_moves, the
node limit and the plan's broker ceilings), through kas_batches_device / 16 over tables the test wrote itself
(tests/crafted_device.py), against the checker (tests/batches_ref.py).  tests/test_batches_cpu.py runs the same cases on the emulator.
"""
import pytest

import crafted_cases as CC
import crafted_device as CD
from batches_ref import assert_same_batches, check_invariants
from kafka_assigner_amd import native

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return native.DeviceContext(0)


@pytest.mark.parametrize("run", CC.runs(CC.BATCH_CASES), ids=CC.run_id)
def test_crafted_batches(ctx, run):
    """every case under each of its caps on one plan: the records against the checker's, the guard records behind the arrays
    untouched, a second call the same bytes; a shape no plan takes is refused as the case table says"""
    name, cells16 = run
    case = CC.batches_case(name)
    why = CC.plan_refusal(name, case, cells16)
    if why:
        CD.assert_plan_refuses(ctx, case, cells16, why, run)
        return
    wants = case.wants(cells16)
    d = CD.device_tables(ctx, case, cells16)
    try:
        for caps, w in zip(case.caps, wants):
            want = case.listed(w)
            stride = w.record["n_batches"] + 2
            scen, recs = CD.run_batches(d, caps, case.select, stride, (run, caps))
            assert_same_batches(want, scen, recs, stride, fill=CD.FILL, what=(run, caps))
            check_invariants(w, caps, what=(run, caps))
    finally:
        d.plan.close()

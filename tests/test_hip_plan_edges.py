"""The plan's change points (tests/plan_edges.py) on the MI355X: at both sides of every edge and at every ceiling the library's plan
is the one the emulator's resolver describes — LDS bytes and grids included, so the launches bisected on the CPU are the ones
issued — and its solve equals the oracle's; one broker past a ceiling the plan is refused before anything is launched; at the four
ceilings without a Context the decision passes (impact, racks, choice, front with moves) run on the same batch against their
checkers.  What hipFuncSetAttribute or a launch of 163,840 B of LDS refuses only shows here: the emulator cannot see it."""
import pytest

import emu_lib
import plan_edges as pe
from choose_ref import assert_same_choice, choose_ref
from front_ref import assert_same_front, front_choice_ref
from impact_ref import assert_same_impact, impact_ref
from kafka_assigner_amd import abi, native
from moves_ref import assert_same_moves, moves_ref
from parity_util import assert_same_outputs
from rack_ref import assert_same_racks, check_identities, rack_ref
from test_front_cpu import _spec
from test_racks_cpu import rack_per_node

pytestmark = pytest.mark.gpu

FAMILY_NAMES = list(pe.FAMILIES)
EDGE_CASES = [(f, n) for f in FAMILY_NAMES for n in pe.EDGES[f][0]]
DECISION_CEILINGS = ["rf3", "rf3_sparse", "rf5", "rf8"]
RESULT_FIELDS = ("status", "fail_topic", "fail_partition", "moved_replicas", "moved_partitions", "digest")
KEYS = ("max_inbound", "moved_replicas")


@pytest.fixture(scope="module")
def ctx():
    return native.DeviceContext(0)


@pytest.fixture(scope="module", autouse=True)
def resolver():
    """the emulator build of the launch resolver, which the plan texts are held to: on a fresh checkout it is compiled here, once
    (g++, no GPU involved), not inside the first case"""
    emu_lib.lib()


def _plan_text(ctx, family, n):
    f = pe.FAMILIES[family]
    plan = native.Plan(ctx, pe.case(family, n), cells16=f.cells16)
    try:
        if f.flags:
            plan.set_flags(f.flags)
        return plan.describe()
    finally:
        plan.close()


def _solve(ctx, family, n):
    f = pe.FAMILIES[family]
    fb = pe.case(family, n)
    if f.cells16:
        return native.solve_host16(fb, ctx)
    return native.solve_host_with_flags(fb, f.flags, ctx) if f.flags else native.solve_host(fb, ctx)


def _check(ctx, family, n):
    f = pe.FAMILIES[family]
    fb = pe.case(family, n)
    pe.assert_case_counts(family, n)
    assert (0, _plan_text(ctx, family, n)) == emu_lib.describe(fb, f.flags, f.cells16), (family, n)
    assert_same_outputs(fb, pe.reference(family, n), _solve(ctx, family, n), f"hip {family}, {n} brokers")


@pytest.mark.parametrize("family,n", EDGE_CASES, ids=[f"{f}-{n}" for f, n in EDGE_CASES])
def test_hip_equals_oracle_on_both_sides_of_an_edge(ctx, family, n):
    for m in (n, n + 1):
        _check(ctx, family, m)


@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_hip_equals_oracle_at_the_ceiling_and_refuses_one_broker_more(ctx, family):
    f = pe.FAMILIES[family]
    ceiling = pe.EDGES[family][1]
    _check(ctx, family, ceiling)
    assert pe.first_fit_failures(family) >= 1, family                       # (some case of the family compares a failing id)
    with pytest.raises(native.KasError) as e:
        _plan_text(ctx, family, ceiling + 1)
    assert e.value.code == abi.KAS_E_UNSUPPORTED and "LDS" in e.value.detail, e.value.detail
    over = pe.case(family, ceiling + 1)
    with pytest.raises(native.KasError) as e:                               # the host call plans before it copies or launches
        native.solve_host16(over, ctx) if f.cells16 else native.solve_host(over, ctx)
    assert e.value.code == abi.KAS_E_UNSUPPORTED, e.value.detail


@pytest.mark.parametrize("family", DECISION_CEILINGS)
def test_decision_passes_at_the_ceiling(ctx, family):
    """kas_solve_host_impact, _rack_impact (the batch's racks; one rack per node, capped at KAS_RACK_LIMIT), _choose with k = S and
    _front with every kind of move, on the ceiling's batch: their LDS carve-ups depend on the largest broker count too"""
    n = pe.EDGES[family][1]
    fb, want = pe.case(family, n), pe.reference(family, n)
    S = fb.n_scenarios
    imp = impact_ref(fb, want)
    assert int(imp[0]["inbound"].sum()) > 0 and int(imp[1]["leaders_moved"].sum()) > 0     # (the passes count rows, not zeros)

    ho, nodes, scen = native.solve_host_impact(fb, ctx=ctx)
    assert_same_outputs(fb, want, ho, f"{family} ceiling: kas_solve_host_impact")
    assert_same_impact(imp, (nodes, scen), f"{family} ceiling: impact records")

    ho, rk = native.solve_host_rack_impact(fb, ctx=ctx)
    assert_same_outputs(fb, want, ho, f"{family} ceiling: kas_solve_host_rack_impact")
    assert_same_impact(imp, (rk.nodes, rk.impact), f"{family} ceiling: impact records beside the rack pass")
    got = (rk.racks, rk.scenarios, rk.rack_off)
    assert_same_racks(rack_ref(fb, want, None, nodes=imp[0]), got, f"{family} ceiling: rack records, the batch's table")
    check_identities(fb, want, imp[0], got)
    table = rack_per_node(fb)
    assert int(table.max()) + 1 == min(n, abi.KAS_RACK_LIMIT)
    _, rk2 = native.solve_host_rack_impact(fb, report_rack=table, select=[], nodes=False, ctx=ctx)
    assert_same_racks(rack_ref(fb, want, table, nodes=imp[0]), (rk2.racks, rk2.scenarios, rk2.rack_off),
                      f"{family} ceiling: rack records, one rack per node")

    sr, out = want.scenario_results, want.out
    got_ho, choice = native.solve_host_choose(fb, KEYS, S, ctx=ctx)
    assert_same_choice(choose_ref(fb, sr, out, imp, KEYS, S), choice, f"{family} ceiling: choice of k = S")
    for name in RESULT_FIELDS:
        assert (got_ho.scenario_results[name][:S] == sr[name][:S]).all(), (family, name)
    for name in abi.SCENARIO_IMPACT_FIELDS:
        assert (choice.scenarios[name] == imp[1][name]).all(), (family, name)

    got_ho, front, ml = native.solve_host_front(fb, _spec(KEYS, S), 7, ctx=ctx)
    want_front = front_choice_ref(fb, sr, out, imp, KEYS, S)
    front.counts = [front.n_ok, front.n_eligible, front.n_front, 0]
    assert_same_front(want_front, front, f"{family} ceiling: front")
    assert_same_choice(want_front, front, f"{family} ceiling: front, rows and node blocks")
    want_moves = moves_ref(fb, want, want_front.chosen, 7)
    assert int(want_moves.move_off[-1]) > 0
    assert_same_moves(want_moves, ml, f"{family} ceiling: moves of the front")
    for name in RESULT_FIELDS:
        assert (got_ho.scenario_results[name][:S] == sr[name][:S]).all(), (family, name)

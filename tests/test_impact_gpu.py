"""The impact pass on the MI355X (ABI v6: kas_impact_device / 16, kas_solve_host_impact / 16, WhatIf.solve(impact=True),
the CLI's --print_impact), against the NumPy checker of tests/impact_ref.py."""
import json
import os
import subprocess

import numpy as np
import pytest

from impact_batches import assert_exercises, replan_batches, solved, whatif_inputs
from impact_ref import assert_same_impact, check_invariants, impact_ref
from kafka_assigner_amd import abi, native
from kafka_assigner_amd import generator as G
from kafka_assigner_amd.flatten import HostOutputs, Scenario, Topic, flatten, host_tables, node_set_batch, to_cells16
from oracle_lib import oracle_solve
from test_impact_cpu import (GOLD, _failing_then_skipped_batch, _many_brokers_batch, _random_batch,
                             _shared_node_range_batch, _width_class, guarded)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESULT_FIELDS = ("status", "fail_topic", "fail_partition", "moved_replicas", "moved_partitions", "digest")


@pytest.fixture(scope="module")
def ctx():
    return native.DeviceContext(0)


def _same_solve(a, b, what):
    """records and every cell of two solves of one batch"""
    for f in RESULT_FIELDS:
        assert (a.scenario_results[f] == b.scenario_results[f]).all(), (what, f)
    for f in ("status", "fail_partition", "moved_replicas", "moved_partitions"):
        assert (a.topic_results[f] == b.topic_results[f]).all(), (what, f)
    assert np.array_equal(a.out, b.out), what


BATCHES = {"random": lambda: _random_batch(42, n_scen=6), "failing_then_skipped": _failing_then_skipped_batch,
           "shared_node_range": _shared_node_range_batch, "many_brokers": _many_brokers_batch}
CLAIMS = {"random": dict(merge=True, widths=[(2, 3), (3, 3)]), "shared_node_range": dict(must_solve=[0, 1]),
          "many_brokers": dict(must_solve=[0])}


def _guard(name, fb):
    """assert_exercises on the oracle's solve of the batch (not for the batch whose subject is failure)"""
    if name in CLAIMS:
        guarded(fb, **CLAIMS[name])


@pytest.mark.parametrize("cells16", [False, True], ids=["int32", "cells16"])
@pytest.mark.parametrize("name", list(BATCHES))
def test_host_impact_equals_checker(ctx, name, cells16):
    fb = BATCHES[name]()
    _guard(name, fb)
    if cells16:
        plain = native.solve_host16(fb, ctx)
    else:
        plain = native.solve_host(fb, ctx)
    ho, nodes, scen = native.solve_host_impact(fb, cells16=cells16, ctx=ctx)
    _same_solve(plain, ho, f"{name}: the solve with and without the impact pass")
    want = impact_ref(fb, ho, cells16=cells16)
    assert_same_impact(want, (nodes, scen), f"{name}, kas_solve_host{'16' if cells16 else ''}_impact")
    check_invariants(fb, ho, want)
    if not cells16:
        assert_same_impact(want, impact_ref(fb, oracle_solve(fb)), f"{name}: the GPU's rows against the oracle's")
    # no rows: the records and the impact only
    ho0, n0, s0 = native.solve_host_impact(fb, select=[], cells16=cells16, ctx=ctx)
    assert_same_impact(want, (n0, s0), f"{name}, n_select = 0")
    for f in RESULT_FIELDS:
        assert (ho0.scenario_results[f] == ho.scenario_results[f]).all()


def _device_impact(ctx, fb, cells16):
    """Plan + solve_device + impact_device on one torch stream: (HostOutputs, (nodes, scenarios))"""
    import torch
    dev = torch.device("cuda", ctx.device)
    plan = native.Plan(ctx, fb, cells16=cells16)
    try:
        _, ho = host_tables(fb)
        cur = to_cells16(fb).view(np.int16) if cells16 else fb.cur
        d_cur = torch.from_numpy(cur.copy()).to(dev)
        d_aux = torch.from_numpy(fb.aux).to(dev) if fb.aux.size else None
        d_out = torch.full((max(fb.out_len, 1),), -2, dtype=torch.int16 if cells16 else torch.int32, device=dev)
        d_tr = torch.zeros(max(fb.n_topics, 1) * 16, dtype=torch.uint8, device=dev)
        d_sr = torch.zeros(max(fb.n_scenarios, 1) * 32, dtype=torch.uint8, device=dev)
        n_nodes = int(native.node_blocks(fb)[-1])
        d_nodes = torch.full((max(n_nodes, 1) * 32,), 0x5A, dtype=torch.uint8, device=dev)
        d_scen = torch.full((max(fb.n_scenarios, 1) * 32,), 0x5A, dtype=torch.uint8, device=dev)
        st = torch.cuda.Stream(dev)
        st.wait_stream(torch.cuda.current_stream(dev))
        aux = d_aux.data_ptr() if d_aux is not None else 0
        plan.solve_device(d_cur.data_ptr(), d_out.data_ptr(), d_tr.data_ptr(), d_sr.data_ptr(), aux=aux, stream=st.cuda_stream)
        plan.impact_device(d_cur.data_ptr(), d_out.data_ptr(), d_tr.data_ptr(), d_nodes.data_ptr(), d_scen.data_ptr(), aux=aux,
                           stream=st.cuda_stream)
        st.synchronize()
        ho.out = d_out.cpu().numpy().view(np.uint16) if cells16 else d_out.cpu().numpy()
        ho.topic_results = d_tr.cpu().numpy().view(abi.TOPIC_RESULT_DTYPE)
        ho.scenario_results = d_sr.cpu().numpy().view(abi.SCENARIO_RESULT_DTYPE)
        nodes = d_nodes.cpu().numpy().view(abi.NODE_IMPACT_DTYPE)[:n_nodes]
        scen = d_scen.cpu().numpy().view(abi.SCENARIO_IMPACT_DTYPE)[:fb.n_scenarios]
        return ho, (nodes, scen)
    finally:
        plan.close()


@pytest.mark.parametrize("cells16", [False, True], ids=["int32", "cells16"])
@pytest.mark.parametrize("name", ["random", "failing_then_skipped", "many_brokers"])
def test_device_impact_equals_checker(ctx, name, cells16):
    fb = BATCHES[name]()
    _guard(name, fb)
    ho, got = _device_impact(ctx, fb, cells16)
    assert (got[0]["reserved"] == 0).all()
    assert_same_impact(impact_ref(fb, ho, cells16=cells16), got, f"{name}, kas_impact_device{'16' if cells16 else ''}")


# ---- the paths no other test counts a row on (impact_batches.BATCHES: small shapes, the oracle's solve shared) --------------
NAMED = ["widths_4_5", "widths_6_8", "rf_4", "rf_4_5", "rf_7_8", "sparse", "dense_and_sparse", "id_range_edge", "beyond_the_table",
         "row_counts", "degenerate", "rows_4096", "rows_4097", "rows_10000", "many_brokers_10000"]
WIDTH_CLASS = {"widths_4_5": 5, "widths_6_8": 8, "rf_4": 4, "rf_4_5": 5, "rf_7_8": 8}


@pytest.mark.parametrize("name", NAMED)
def test_host_and_device_impact_on_the_named_batches(ctx, name):
    """kas_solve_host_impact and kas_impact_device on int32 cells: lists 4-8 wide (RF raised and lowered among them), the binary
    search alone / beside a direct table / on either side of KAS_IDMAP_CAP, the row loop's edges, scenarios without topics or
    brokers, a scenario cut into row-range items at 4096 rows (one, two and three items; FLUSH + merge) and three workgroups
    adding into one region of global counters (7,000 brokers) -- against the checker on the GPU's own rows and on the oracle's"""
    fb, _, want = solved(name)
    if name in WIDTH_CLASS:
        plan = native.Plan(ctx, fb)
        try:
            assert _width_class(fb) == WIDTH_CLASS[name] and f"kas_fill_kernel<{WIDTH_CLASS[name]}," in plan.describe(), plan.describe()
        finally:
            plan.close()
    ho, nodes, scen = native.solve_host_impact(fb, ctx=ctx)
    assert_same_impact(impact_ref(fb, ho), (nodes, scen), f"{name}, kas_solve_host_impact on its own rows")
    assert_same_impact(want, (nodes, scen), f"{name}, kas_solve_host_impact against the oracle's rows")
    check_invariants(fb, ho, (nodes, scen))
    hd, got = _device_impact(ctx, fb, False)
    assert (got[0]["reserved"] == 0).all()
    assert_same_impact(impact_ref(fb, hd), got, f"{name}, kas_impact_device on its own rows")
    assert_same_impact(want, got, f"{name}, kas_impact_device against the oracle's rows")


@pytest.mark.parametrize("name", ["row_counts", "rows_10000", "many_brokers_10000"])
def test_host_and_device_impact16_on_the_named_batches(ctx, name):
    """the same on 16-bit cells: the row loop's edges, FLUSH items + merge, GLOBAL counters shared by three workgroups"""
    fb, _, want = solved(name)
    ho, nodes, scen = native.solve_host_impact(fb, cells16=True, ctx=ctx)
    assert ho.out.dtype == np.uint16
    assert_same_impact(impact_ref(fb, ho, cells16=True), (nodes, scen), f"{name}, kas_solve_host16_impact on its own rows")
    assert_same_impact(want, (nodes, scen), f"{name}, kas_solve_host16_impact against the oracle's int32 solve")
    hd, got = _device_impact(ctx, fb, True)
    assert_same_impact(impact_ref(fb, hd, cells16=True), got, f"{name}, kas_impact_device16 on its own rows")
    assert_same_impact(want, got, f"{name}, kas_impact_device16 against the oracle's int32 solve")


def test_host16_impact_widened_to_int32_cells(ctx):
    """kas_solve_host16_impact at RF 5 and 4: kas_cells16_ok admits lists up to 3 wide, so the call is widened to int32 cells and
    the pass runs over the widened tables; a 16-bit plan of that batch is refused"""
    fb, _, want = solved("rf_4_5")
    h32, n32, s32 = native.solve_host_impact(fb, ctx=ctx)
    h16, n16, s16 = native.solve_host_impact(fb, cells16=True, ctx=ctx)
    assert h16.out.dtype == np.uint16
    assert_same_impact((n32, s32), (n16, s16), "RF 5: 16-bit call against the int32 call")
    assert_same_impact(want, (n16, s16), "RF 5: 16-bit call against the oracle")
    assert_same_impact(impact_ref(fb, h16, cells16=True), (n16, s16), "RF 5: 16-bit call on the rows it returned")
    with pytest.raises(native.KasError) as e:
        native.Plan(ctx, fb, cells16=True)
    assert e.value.code == abi.KAS_E_UNSUPPORTED and "16-bit cells: lists up to 3 wide" in e.value.detail


def test_host_impact_on_a_plan_rebuilt_in_place_for_other_broker_sets():
    """Three kas_solve_host_impact calls of one shape on one context whose broker sets differ in size (1, 2 and 3 brokers taken
    out): the cached plan is rebuilt in place (no hit, no allocation) and node_base, region_off and the work list with it"""
    ctx = native.DeviceContext(0)
    try:
        fbs = replan_batches()
        assert len({tuple(fb.scen["n_nodes"].tolist()) for fb in fbs}) == 3
        stats = []
        for k, fb in enumerate(fbs + fbs[:1]):
            assert fb.topics.tobytes() == fbs[0].topics.tobytes() and np.array_equal(fb.cur, fbs[0].cur)
            _, want = guarded(fb, merge=True)
            ho, nodes, scen = native.solve_host_impact(fb, ctx=ctx)
            assert_same_impact(impact_ref(fb, ho), (nodes, scen), f"call {k}, on its own rows")
            assert_same_impact(want, (nodes, scen), f"call {k}, against the oracle's rows")
            stats.append(ctx.host_stats())
        assert [s[0] for s in stats] == [1, 2, 3, 4] and all(s[1] == 0 for s in stats[:3])     # every call a miss ...
        assert stats[0][2] > 0 and all(s[2] == stats[0][2] for s in stats[1:]), stats           # ... and yet no allocation
    finally:
        ctx.close()


def _whatif_check(w, variants, ctx):
    """WhatIf.solve(impact=True, rows=False) against the checker on the oracle's solve of the same batch"""
    res = w.solve(variants, impact=True, rows=False)
    fb = w.flat_batch(variants)
    ho, (nodes, scen) = guarded(fb, merge=True)
    base = native.node_blocks(fb)
    for s, r in enumerate(res):
        for f in abi.SCENARIO_IMPACT_FIELDS:
            assert getattr(r, f) == int(scen[f][s]), (s, f)
        ids = fb.node_id[int(fb.scen["node_off"][s]):][:int(fb.scen["n_nodes"][s])]
        assert r.broker_impact() == {int(b): {f: int(nodes[f][base[s] + i]) for f in abi.NODE_IMPACT_FIELDS} for i, b in enumerate(ids)}
        assert r.moved_replicas == int(ho.scenario_results["moved_replicas"][s]) and r.status == int(ho.scenario_results["status"][s])
    return res


def test_whatif_impact_twice_with_other_variants(ctx):
    """what the what-if caller does on every call after its first: other broker sets over the same snapshot"""
    from kafka_assigner_amd.whatif import Variant, WhatIf
    w = WhatIf(*whatif_inputs())
    first = _whatif_check(w, [Variant(label="as is"), Variant(remove=[3]), Variant(remove=[1, 2, 5]),
                              Variant(add={60: "r0", 61: "r1"}), Variant(rack_aware=False)], ctx)
    second = _whatif_check(w, [Variant(remove=[7, 40]), Variant(remove=[11]), Variant(remove=[0, 59], rack_aware=False),
                               Variant(remove=[20, 21, 22]), Variant(remove=[33])], ctx)
    assert 3 not in first[1].broker_impact() and 60 in first[3].broker_impact()
    assert 7 not in second[0].broker_impact() and len(second[3].broker_impact()) == 57


def _device_impact_twice(ctx, fb):
    """_device_impact's sequence with a second kas_impact_device on another stream, no host synchronisation in between and
    output arrays of its own: (HostOutputs, first (nodes, scenarios), second (nodes, scenarios))"""
    import torch
    dev = torch.device("cuda", ctx.device)
    plan = native.Plan(ctx, fb)
    try:
        _, ho = host_tables(fb)
        d_cur = torch.from_numpy(fb.cur.copy()).to(dev)
        d_aux = torch.from_numpy(fb.aux).to(dev) if fb.aux.size else None
        d_out = torch.full((max(fb.out_len, 1),), -2, dtype=torch.int32, device=dev)
        d_tr = torch.zeros(max(fb.n_topics, 1) * 16, dtype=torch.uint8, device=dev)
        d_sr = torch.zeros(max(fb.n_scenarios, 1) * 32, dtype=torch.uint8, device=dev)
        n_nodes = int(native.node_blocks(fb)[-1])
        outs = [(torch.full((max(n_nodes, 1) * 32,), 0x5A, dtype=torch.uint8, device=dev),
                 torch.full((max(fb.n_scenarios, 1) * 32,), 0x5A, dtype=torch.uint8, device=dev)) for _ in range(2)]
        streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
        for st in streams:
            st.wait_stream(torch.cuda.current_stream(dev))
        aux = d_aux.data_ptr() if d_aux is not None else 0
        plan.solve_device(d_cur.data_ptr(), d_out.data_ptr(), d_tr.data_ptr(), d_sr.data_ptr(), aux=aux, stream=streams[0].cuda_stream)
        for st, (d_nodes, d_scen) in zip(streams, outs):
            plan.impact_device(d_cur.data_ptr(), d_out.data_ptr(), d_tr.data_ptr(), d_nodes.data_ptr(), d_scen.data_ptr(), aux=aux,
                               stream=st.cuda_stream)
        for st in streams:
            st.synchronize()
        ho.out = d_out.cpu().numpy()
        ho.topic_results = d_tr.cpu().numpy().view(abi.TOPIC_RESULT_DTYPE)
        ho.scenario_results = d_sr.cpu().numpy().view(abi.SCENARIO_RESULT_DTYPE)
        got = [(n.cpu().numpy().view(abi.NODE_IMPACT_DTYPE)[:n_nodes], s.cpu().numpy().view(abi.SCENARIO_IMPACT_DTYPE)[:fb.n_scenarios])
               for n, s in outs]
        return ho, got[0], got[1]
    finally:
        plan.close()


@pytest.mark.parametrize("name", ["rows_10000", "many_brokers_10000"], ids=["flush", "global"])
def test_two_impact_passes_on_one_plan(ctx, name):
    """the plan's counters are zeroed again before the second pass, which waits for the first (ev_impact) on its own stream"""
    fb, _, want = solved(name)
    ho, first, second = _device_impact_twice(ctx, fb)
    assert_same_impact(impact_ref(fb, ho), first, f"{name}: first pass")
    assert_same_impact(want, first, f"{name}: first pass against the oracle's rows")
    assert_same_impact(want, second, f"{name}: second pass, other stream")


def _headline(seed=5, S=1000, P=100_000, N=1000, R=20):
    """BASELINE's headline shape as a what-if: S broker-set variants of ONE P x RF 3 snapshot over N brokers in R racks"""
    cur = G.random_assignment(seed, P, N, R, 3)
    ids, racks = [], []
    for s in range(S):
        _, bs = G.scenario_action(seed, s, N, R, actions=G.BENCH_ACTIONS)
        ids.append(bs.node_id); racks.append(bs.node_rack)
    return node_set_batch(ids, racks, P, 3, 3, shared_cur=True, cur=cur), cur


def _one_variant(fb, cur, s, ho_sel, at, scen_rec, topic_rec):
    """scenario s of a single-topic what-if batch as a batch of its own, with its packed rows from ho_sel.out[at:]"""
    off, n = int(fb.scen["node_off"][s]), int(fb.scen["n_nodes"][s])
    P, ow = int(fb.topics["n_partitions"][s]), int(fb.topics["out_width"][s])
    one = node_set_batch([fb.node_id[off:off + n]], [fb.node_rack[off:off + n]], P, cur.shape[1], 3, cur=cur)
    ho = HostOutputs(out=ho_sel.out[at:at + P * ow].copy(), topic_results=topic_rec, scenario_results=scen_rec, ctx=one.ctx)
    return one, ho


def test_headline_batch_and_ratio_guard(ctx):
    """1000 x 100k x 1k brokers x 20 racks, RF 3: the host call's impact against the checker on sampled variants and the
    invariants on all; the device pass at most half the solve's device time, both measured here"""
    import torch
    fb, cur = _headline()
    sel = [0, 1, 499, 998]
    ho, nodes, scen = native.solve_host_impact(fb, select=sel, ctx=ctx)
    base = native.node_blocks(fb)
    assert (nodes["inbound"].reshape(-1).sum() == ho.scenario_results["moved_replicas"].sum())
    for s in range(fb.n_scenarios):
        blk = nodes[base[s]:base[s + 1]]
        assert int(blk["inbound"].sum()) == int(ho.scenario_results["moved_replicas"][s])
        if int(ho.scenario_results["status"][s]) == abi.KAS_OK:
            assert int(blk["replicas_after"].sum()) == 3 * 100_000 and int(blk["leaders_after"].sum()) == 100_000
    for k, s in enumerate(sel):
        one, h1 = _one_variant(fb, cur, s, ho, k * 300_000, ho.scenario_results[s:s + 1], ho.topic_results[s:s + 1])
        assert_same_impact(impact_ref(one, h1), (nodes[base[s]:base[s + 1]], scen[s:s + 1]), f"headline variant {s}")
    # device time: the plan's solve (kas_plan_kernel_time_us) against the impact pass (events on the same stream)
    dev = torch.device("cuda", ctx.device)
    plan = native.Plan(ctx, fb)
    try:
        d_cur = torch.from_numpy(fb.cur).to(dev)
        d_out = torch.empty(fb.out_len, dtype=torch.int32, device=dev)
        d_tr = torch.zeros(fb.n_topics * 16, dtype=torch.uint8, device=dev)
        d_sr = torch.zeros(fb.n_scenarios * 32, dtype=torch.uint8, device=dev)
        d_nodes = torch.empty(int(base[-1]) * 32, dtype=torch.uint8, device=dev)
        d_scen = torch.empty(fb.n_scenarios * 32, dtype=torch.uint8, device=dev)
        st = torch.cuda.Stream(dev)
        st.wait_stream(torch.cuda.current_stream(dev))
        args = (d_cur.data_ptr(), d_out.data_ptr(), d_tr.data_ptr())
        solve = lambda: plan.solve_device(*args, d_sr.data_ptr(), stream=st.cuda_stream)
        impact = lambda: plan.impact_device(*args, d_nodes.data_ptr(), d_scen.data_ptr(), stream=st.cuda_stream)
        solve(); impact(); st.synchronize()
        plan.kernel_time_us()                                    # (resets the accumulator)
        n, imp_ms = 3, []
        for _ in range(n):
            solve()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st); impact(); e1.record(st)
            st.synchronize()
            imp_ms.append(e0.elapsed_time(e1))
        solve_us, launches = plan.kernel_time_us()
        assert launches == n
        imp_us = 1e3 * float(np.median(imp_ms))
        print(f"headline: solve {solve_us:.0f} us, impact pass {imp_us:.0f} us ({imp_us / solve_us:.2f}x)")
        assert imp_us <= 0.5 * solve_us, (imp_us, solve_us)
        got_n = d_nodes.cpu().numpy().view(abi.NODE_IMPACT_DTYPE)
        assert_same_impact((nodes, scen), (got_n, d_scen.cpu().numpy().view(abi.SCENARIO_IMPACT_DTYPE)), "headline, device pass")
    finally:
        plan.close()


def test_host_path_cut_into_ranges(ctx):
    """scenario-by-scenario tables of ~96 MB: the host call cuts them into scenario ranges (one impact pass per range);
    int32 and 16-bit cells give identical impact records"""
    S, P, N, R = 40, 100_000, 200, 10
    cur = np.stack([G.random_assignment(60 + s, P, N, R, 3) for s in range(S)])
    sets = [G.scenario_action(61, s, N, R, actions=G.BENCH_ACTIONS)[1] for s in range(S)]
    fb = node_set_batch([b.node_id for b in sets], [b.node_rack for b in sets], P, 3, 3, cur=cur)
    plain = native.solve_host(fb, ctx)
    ho, nodes, scen = native.solve_host_impact(fb, ctx=ctx)
    _same_solve(plain, ho, "ranges: the solve with and without the impact pass")
    want = impact_ref(fb, ho)
    assert_same_impact(want, (nodes, scen), "host path cut into ranges")
    check_invariants(fb, ho, want)
    _, n16, s16 = native.solve_host_impact(fb, cells16=True, ctx=ctx)
    assert_same_impact((nodes, scen), (n16, s16), "int32 and 16-bit cells")


def test_configs4_scenario(ctx):
    """BASELINE configs[4]'s scenario: 1M partitions x 5k brokers, RF 5 (topic cut into items, merged)"""
    N, P, R = 5000, 1_000_000, 25
    cur = G.random_assignment(77, P, N, R, 5)
    bs = G.perturb_brokers(N, R, remove=list(range(0, 100, 5)), add=30)
    fb = node_set_batch([bs.node_id], [bs.node_rack], P, 5, 5, cur=cur)
    ho, nodes, scen = native.solve_host_impact(fb, ctx=ctx)
    assert int(ho.scenario_results["status"][0]) == abi.KAS_OK
    want = impact_ref(fb, ho)
    assert_same_impact(want, (nodes, scen), "configs[4] scenario")
    assert int(scen["departed_replicas"][0]) > 0 and int(scen["max_inbound"][0]) > 0


def test_whatif_impact_without_rows_equals_checker(ctx):
    from kafka_assigner_amd.whatif import Variant, WhatIf
    brokers = {b: "r%d" % (b % 6) for b in range(60)}
    topics = {name: {p: G.random_assignment(seed, P, 60, 6, 3)[p].tolist() for p in range(P)}
              for name, P, seed in (("orders", 3000, 1), ("clicks", 1200, 2))}
    w = WhatIf(brokers, topics)
    variants = [Variant(label="as is"), Variant(remove=[3], label="-3"), Variant(remove=[1, 2, 5]),
                Variant(add={60: "r0", 61: "r1"}, label="+2"), Variant(rack_aware=False)]
    res = w.solve(variants, impact=True, rows=False)
    fb = w.flat_batch(variants)
    ho = native.solve_host(fb, ctx)
    nodes, scen = impact_ref(fb, ho)
    base = native.node_blocks(fb)
    for s, r in enumerate(res):
        for f in abi.SCENARIO_IMPACT_FIELDS:
            assert getattr(r, f) == int(scen[f][s]), (s, f)
        ids = fb.node_id[int(fb.scen["node_off"][s]):][:int(fb.scen["n_nodes"][s])]
        want = {int(b): {f: int(nodes[f][base[s] + i]) for f in abi.NODE_IMPACT_FIELDS} for i, b in enumerate(ids)}
        assert r.broker_impact() == want
        assert r.moved_replicas == int(ho.scenario_results["moved_replicas"][s])
        with pytest.raises(ValueError):
            r.assignment("orders")
    assert 3 not in res[1].broker_impact() and 60 in res[3].broker_impact()
    ok = [r for r in res if r.status == abi.KAS_OK]
    assert ok and all(sum(v["replicas_after"] for v in r.broker_impact().values()) == 3 * 4200 for r in ok)
    plain = w.solve(variants)                                    # the defaults: today's behaviour
    assert plain[0].max_inbound is None and plain[1].assignment("orders")


def test_cli_print_impact(tmp_path):
    from kafka_assigner_amd import build as kbuild
    from test_host_cli import _run, _sections, _snapshot
    cli = kbuild.build_host()
    C1 = GOLD["config1"]
    case = [c for c in C1["cases"] if c["name"] == "replace 5->6 (rack c)"][0]
    all_brokers = set(range(9))
    racks = {str(b): "abc"[b % 3] for b in range(6)}
    racks.update({"6": "c", "7": "a", "8": "b"})
    path, _ = _snapshot(tmp_path, all_brokers, racks)
    args = ["--snapshot", path, "--mode", "PRINT_REASSIGNMENT", "--integer_broker_ids", ",".join(str(b) for b in case["brokers"])]
    plain = _run(cli, *args)
    assert plain.returncode == 0, plain.stderr
    assert "REASSIGNMENT IMPACT" not in plain.stdout
    r = _run(cli, *args, "--print_impact")
    assert r.returncode == 0, r.stderr
    head, tail = r.stdout.split("REASSIGNMENT IMPACT:\n")
    assert head == plain.stdout                                  # everything before it exactly as without the flag
    got = json.loads(tail)
    brokers = sorted(case["brokers"])
    sc = Scenario(brokers=brokers, racks={b: racks[str(b)] for b in brokers},
                  topics=[Topic(name, {int(p): v for p, v in C1["current"][t].items()}, 3) for t, name in enumerate(C1["topics"])])
    fb = flatten([sc])
    ho = oracle_solve(fb)
    nodes, scen = impact_ref(fb, ho)
    want = [{"id": int(b), **{f: int(nodes[f][i]) for f in abi.NODE_IMPACT_FIELDS}} for i, b in enumerate(fb.node_id)]
    assert got["brokers"] == want
    assert got["departed_replicas"] == int(scen["departed_replicas"][0]) > 0
    assert got["leaders_moved"] == int(scen["leaders_moved"][0])
    assert got["moved_replicas"] == int(ho.scenario_results["moved_replicas"][0]) == sum(case["moved_replicas"])

"""The rack pass on the MI355X (kas_rack_impact_device / 16, kas_solve_host_rack_impact / 16, WhatIf.solve(racks=True), the CLI's
--print_rack_impact), against the NumPy checker of tests/rack_ref.py.  Everything is integer and compared for equality."""
import json
import os

import numpy as np
import pytest

from impact_batches import solved, whatif_inputs
from impact_ref import assert_same_impact, impact_ref
from kafka_assigner_amd import abi, native
from kafka_assigner_amd import generator as G
from kafka_assigner_amd.flatten import HostOutputs, Scenario, Topic, flatten, host_tables, node_set_batch, to_cells16
from oracle_lib import oracle_solve
from rack_ref import assert_same_racks, check_identities, rack_counts, rack_ref
from test_racks_cpu import blocks_of_six, one_rack, own, rack_per_node, real_racks

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    return native.DeviceContext(0)


def _batch(name):
    """(fb, the report table the case is about or None)"""
    if name in ("rack_unaware", "shared_prefix", "duplicates", "width_1", "split_9000"):
        fb, ho = own(name)
        assert (ho.topic_results["status"] == abi.KAS_OK).all(), name       # (the oracle's solve: the batch counts rows)
        return fb, {"rack_unaware": lambda: real_racks(fb, 8), "shared_prefix": lambda: blocks_of_six(fb)}.get(name, lambda: None)()
    return solved(name)[0], None


def _got(rk):
    return rk.racks, rk.scenarios, rk.rack_off


HOST_CASES = ["mixed7", "mixed42", "row_counts", "degenerate", "widths_4_5", "widths_6_8", "sparse", "rows_10000", "many_brokers",
              "rack_unaware", "shared_prefix", "duplicates", "width_1", "split_9000"]


@pytest.mark.parametrize("name", HOST_CASES)
def test_host_rack_impact_equals_checker(ctx, name):
    """kas_solve_host_rack_impact on int32 cells: the checker on the GPU's own rows, the same records as kas_solve_host_impact,
    and again with the node records left on the device (nodes == NULL), on one rack and on one rack per node"""
    fb, table = _batch(name)
    plain, n0, s0 = native.solve_host_impact(fb, ctx=ctx)
    ho, rk = native.solve_host_rack_impact(fb, report_rack=table, ctx=ctx)
    assert np.array_equal(plain.out, ho.out) and (plain.scenario_results["digest"] == ho.scenario_results["digest"]).all()
    assert_same_impact((n0, s0), (rk.nodes, rk.impact), f"{name}: the impact records with and without the rack pass")
    assert_same_impact(impact_ref(fb, ho), (rk.nodes, rk.impact), f"{name}: the impact records against the checker")
    want = rack_ref(fb, ho, table, nodes=rk.nodes)
    assert_same_racks(want, _got(rk), f"{name}, kas_solve_host_rack_impact")
    check_identities(fb, ho, rk.nodes, _got(rk))
    for t2 in (one_rack(fb), rack_per_node(fb)):
        ho2, rk2 = native.solve_host_rack_impact(fb, report_rack=t2, select=[], nodes=False, ctx=ctx)
        assert rk2.nodes is None
        assert_same_racks(rack_ref(fb, ho, t2, nodes=rk.nodes), _got(rk2), f"{name}, nodes == NULL, n_select = 0, another table")
        assert_same_impact((rk.nodes, rk.impact), (rk.nodes, rk2.impact), f"{name}: scenario impact records, nodes == NULL")


@pytest.mark.parametrize("name", ["mixed7", "row_counts", "degenerate", "rows_10000", "many_brokers", "rack_unaware", "shared_prefix"])
def test_host16_rack_impact_equals_checker(ctx, name):
    fb, table = _batch(name)
    ho, rk = native.solve_host_rack_impact(fb, report_rack=table, cells16=True, ctx=ctx)
    assert ho.out.dtype == np.uint16
    nodes = impact_ref(fb, ho, cells16=True)[0]
    assert_same_racks(rack_ref(fb, ho, table, cells16=True, nodes=nodes), _got(rk), f"{name}, kas_solve_host16_rack_impact")
    _, rk32 = native.solve_host_rack_impact(fb, report_rack=table, ctx=ctx)
    assert_same_racks(_got(rk32), _got(rk), f"{name}: int32 and 16-bit cells")


def test_host16_rack_impact_widened_to_int32_cells(ctx):
    """lists 4 and 5 wide: the 16-bit call is widened and the pass runs over the widened tables"""
    fb, _, _ = solved("rf_4_5")
    _, rk32 = native.solve_host_rack_impact(fb, ctx=ctx)
    ho, rk16 = native.solve_host_rack_impact(fb, cells16=True, ctx=ctx)
    assert_same_racks(_got(rk32), _got(rk16), "RF 5: 16-bit call against the int32 call")
    assert_same_racks(rack_ref(fb, ho, None, cells16=True), _got(rk16), "RF 5: 16-bit call on the rows it returned")


def _device_racks(ctx, fb, cells16, tables):
    """Plan + solve_device + impact_device + one rack_impact_device per table of `tables` on one torch stream, no host
    synchronisation between the rack passes (each has output arrays of its own): (HostOutputs, nodes, [(racks, scen, rack_off)])"""
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
        caps = [int(rack_counts(fb, t).sum()) for t in tables]
        outs = [(torch.full((max(c, 1) * 32,), 0x5A, dtype=torch.uint8, device=dev),
                 torch.full((max(fb.n_scenarios, 1) * 64,), 0x5A, dtype=torch.uint8, device=dev)) for c in caps]
        st = torch.cuda.Stream(dev)
        st.wait_stream(torch.cuda.current_stream(dev))
        aux = d_aux.data_ptr() if d_aux is not None else 0
        args = (d_cur.data_ptr(), d_out.data_ptr(), d_tr.data_ptr())
        # before the plan has solved: refused
        with pytest.raises(native.KasError) as e:
            plan.rack_impact_device(*args, d_nodes.data_ptr(), d_scen.data_ptr(), outs[0][0].data_ptr(), caps[0], outs[0][1].data_ptr(),
                                    report_rack=tables[0], aux=aux, stream=st.cuda_stream)
        assert e.value.code == abi.KAS_E_INVALID_ARG and "no solve and impact pass" in e.value.detail
        plan.solve_device(*args, d_sr.data_ptr(), aux=aux, stream=st.cuda_stream)
        plan.impact_device(*args, d_nodes.data_ptr(), d_scen.data_ptr(), aux=aux, stream=st.cuda_stream)
        offs = []
        for t, c, (d_racks, d_rscen) in zip(tables, caps, outs):
            offs.append(plan.rack_impact_device(*args, d_nodes.data_ptr(), d_scen.data_ptr(), d_racks.data_ptr(), c, d_rscen.data_ptr(),
                                                report_rack=t, aux=aux, stream=st.cuda_stream))
        st.synchronize()
        ho.out = d_out.cpu().numpy().view(np.uint16) if cells16 else d_out.cpu().numpy()
        ho.topic_results = d_tr.cpu().numpy().view(abi.TOPIC_RESULT_DTYPE)
        ho.scenario_results = d_sr.cpu().numpy().view(abi.SCENARIO_RESULT_DTYPE)
        nodes = d_nodes.cpu().numpy().view(abi.NODE_IMPACT_DTYPE)[:n_nodes]
        got = [(r.cpu().numpy().view(abi.RACK_IMPACT_DTYPE)[:c], s.cpu().numpy().view(abi.SCENARIO_RACK_IMPACT_DTYPE)[:fb.n_scenarios], o)
               for (r, s), c, o in zip(outs, caps, offs)]
        return ho, nodes, got
    finally:
        plan.close()


@pytest.mark.parametrize("cells16", [False, True], ids=["int32", "cells16"])
@pytest.mark.parametrize("name", ["mixed7", "rows_10000", "many_brokers", "shared_prefix"])
def test_device_rack_impact_and_a_change_of_table(ctx, name, cells16):
    """kas_rack_impact_device / 16: the batch's own table (NULL), another table, a copy of it at another address, the first
    again -- four passes on one plan and one stream, each with its own table's records"""
    fb, table = _batch(name)
    other = rack_per_node(fb) if table is None else table
    tables = [None, other, other.copy(), None]
    ho, nodes, got = _device_racks(ctx, fb, cells16, tables)
    want_nodes = impact_ref(fb, ho, cells16=cells16)[0]
    for f in abi.NODE_IMPACT_FIELDS:
        assert (nodes[f] == want_nodes[f]).all(), f
    for k, (t, g) in enumerate(zip(tables, got)):
        assert (g[0]["reserved"] == 0).all() and (g[1]["reserved"] == 0).all()
        assert_same_racks(rack_ref(fb, ho, t, cells16=cells16, nodes=want_nodes), g, f"{name}: pass {k}")
    assert int(got[0][2][-1]) != int(got[1][2][-1])                              # (the two tables lay their blocks out differently)


def test_refusals_before_any_gpu_work(ctx):
    fb, _, _ = solved("mixed7")
    need = int(rack_counts(fb).sum())
    neg = fb.node_rack.copy(); neg[3] = -1
    big = fb.node_rack.copy(); big[5] = abi.KAS_RACK_LIMIT
    both = big.copy(); both[int(fb.scen["node_off"][1]) + 2] = -1
    calls0 = ctx.host_stats()
    for table, cap, code, text in ((neg, None, abi.KAS_E_INVALID_ARG, "negative"), (big, None, abi.KAS_E_UNSUPPORTED, "KAS_RACK_LIMIT"),
                                   (both, 0, abi.KAS_E_INVALID_ARG, "negative"), (big, 0, abi.KAS_E_UNSUPPORTED, "KAS_RACK_LIMIT"),
                                   (None, need - 1, abi.KAS_E_INVALID_ARG, "racks_cap")):
        with pytest.raises(native.KasError) as e:
            native.solve_host_rack_impact(fb, report_rack=table, racks_cap=cap if cap is not None else 5000, ctx=ctx)
        assert e.value.code == code and text in e.value.detail, e.value.detail
    assert ctx.host_stats()[2] == calls0[2]                                      # nothing was allocated for them
    ho, rk = native.solve_host_rack_impact(fb, racks_cap=need + 7, ctx=ctx)       # a roomy capacity is fine
    assert_same_racks(rack_ref(fb, ho, None), _got(rk), "roomy racks_cap")


def test_host_path_cut_into_scenario_ranges(ctx):
    """scenario-by-scenario tables of 52.8 MB (above KAS_HOST_SPLIT_MIN_BYTES = 48 MiB): the host call cuts them into two scenario
    ranges, one rack pass per range on the range's stream with its slice of the report table; the records equal those of the two
    halves (26.4 MB: one range each) solved as calls of their own, and the checker's on the first scenario of each range"""
    S, P, N, R = 22, 100_000, 200, 10
    cur = np.stack([G.random_assignment(60 + s, P, N, R, 3) for s in range(S)])
    sets = [G.scenario_action(61, s, N, R, actions=G.BENCH_ACTIONS)[1] for s in range(S)]
    fb = node_set_batch([b.node_id for b in sets], [b.node_rack for b in sets], P, 3, 3, cur=cur)
    table = (fb.node_id % 7).astype(np.int32)                                    # not the solver's table
    assert 48 << 20 <= 4 * (fb.cur.shape[0] + fb.out_len) < 3 * (24 << 20)
    ho, rk = native.solve_host_rack_impact(fb, report_rack=table, ctx=ctx)
    hits = ctx.host_stats()[1]
    again = native.solve_host_rack_impact(fb, report_rack=table.copy(), ctx=ctx)[1]      # the same call: every range finds its plan
    assert ctx.host_stats()[1] - hits == 2, "the call was not cut into two scenario ranges"
    assert_same_racks(_got(rk), _got(again), "the second call, on cached plans that hold the table already")
    assert rk.scenarios["n_racks"].tolist() == [7] * S and rk.rack_off.tolist() == list(range(0, 7 * S + 1, 7))
    check_identities(fb, ho, rk.nodes, _got(rk))
    halves = []
    for lo, hi in ((0, S // 2), (S // 2, S)):
        half = node_set_batch([b.node_id for b in sets[lo:hi]], [b.node_rack for b in sets[lo:hi]], P, 3, 3, cur=cur[lo:hi])
        n_lo, n_hi = int(fb.scen["node_off"][lo]), int(fb.scen["node_off"][hi - 1]) + int(fb.scen["n_nodes"][hi - 1])
        _, r = native.solve_host_rack_impact(half, report_rack=table[n_lo:n_hi], ctx=ctx)
        halves.append(r)
    for f in abi.RACK_IMPACT_FIELDS:
        assert (np.concatenate([h.racks[f] for h in halves]) == rk.racks[f]).all(), f
    for f in abi.SCENARIO_RACK_FIELDS:
        assert (np.concatenate([h.scenarios[f] for h in halves]) == rk.scenarios[f]).all(), f
    base = native.node_blocks(fb)
    # (first fit strands a row in about half of these scenarios; a failed scenario counts nothing, so the checker looks at the first
    # scenario of each range that solves, and the rows it counts collide on a table that is not the solver's)
    ok = ho.scenario_results["status"] == abi.KAS_OK
    sample = [int(np.nonzero(ok[lo:hi])[0][0]) + lo for lo, hi in ((0, S // 2), (S // 2, S))]
    assert ok[:S // 2].sum() >= 3 and ok[S // 2:].sum() >= 3, ok.tolist()
    assert (rk.scenarios["colocated_after"][ok] > 0).all() and not rk.scenarios["colocated_after"][~ok].any()
    for s in sample:
        off, n = int(fb.scen["node_off"][s]), int(fb.scen["n_nodes"][s])
        one = node_set_batch([fb.node_id[off:off + n]], [fb.node_rack[off:off + n]], P, 3, 3, cur=cur[s:s + 1])
        o = int(fb.topics["out_off"][s])
        h1 = HostOutputs(out=ho.out[o:o + 3 * P].copy(), topic_results=ho.topic_results[s:s + 1], scenario_results=ho.scenario_results[s:s + 1],
                         ctx=one.ctx)
        want = rack_ref(one, h1, table[off:off + n], nodes=rk.nodes[base[s]:base[s + 1]])
        assert_same_racks(want, (rk.of(s), rk.scenarios[s:s + 1], np.asarray([0, 7])), f"range scenario {s}")


def test_whatif_racks_with_a_rack_unaware_variant(ctx):
    """WhatIf.solve(impact=True, racks=True): the rack-unaware variant is reported on the real racks and collides, its rack-aware
    sibling does not; the oracle's rows (CPU) collide on the same fixture"""
    from kafka_assigner_amd.whatif import Variant, WhatIf
    w = WhatIf(*whatif_inputs())
    variants = [Variant(remove=[3, 17], rack_aware=False, label="unaware"), Variant(remove=[3, 17], label="aware"), Variant(label="as is")]
    fb = w.flat_batch(variants)
    table, names = w.report_racks(variants)
    oracle = rack_ref(fb, oracle_solve(fb), table)
    assert int(oracle[1]["colocated_after"][0]) > 0 and int(oracle[1]["colocated_after"][1]) == 0     # the oracle's rows collide
    res = w.solve(variants, impact=True, racks=True, rows=False)
    assert all(r.status == abi.KAS_OK for r in res)
    assert res[0].colocated_after > 0 and res[0].rows_colocated_after > 0 and res[1].colocated_after == 0 and res[2].colocated_after == 0
    assert res[0].n_racks == res[1].n_racks == 6 and res[0].colocated_before == 0
    ho = native.solve_host(fb, ctx)
    want = rack_ref(fb, ho, table)
    for s, r in enumerate(res):
        for f in abi.SCENARIO_RACK_FIELDS:
            assert getattr(r, f) == int(want[1][f][s]), (s, f)
        blk = want[0][int(want[2][s]):int(want[2][s + 1])]
        assert r.rack_impact() == {names[s][k]: {f: int(blk[f][k]) for f in abi.RACK_IMPACT_FIELDS} for k in range(len(blk))}
        assert sorted(r.rack_impact()) == ["r%d" % k for k in range(6)]
        assert sum(v["inbound"] for v in r.rack_impact().values()) == r.moved_replicas
        assert sum(v["replicas_after"] for v in r.rack_impact().values()) == sum(v["replicas_after"] for v in r.broker_impact().values())
    with_rows = w.solve(variants[:2], impact=True, racks=True)
    assert with_rows[0].assignment("orders") and with_rows[0].colocated_after == res[0].colocated_after
    plain = w.solve(variants[:2], impact=True)                                   # the defaults: today's behaviour
    assert plain[0].colocated_after is None and plain[0].max_inbound == res[0].max_inbound
    with pytest.raises(ValueError):
        plain[0].rack_impact()
    with pytest.raises(ValueError):
        w.solve(variants, racks=True)


def test_cli_print_rack_impact(tmp_path):
    from kafka_assigner_amd import build as kbuild
    from test_host_cli import _run, _snapshot
    from test_impact_cpu import GOLD
    cli = kbuild.build_host()
    C1 = GOLD["config1"]
    case = [c for c in C1["cases"] if c["name"] == "replace 5->6 (rack c)"][0]
    racks = {str(b): "abc"[b % 3] for b in range(6)}
    racks.update({"6": "c", "7": "a", "8": "b"})
    path, _ = _snapshot(tmp_path, set(range(9)), racks)
    args = ["--snapshot", path, "--mode", "PRINT_REASSIGNMENT", "--integer_broker_ids", ",".join(str(b) for b in case["brokers"])]
    brokers = sorted(case["brokers"])
    for extra, rack_aware in (([], True), (["--disable_rack_awareness"], False)):
        plain = _run(cli, *args, *extra, "--print_impact")
        assert plain.returncode == 0 and "REASSIGNMENT RACK IMPACT" not in plain.stdout, plain.stderr
        r = _run(cli, *args, *extra, "--print_impact", "--print_rack_impact")
        assert r.returncode == 0, r.stderr
        head, tail = r.stdout.split("REASSIGNMENT RACK IMPACT:\n")
        assert head == plain.stdout                              # everything before it exactly as without the flag
        got = json.loads(tail)
        alone = _run(cli, *args, *extra, "--print_rack_impact")     # without --print_impact: the node records stay on the device
        assert alone.returncode == 0 and json.loads(alone.stdout.split("REASSIGNMENT RACK IMPACT:\n")[1]) == got, alone.stderr
        # the run solves its topics one by one (one Context): the per-rack counters and the row sums of the topics add up
        real = {b: racks[str(b)] for b in brokers}
        names = []
        for b in brokers:
            if real[b] not in names:
                names.append(real[b])
        table = np.asarray([names.index(real[b]) for b in brokers], dtype=np.int32)
        sc = Scenario(brokers=brokers, racks=real if rack_aware else {},
                      topics=[Topic(name, {int(p): v for p, v in C1["current"][t].items()}, 3) for t, name in enumerate(C1["topics"])])
        fb = flatten([sc])
        ho = oracle_solve(fb)
        want = rack_ref(fb, ho, table)
        assert [e["rack"] for e in got["racks"]] == names
        for k, e in enumerate(got["racks"]):
            assert {f: e[f] for f in abi.RACK_IMPACT_FIELDS} == {f: int(want[0][f][k]) for f in abi.RACK_IMPACT_FIELDS}, (k, e)
        for f in abi.SCENARIO_RACK_ROW_FIELDS:
            assert got[f] == int(want[1][f][0]), f
        assert got["colocated_before"] == 0

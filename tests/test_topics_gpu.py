"""The topic pass on the MI355X (kas_topic_impact_device / 16, kas_solve_host_topic_impact / 16, WhatIf.solve(topics=True), the
CLI's --print_topic_impact), against the checker of tests/topic_ref.py.  Everything is integer and compared for equality."""
import copy
import json
import os

import numpy as np
import pytest

from impact_batches import solved, whatif_inputs
from impact_ref import assert_same_impact, impact_ref
from kafka_assigner_amd import abi, native
from kafka_assigner_amd.flatten import Scenario, Topic, flatten, host_tables, to_cells16
from oracle_lib import oracle_solve
from test_topics_cpu import own
from topic_ref import assert_same_topics, check_topic_identities, topic_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    return native.DeviceContext(0)


def _batch(name):
    return own(name)[0] if name in ("A", "B", "C") else solved(name)[0]


def _got(tp):
    return tp.topics, tp.scenarios


HOST_CASES = ["mixed7", "row_counts", "widths_4_5", "widths_6_8", "sparse", "degenerate", "rows_10000", "A", "B", "C"]


@pytest.mark.parametrize("name", HOST_CASES)
def test_host_topic_impact_equals_checker(ctx, name):
    """kas_solve_host_topic_impact on int32 cells: the solve's own outputs and the impact records are kas_solve_host_impact's,
    the topic records the checker's on the GPU's own rows, and the identities that tie them to the impact records hold"""
    fb = _batch(name)
    plain, n0, s0 = native.solve_host_impact(fb, ctx=ctx)
    ho, tp = native.solve_host_topic_impact(fb, ctx=ctx)
    assert np.array_equal(plain.out, ho.out) and (plain.scenario_results["digest"] == ho.scenario_results["digest"]).all()
    assert plain.topic_results.tobytes() == ho.topic_results.tobytes() and plain.scenario_results.tobytes() == ho.scenario_results.tobytes()
    assert_same_impact((n0, s0), (tp.nodes, tp.impact), f"{name}: the impact records with and without the topic pass")
    want = topic_ref(fb, ho)
    assert_same_topics(want, _got(tp), f"{name}, kas_solve_host_topic_impact")
    check_topic_identities(fb, ho, impact_ref(fb, ho), _got(tp))
    if name in ("A", "B", "C"):                                   # (the GPU's solve is the oracle's: the counts the issue names)
        assert_same_topics(own(name)[3], _got(tp), f"{name}: the oracle's rows")


@pytest.mark.parametrize("name", HOST_CASES)
def test_host16_topic_impact_equals_checker(ctx, name):
    """16-bit cells: on the kernels with that I/O where the batch is taken, widened to int32 cells where it is not (lists wider
    than 3); either way the records of the int32 call"""
    fb = _batch(name)
    ho, tp = native.solve_host_topic_impact(fb, cells16=True, ctx=ctx)
    assert ho.out.dtype == np.uint16
    assert_same_topics(topic_ref(fb, ho, cells16=True), _got(tp), f"{name}, kas_solve_host16_topic_impact")
    _, tp32 = native.solve_host_topic_impact(fb, ctx=ctx)
    assert_same_topics(_got(tp32), _got(tp), f"{name}: int32 and 16-bit cells")


@pytest.mark.parametrize("cells16", [False, True], ids=["int32", "cells16"])
@pytest.mark.parametrize("name", ["mixed7", "A", "C"])
def test_host_impact_null_and_nodes_null(ctx, name, cells16):
    """host_impact == NULL: no impact pass, the same topic records and the same solve; host_impact->nodes == NULL: the scenario
    impact records come back, the node records stay on the device; n_select = 0: no rows"""
    fb = _batch(name)
    ho, tp = native.solve_host_topic_impact(fb, cells16=cells16, ctx=ctx)
    ho0, bare = native.solve_host_topic_impact(fb, cells16=cells16, impact=False, ctx=ctx)
    assert bare.nodes is None and bare.impact is None
    assert np.array_equal(ho.out, ho0.out) and ho.topic_results.tobytes() == ho0.topic_results.tobytes()
    assert_same_topics(_got(tp), _got(bare), f"{name}: host_impact == NULL")
    ho1, lean = native.solve_host_topic_impact(fb, cells16=cells16, select=[], nodes=False, ctx=ctx)
    assert lean.nodes is None
    assert_same_topics(_got(tp), _got(lean), f"{name}: nodes == NULL, n_select = 0")
    assert_same_impact((tp.nodes, tp.impact), (tp.nodes, lean.impact), f"{name}: scenario impact records, nodes == NULL")
    ho2, none = native.solve_host_topic_impact(fb, cells16=cells16, select=[], impact=False, ctx=ctx)
    assert_same_topics(_got(tp), _got(none), f"{name}: host_impact == NULL, n_select = 0")
    assert ho2.scenario_results.tobytes() == ho.scenario_results.tobytes()


def _leaders_swapped(fb):
    """the batch with the first two cells of every cur row swapped: other tables for the same plan"""
    fb2 = copy.copy(fb)
    fb2.cur = fb.cur.copy()
    for td in fb.topics:
        P, cw, co = int(td["n_partitions"]), int(td["cur_width"]), int(td["cur_off"])
        if cw >= 2 and P > 0:
            rows = fb2.cur[co:co + P * cw].reshape(P, cw)
            rows[:, [0, 1]] = rows[:, [1, 0]]
    return fb2


def _device_topics(ctx, fb, fb2, cells16):
    """Plan + solve_device + two topic passes, then a solve over fb2's tables and a third pass, on one torch stream with no host
    synchronisation in between and no impact pass at all: [(HostOutputs, topics, scenarios)] x 3"""
    import torch
    dev = torch.device("cuda", ctx.device)
    plan = native.Plan(ctx, fb, cells16=cells16)
    try:
        T, S = fb.n_topics, fb.n_scenarios
        d_aux = torch.from_numpy(fb.aux).to(dev) if fb.aux.size else None
        aux = d_aux.data_ptr() if d_aux is not None else 0
        st = torch.cuda.Stream(dev)
        st.wait_stream(torch.cuda.current_stream(dev))

        def tables(b):
            cur = to_cells16(b).view(np.int16) if cells16 else b.cur
            return (torch.from_numpy(cur.copy()).to(dev),
                    torch.full((max(b.out_len, 1),), -2, dtype=torch.int16 if cells16 else torch.int32, device=dev),
                    torch.zeros(max(T, 1) * 16, dtype=torch.uint8, device=dev), torch.zeros(max(S, 1) * 32, dtype=torch.uint8, device=dev))

        def records():                                         # (every record must be written: 0x5A everywhere first)
            return (torch.full((max(T, 1) * 32,), 0x5A, dtype=torch.uint8, device=dev),
                    torch.full((max(S, 1) * 64,), 0x5A, dtype=torch.uint8, device=dev))
        t1, t2 = tables(fb), tables(fb2)
        outs = [records() for _ in range(3)]
        torch.cuda.current_stream(dev).synchronize()
        args1 = (t1[0].data_ptr(), t1[1].data_ptr(), t1[2].data_ptr())
        args2 = (t2[0].data_ptr(), t2[1].data_ptr(), t2[2].data_ptr())
        # before the plan has solved: refused; a NULL array comes first
        with pytest.raises(native.KasError) as e:
            plan.topic_impact_device(*args1, outs[0][0].data_ptr(), outs[0][1].data_ptr(), aux=aux, stream=st.cuda_stream)
        assert e.value.code == abi.KAS_E_INVALID_ARG and "no solve" in e.value.detail
        with pytest.raises(native.KasError) as e:
            plan.topic_impact_device(*args1, 0, outs[0][1].data_ptr(), aux=aux, stream=st.cuda_stream)
        assert e.value.code == abi.KAS_E_INVALID_ARG and "kas_topic_impact_tables" in e.value.detail
        plan.solve_device(*args1, t1[3].data_ptr(), aux=aux, stream=st.cuda_stream)
        plan.topic_impact_device(*args1, outs[0][0].data_ptr(), outs[0][1].data_ptr(), aux=aux, stream=st.cuda_stream)
        plan.topic_impact_device(*args1, outs[1][0].data_ptr(), outs[1][1].data_ptr(), aux=aux, stream=st.cuda_stream)
        plan.solve_device(*args2, t2[3].data_ptr(), aux=aux, stream=st.cuda_stream)
        plan.topic_impact_device(*args2, outs[2][0].data_ptr(), outs[2][1].data_ptr(), aux=aux, stream=st.cuda_stream)
        st.synchronize()
        res = []
        for k, (b, t) in enumerate(((fb, t1), (fb, t1), (fb2, t2))):
            _, ho = host_tables(b)
            ho.out = t[1].cpu().numpy().view(np.uint16) if cells16 else t[1].cpu().numpy()
            ho.topic_results = t[2].cpu().numpy().view(abi.TOPIC_RESULT_DTYPE)
            ho.scenario_results = t[3].cpu().numpy().view(abi.SCENARIO_RESULT_DTYPE)
            res.append((ho, outs[k][0].cpu().numpy().view(abi.TOPIC_IMPACT_DTYPE)[:T],
                        outs[k][1].cpu().numpy().view(abi.SCENARIO_TOPIC_IMPACT_DTYPE)[:S]))
        return res
    finally:
        plan.close()


@pytest.mark.parametrize("cells16", [False, True], ids=["int32", "cells16"])
@pytest.mark.parametrize("name", ["A", "C", "row_counts"])
def test_device_topic_impact_twice_and_after_a_resolve(ctx, name, cells16):
    """kas_topic_impact_device / 16 without an impact pass on the plan: two passes behind one solve write the same records (the
    plan's counters are zeroed in front of each), a third behind a solve over other tables writes those tables' records"""
    fb = _batch(name)
    fb2 = _leaders_swapped(fb)
    (ho, tp_a, sc_a), (_, tp_b, sc_b), (ho2, tp_c, sc_c) = _device_topics(ctx, fb, fb2, cells16)
    want = topic_ref(fb, ho, cells16=cells16)
    assert_same_topics(want, (tp_a, sc_a), f"{name}: first pass")
    assert_same_topics((tp_a, sc_a), (tp_b, sc_b), f"{name}: second pass on the same solve")
    want2 = topic_ref(fb2, ho2, cells16=cells16)
    assert_same_topics(want2, (tp_c, sc_c), f"{name}: behind a solve over other tables")
    assert tp_a.tobytes() != tp_c.tobytes()                     # (other leaders before: leaders_moved differs)
    assert (sc_a["reserved"] == 0).all() and (sc_c["reserved"] == 0).all()


def test_whatif_topics(ctx):
    """WhatIf.solve(topics=True, rows=False) over remove / add / rack-unaware variants, against the checker and the identities;
    with impact, with rows and with racks the same figures"""
    from kafka_assigner_amd.whatif import Variant, WhatIf
    w = WhatIf(*whatif_inputs())
    # (three new brokers: with one, two or six the reference's first fit strands a partition of this snapshot)
    variants = [Variant(remove=[3, 17], label="remove"), Variant(add={60: "r0", 61: "r1", 62: "r2"}, label="add"),
                Variant(remove=[3, 17], rack_aware=False, label="unaware")]
    fb = w.flat_batch(variants)
    res = w.solve(variants, topics=True, rows=False)
    assert all(r.status == abi.KAS_OK for r in res)
    ho = native.solve_host(fb, ctx)
    want = topic_ref(fb, ho)
    check_topic_identities(fb, ho, impact_ref(fb, ho), want)
    for s, r in enumerate(res):
        for f in abi.SCENARIO_TOPIC_FIELDS:
            assert getattr(r, f) == int(want[1][f][s]), (s, f)
        assert r.max_inbound is None and r.colocated_after is None
        tb = int(fb.scen["topic_begin"][s])
        ti = r.topic_impact()
        assert list(ti) == ["orders", "clicks"]
        for k, name in enumerate(ti):
            rec = {f: int(want[0][f][tb + k]) for f in abi.TOPIC_IMPACT_FIELDS}
            rec.update(status=abi.KAS_OK, moved_replicas=int(ho.topic_results["moved_replicas"][tb + k]),
                       moved_partitions=int(ho.topic_results["moved_partitions"][tb + k]))
            assert ti[name] == rec, (s, name)
        assert sum(v["moved_replicas"] for v in ti.values()) == r.moved_replicas
        assert r.topics_ok == 2 and r.max_topic_inbound > 0
        with pytest.raises(ValueError):
            r.assignment("orders")
    assert res[0].topics_departed == 2 and res[1].topics_departed == 0
    full = w.solve(variants, topics=True, impact=True, racks=True)
    lean = w.solve(variants, topics=True, impact=True, rows=False)
    for a, b, c in zip(res, full, lean):
        for f in abi.SCENARIO_TOPIC_FIELDS:
            assert getattr(a, f) == getattr(b, f) == getattr(c, f), f
        assert a.topic_impact() == b.topic_impact() == c.topic_impact()
        assert b.max_inbound == c.max_inbound is not None and b.colocated_after is not None and c.colocated_after is None
        assert b.assignment("orders") and b.max_topic_inbound <= b.max_inbound
    plain = w.solve(variants[:1], impact=True)                  # the defaults: today's behaviour
    assert plain[0].topics_ok is None and plain[0].max_inbound == full[0].max_inbound
    with pytest.raises(ValueError):
        plain[0].topic_impact()


def test_cli_print_topic_impact(tmp_path):
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
        plain = _run(cli, *args, *extra, "--print_impact", "--print_rack_impact")
        assert plain.returncode == 0 and "REASSIGNMENT TOPIC IMPACT" not in plain.stdout, plain.stderr
        r = _run(cli, *args, *extra, "--print_impact", "--print_rack_impact", "--print_topic_impact")
        assert r.returncode == 0, r.stderr
        head, tail = r.stdout.split("REASSIGNMENT TOPIC IMPACT:\n")
        assert head == plain.stdout                              # everything before it exactly as without the flag
        got = json.loads(tail)
        for flags in ((), ("--print_impact",)):                  # alone (no impact pass at all) and with the impact records
            alone = _run(cli, *args, *extra, *flags, "--print_topic_impact")
            assert alone.returncode == 0 and json.loads(alone.stdout.split("REASSIGNMENT TOPIC IMPACT:\n")[1]) == got, alone.stderr
            bare = _run(cli, *args, *extra, *flags)
            assert alone.stdout.split("REASSIGNMENT TOPIC IMPACT:\n")[0] == bare.stdout
        # the run solves its topics one by one under one Context: the oracle's solve of all of them in one scenario
        real = {b: racks[str(b)] for b in brokers}
        sc = Scenario(brokers=brokers, racks=real if rack_aware else {},
                      topics=[Topic(name, {int(p): v for p, v in C1["current"][t].items()}, 3) for t, name in enumerate(C1["topics"])])
        fb = flatten([sc])
        ho = oracle_solve(fb)
        want = topic_ref(fb, ho)
        assert [e["topic"] for e in got["topics"]] == list(C1["topics"])
        for k, e in enumerate(got["topics"]):
            assert {f: e[f] for f in abi.TOPIC_IMPACT_FIELDS} == {f: int(want[0][f][k]) for f in abi.TOPIC_IMPACT_FIELDS}, (k, e)
            assert e["moved_replicas"] == int(ho.topic_results["moved_replicas"][k])
            assert e["moved_partitions"] == int(ho.topic_results["moved_partitions"][k])
        assert got["summary"] == {f: int(want[1][f][0]) for f in abi.SCENARIO_TOPIC_FIELDS}

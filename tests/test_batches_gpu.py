"""Execution batches (include/kas_abi.h: kas_batch_spec / kas_move_batch / kas_scenario_batches / kas_batches) on the GPU, through the
C ABI, against the checker (tests/batches_ref.py) over the oracle's rows: the host form on int32 and 16-bit cells, the device form
behind a solve and a choice, a host call cut into scenario ranges, the counts of every what-if variant, WhatIf.solve / best / front.
"""
from types import SimpleNamespace

import numpy as np
import pytest

import test_choose_gpu as tg
from batches_ref import assert_same_batches, batches_ref, check_invariants, replay
from kafka_assigner_amd import abi, native
from test_choose_cpu import k_largest, whatif_solved
from test_moves_gpu import reference

pytestmark = pytest.mark.gpu

FILL = 0x5A5A5A5A
CAPS = ({"inbound": 1}, {"inbound": 3, "outbound": 2, "max_moves": 50}, {"inbound": 10 ** 6})
RESULT_FIELDS = ("status", "fail_topic", "fail_partition", "moved_replicas", "moved_partitions", "digest")


@pytest.fixture(scope="module")
def ctx():
    return native.DeviceContext(0)


def host_check(ctx, fb, cur, ho, select, caps, cells16, what, stride=None, want=None):
    """one kas_solve_host_batches / 16 call into arrays full of FILL, against the checker; returns (the checker's list, BatchList)"""
    listed = list(range(fb.n_scenarios)) if select is None else list(select)
    want = want or batches_ref(fb, ho, listed, caps, cells16=cells16, cur16=cur if cells16 else None)
    if stride is None:
        stride = max([w.record["n_batches"] for w in want if w is not None] + [1]) + 2
    got_ho, bl = native.solve_host_batches(fb, caps, select=select, stride=stride, cells16=cells16, ctx=ctx, fill=FILL)
    assert_same_batches(want, bl.scenarios, bl.batches, stride, fill=FILL, what=what)
    S = fb.n_scenarios
    for f in RESULT_FIELDS:                                         # the solve's records are the oracle's
        assert (got_ho.scenario_results[f][:S] == ho.scenario_results[f][:S]).all(), (what, f)
    for j, s in enumerate(listed):
        if want[j] is not None:
            check_invariants(want[j], caps, ho.scenario_results["moved_partitions"][s], ho.scenario_results["moved_replicas"][s], what=(what, j))
    return want, bl


@pytest.mark.parametrize("cells16", [False, True], ids=["int32", "cells16"])
@pytest.mark.parametrize("name", ["mixed42", "degenerate", "widths_4_5", "widths_6_8", "sparse", "many_brokers"])
def test_host_batches_on_the_named_batches(ctx, name, cells16):
    fb, cur, ho = reference(name, cells16)
    S = fb.n_scenarios
    moved = 0
    for caps in CAPS:                                               # (later calls find the plan of the first: other caps on the same plan)
        want, _ = host_check(ctx, fb, cur, ho, None, caps, cells16, (name, caps, cells16))
        moved += sum(w.record["n_moves"] for w in want)
    assert moved > 0
    # a list with an empty slot and a scenario listed twice; strides of exactly n_batches, one less (the guard stays), 0 with NULL
    select = [S - 1, -1, 0, S - 1]
    want, _ = host_check(ctx, fb, cur, ho, select, CAPS[0], cells16, (name, "list"))
    nb = max(w.record["n_batches"] for w in want if w is not None)
    for stride in (nb, max(nb - 1, 0), 0):
        _, bl = host_check(ctx, fb, cur, ho, select, CAPS[0], cells16, (name, "stride", stride), stride=stride, want=want)
        assert any(bl.truncated(j) for j in range(len(select))) == (stride < nb)
    a = native.solve_host_batches(fb, CAPS[1], select=select, stride=nb, cells16=cells16, ctx=ctx)[1]
    b = native.solve_host_batches(fb, CAPS[1], select=select, stride=nb, cells16=cells16, ctx=ctx)[1]
    assert a.scenarios.tobytes() == b.scenarios.tobytes() and a.batches.tobytes() == b.batches.tobytes()


def test_host_batches_refusals(ctx):
    fb, cur, ho = reference("degenerate", False)
    S = fb.n_scenarios
    for caps, select, stride, code in (({"inbound": -1}, [S], -1, abi.KAS_E_INVALID_ARG), ({}, [0], 4, abi.KAS_E_INVALID_ARG),
                                       ({"inbound": 1}, [0], -1, abi.KAS_E_INVALID_ARG), ({"inbound": 1}, [S], 4, abi.KAS_E_INVALID_ARG),
                                       ({"inbound": 1}, [-2], 4, abi.KAS_E_INVALID_ARG)):
        with pytest.raises(native.KasError) as e:
            native.solve_host_batches(fb, caps, select=select, stride=stride, ctx=ctx)
        assert e.value.code == code, (caps, select, stride, str(e.value))
    host_check(ctx, fb, cur, ho, [0], {"inbound": 1}, False, "after the refusals")


@pytest.mark.parametrize("cells16", [False, True], ids=["int32", "cells16"])
def test_device_batches_behind_a_choice_on_one_stream(ctx, cells16):
    """Plan + solve_device + impact_device + choose_device + batches_device three times on one plan (fed the device chosen[] with
    its -1 tail; a list of its own under other caps; the counts only) on one non-default torch stream, sentinel-filled outputs"""
    import torch
    fb, cur, ho = reference("mixed42", cells16)
    S = fb.n_scenarios
    k = S                                                         # (a scenario that fails leaves a -1 tail in chosen[])
    dev = torch.device("cuda", ctx.device)
    plan = native.Plan(ctx, fb, cells16=cells16)
    try:
        cdt = torch.int16 if cells16 else torch.int32
        d_cur = torch.from_numpy((cur.view(np.int16) if cells16 else cur).copy()).to(dev)
        d_aux = torch.from_numpy(fb.aux).to(dev) if fb.aux.size else None
        d_out = torch.full((max(fb.out_len, 1),), -2, dtype=cdt, device=dev)
        d_tr = torch.zeros(max(fb.n_topics, 1) * 16, dtype=torch.uint8, device=dev)
        d_sr = torch.zeros(max(S, 1) * 32, dtype=torch.uint8, device=dev)
        n_nodes = int(native.node_blocks(fb)[-1])
        d_nodes = torch.zeros(max(n_nodes, 1) * 32, dtype=torch.uint8, device=dev)
        d_scen = torch.zeros(max(S, 1) * 32, dtype=torch.uint8, device=dev)
        rows_cap, nodes_cap = k_largest(fb, k)
        d_rank = torch.zeros(S, dtype=torch.int32, device=dev)
        d_chosen = torch.full((k,), -9, dtype=torch.int32, device=dev)
        d_roff, d_noff = torch.zeros(k + 1, dtype=torch.int64, device=dev), torch.zeros(k + 1, dtype=torch.int64, device=dev)
        d_nok = torch.zeros(1, dtype=torch.int32, device=dev)
        d_rows = torch.zeros(rows_cap + 8, dtype=cdt, device=dev)
        d_cnodes = torch.zeros((nodes_cap + 1) * 32, dtype=torch.uint8, device=dev)
        own = [0, -1, S - 1, 0, S]                                # (S: no scenario of the tables, an empty slot on the device)
        d_own = torch.tensor(own, dtype=torch.int32, device=dev)
        c16 = dict(cells16=cells16, cur16=cur if cells16 else None)
        stride = 2 + max(w.record["n_batches"] for caps in CAPS[:2] for w in batches_ref(fb, ho, range(S), caps, **c16))   # room for every record
        runs = ((CAPS[0], d_chosen, k, stride), (CAPS[1], d_own, len(own), stride), (CAPS[0], d_own, len(own), 0))
        outs = [SimpleNamespace(scen=torch.full(((n + 1) * 8,), FILL, dtype=torch.int32, device=dev),
                                recs=torch.full(((n * st_ + 1) * 8,), FILL, dtype=torch.int32, device=dev)) for _, _, n, st_ in runs]
        st = torch.cuda.Stream(dev)
        st.wait_stream(torch.cuda.current_stream(dev))
        aux = d_aux.data_ptr() if d_aux is not None else 0
        plan.solve_device(d_cur.data_ptr(), d_out.data_ptr(), d_tr.data_ptr(), d_sr.data_ptr(), aux=aux, stream=st.cuda_stream)
        plan.impact_device(d_cur.data_ptr(), d_out.data_ptr(), d_tr.data_ptr(), d_nodes.data_ptr(), d_scen.data_ptr(), aux=aux, stream=st.cuda_stream)
        plan.choose_device(("moved_replicas", "leaders_moved"), k, d_out.data_ptr(), d_sr.data_ptr(), d_nodes.data_ptr(), d_scen.data_ptr(),
                           d_rank.data_ptr(), d_chosen.data_ptr(), d_roff.data_ptr(), d_noff.data_ptr(), d_nok.data_ptr(), d_rows.data_ptr(),
                           rows_cap, d_cnodes.data_ptr(), nodes_cap, stream=st.cuda_stream)
        for o, (caps, sel, n, st_) in zip(outs, runs):
            plan.batches_device(caps, sel.data_ptr(), n, d_cur.data_ptr(), d_out.data_ptr(), d_tr.data_ptr(), o.scen.data_ptr(),
                                o.recs.data_ptr() if st_ else 0, st_, aux=aux, stream=st.cuda_stream)
        st.synchronize()
        chosen = d_chosen.cpu().numpy()
        assert (chosen >= 0).any() and (chosen == -1).any() or (ho.scenario_results["status"][:S] == 0).all()
        for o, (caps, sel, n, st_) in zip(outs, runs):
            listed = chosen.tolist() if sel is d_chosen else own
            want = batches_ref(fb, ho, listed, caps, **c16)
            scen, recs = o.scen.cpu().numpy(), o.recs.cpu().numpy()
            assert (scen[8 * n:] == FILL).all() and (recs[8 * n * st_:] == FILL).all(), "written behind the arrays"
            assert_same_batches(want, scen[:8 * n].view(abi.SCENARIO_BATCHES_DTYPE), recs[:8 * n * st_].view(abi.MOVE_BATCH_DTYPE), st_, fill=FILL,
                                what=("device", caps, cells16))
    finally:
        plan.close()


def test_host_batches_over_scenario_ranges(ctx, monkeypatch):
    """44 x 100k x 200 brokers with a `cur` per scenario: the planner cuts the call into two ranges, then (KAS_HOST_RANGES) three;
    the pass runs behind every range's done event, for a list that names scenarios of both halves"""
    fb, ho, _, _ = tg._ranges_batch()
    S = fb.n_scenarios
    ok = np.nonzero(ho.scenario_results["status"][:S] == abi.KAS_OK)[0]
    lo, hi = ok[ok < S // 2], ok[ok >= S // 2]
    select = [int(hi[-1]), -1, int(lo[0]), int(hi[0]), int(hi[-1])]
    caps = {"inbound": 5}
    want = batches_ref(fb, ho, select, caps)
    assert all(w.record["n_batches"] >= 2 for w in want if w is not None)
    r = replay(want[0].moves, caps)
    assert r.groups >= 10 and r.replayed >= 1                      # lists of thousands of moves: many groups, and the replay
    hits = ctx.host_stats()[1]
    host_check(ctx, fb, fb.cur, ho, select, caps, False, "two ranges", want=want)
    host_check(ctx, fb, fb.cur, ho, select, caps, False, "two ranges again", want=want)
    assert ctx.host_stats()[1] - hits >= 2, "the call was not cut into two scenario ranges"
    monkeypatch.setenv("KAS_HOST_RANGES", "3")
    host_check(ctx, fb, fb.cur, ho, select, caps, False, "three ranges", want=want)
    hits = ctx.host_stats()[1]
    host_check(ctx, fb, fb.cur, ho, select, caps, False, "three ranges again", want=want)
    assert ctx.host_stats()[1] - hits == 3, "the call was not cut into three scenario ranges"


def test_counts_of_every_whatif_variant(ctx):
    """n_select < 0 with stride 0 and batches == NULL over the 302 variants: the counts only"""
    _, _, fb, ho, _ = whatif_solved()
    S = fb.n_scenarios
    for caps in ({"inbound": 5}, {"inbound": 1, "max_moves": 100}):
        want, bl = host_check(ctx, fb, fb.cur, ho, None, caps, False, ("what-if counts", caps), stride=0)
        assert bl.batches.size == 0 and sum(w.record["n_batches"] for w in want) >= 100
        solved = ho.scenario_results["status"][:S] == abi.KAS_OK
        assert (bl.scenarios["n_moves"][solved] == ho.scenario_results["moved_partitions"][:S][solved]).all()


def test_whatif_solve_best_and_front_with_batches(ctx):
    w, vs, fb, ho, _ = whatif_solved()
    caps = {"inbound": 5, "outbound": 0, "max_moves": 0}
    few = vs[:12]
    fbf = w.flat_batch(few)
    from oracle_lib import oracle_solve
    hof = oracle_solve(fbf)
    want = batches_ref(fbf, hof, range(len(few)), caps)
    res = w.solve(few, moves=("replicas", "leader", "order"), batches=caps, batch_room=64)
    moved = 0
    for s, r in enumerate(res):
        rec = want[s].record
        assert (r.n_batches, r.batch_moves, r.batch_replicas, r.max_batch_moves, r.max_batch_replicas) == \
            (rec["n_batches"], rec["n_moves"], rec["replicas"], rec["max_batch_moves"], rec["max_batch_replicas"]), r.label
        assert (r.closed_by_max_moves, r.closed_by_inbound, r.closed_by_outbound) == (0, rec["closed_by_inbound"], 0)
        bt = r.batches()
        assert len(bt) == min(rec["n_batches"], 64)
        for g, b in zip(bt, want[s].batches):
            assert g == dict(b, topic=w.topic_names[b["topic"]], closed_by=abi.BATCH_CLOSED_BY[b["closed_by"]])
        if r.n_batches <= 64:
            objs = r.reassignment_batches()
            assert len(objs) == max(r.n_batches, 1 if r.moves() else 0)
            assert [p for o in objs for p in o["partitions"]] == r.reassignment()["partitions"]
            flagged = [[(p["topic"], p["partition"]) for p in o["partitions"]] for o in r.reassignment_batches(kinds=("replicas",))]
            assert [len(f) for f in flagged] == [b["n_moves"] for b in bt]
            moved += len(bt)
    assert moved >= 10
    tight = w.solve(few[2:4], moves=("replicas",), batches={"max_moves": 1}, batch_room=2)
    assert any(r.n_batches > 2 for r in tight)
    for r in tight:
        if r.n_batches > 2:
            assert len(r.batches()) == 2
            with pytest.raises(ValueError):
                r.reassignment_batches()
    plain = w.solve(few)
    assert all(r.n_batches is None for r in plain)
    with pytest.raises(ValueError):
        plain[0].batches()
    # best() and front(): the winners' batches are those of the same variants in the full what-if batch
    for winners in (w.best(vs, k=3, by=("max_inbound", "moved_replicas"), moves=("replicas",), rows=False, batches=caps, batch_room=256),
                    w.front(vs, by=("moved_replicas", "replica_spread"), k=4, moves=("replicas",), rows=False, batches=caps, batch_room=256)):
        assert len(winners) >= 2
        ref = batches_ref(fb, ho, [r._index for r in winners], caps)
        for r, wnt in zip(winners, ref):
            assert r.n_batches == wnt.record["n_batches"] and r.batch_moves == wnt.record["n_moves"] == r.moved_partitions
            assert [b["n_moves"] for b in r.batches()] == [b["n_moves"] for b in wnt.batches]
            objs = r.reassignment_batches()
            assert [p for o in objs for p in o["partitions"]] == r.reassignment()["partitions"]

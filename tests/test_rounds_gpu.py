"""Packed rounds (include/kas_abi.h: kas_round_spec / kas_move_round / kas_scenario_rounds / kas_rounds) on the GPU, through the C ABI,
against the checker (tests/rounds_ref.py) over the oracle's rows: the host form on int32 and 16-bit cells, the device form behind a
choice and on a stream of its own, a host call cut into scenario ranges, the counts of every what-if variant, WhatIf.solve / best /
front.
"""
from types import SimpleNamespace

import numpy as np
import pytest

import test_choose_gpu as tg
from kafka_assigner_amd import abi, native
from rounds_ref import assert_same_rounds, check_invariants, rounds_ref, spec_of
from test_choose_cpu import k_largest, whatif_solved
from test_moves_gpu import reference

pytestmark = pytest.mark.gpu

FILL = 0x5A5A5A5A
CAPS = ({"inbound": 1}, {"inbound": 3, "outbound": 2}, {"outbound": 1}, {"inbound": 10 ** 6})
RESULT_FIELDS = ("status", "fail_topic", "fail_partition", "moved_replicas", "moved_partitions", "digest")


@pytest.fixture(scope="module")
def ctx():
    return native.DeviceContext(0)


def strides_for(want):
    return (max([w.record["n_rounds"] for w in want if w is not None] + [1]) + 2,
            max([w.record["n_moves"] for w in want if w is not None] + [1]) + 3)


def host_check(ctx, fb, cur, ho, select, caps, cells16, what, strides=None, want=None):
    """one kas_solve_host_rounds / 16 call into arrays full of FILL, against the checker; returns (the checker's list, RoundList)"""
    listed = list(range(fb.n_scenarios)) if select is None else list(select)
    want = want or rounds_ref(fb, ho, listed, caps, cells16=cells16, cur16=cur if cells16 else None)
    rs, ms = strides_for(want) if strides is None else strides
    got_ho, rl = native.solve_host_rounds(fb, caps, select=select, round_stride=rs, move_stride=ms, cells16=cells16, ctx=ctx, fill=FILL)
    assert_same_rounds(want, rl.scenarios, rl.rounds, rs, rl.round_of, ms, fill=FILL, what=what)
    S = fb.n_scenarios
    for f in RESULT_FIELDS:                                         # the solve's records are the oracle's
        assert (got_ho.scenario_results[f][:S] == ho.scenario_results[f][:S]).all(), (what, f)
    for j, s in enumerate(listed):
        if want[j] is not None:
            check_invariants(want[j], caps, ho.scenario_results["moved_partitions"][s], ho.scenario_results["moved_replicas"][s], what=(what, j))
    return want, rl


@pytest.mark.parametrize("cells16", [False, True], ids=["int32", "cells16"])
@pytest.mark.parametrize("name", ["mixed42", "degenerate", "widths_4_5", "widths_6_8", "sparse", "many_brokers"])
def test_host_rounds_on_the_named_batches(ctx, name, cells16):
    fb, cur, ho = reference(name, cells16)
    S = fb.n_scenarios
    moved = 0
    for caps in CAPS:                                               # (later calls find the plan of the first: other caps on the same plan)
        want, _ = host_check(ctx, fb, cur, ho, None, caps, cells16, (name, caps, cells16))
        moved += sum(w.record["n_moves"] for w in want)
    assert moved > 0
    # a list with an empty slot and a scenario listed twice; strides of exactly the counts, one less (the guard stays), 0 with NULL
    select = [S - 1, -1, 0, S - 1]
    want, _ = host_check(ctx, fb, cur, ho, select, CAPS[0], cells16, (name, "list"))
    nr = max(w.record["n_rounds"] for w in want if w is not None)
    nm = max(w.record["n_moves"] for w in want if w is not None)
    for rs, ms in ((nr, nm), (max(nr - 1, 0), max(nm - 1, 0)), (0, 0)):
        _, rl = host_check(ctx, fb, cur, ho, select, CAPS[0], cells16, (name, "strides", rs, ms), strides=(rs, ms), want=want)
        assert any(rl.truncated(j) for j in range(len(select))) == (rs < nr or ms < nm)
    a = native.solve_host_rounds(fb, CAPS[1], select=select, round_stride=nr, move_stride=nm, cells16=cells16, ctx=ctx)[1]
    b = native.solve_host_rounds(fb, CAPS[1], select=select, round_stride=nr, move_stride=nm, cells16=cells16, ctx=ctx)[1]
    assert a.scenarios.tobytes() == b.scenarios.tobytes() and a.rounds.tobytes() == b.rounds.tobytes() and a.round_of.tobytes() == b.round_of.tobytes()


def test_host_rounds_refusals(ctx):
    """the planner's refusals reach the caller with their codes (tests/test_rounds_cpu.py has their order and texts), and the
    context serves the next call"""
    fb, cur, ho = reference("degenerate", False)
    S = fb.n_scenarios
    for caps, select, rs, ms in (({"inbound": -1}, [S], -1, 0), ({}, [0], 4, 4), ({"inbound": 1, "policy": 1}, [0], 4, 4), ({"inbound": 1}, [0], -1, 4),
                                 ({"inbound": 1}, [0], 4, -1), ({"inbound": 1}, [S], 4, 4), ({"inbound": 1}, [-2], 4, 4)):
        with pytest.raises(native.KasError) as e:
            native.solve_host_rounds(fb, caps, select=select, round_stride=rs, move_stride=ms, ctx=ctx)
        assert e.value.code == abi.KAS_E_INVALID_ARG, (caps, select, rs, ms, str(e.value))
    host_check(ctx, fb, cur, ho, [0], {"inbound": 1}, False, "after the refusals")


def _device_tables(ctx, fb, cur, cells16):
    import torch
    dev = torch.device("cuda", ctx.device)
    S = fb.n_scenarios
    cdt = torch.int16 if cells16 else torch.int32
    d = SimpleNamespace(dev=dev, cdt=cdt)
    d.cur = torch.from_numpy((cur.view(np.int16) if cells16 else cur).copy()).to(dev)
    d.aux_t = torch.from_numpy(fb.aux).to(dev) if fb.aux.size else None
    d.aux = d.aux_t.data_ptr() if d.aux_t is not None else 0
    d.out = torch.full((max(fb.out_len, 1),), -2, dtype=cdt, device=dev)
    d.tr = torch.zeros(max(fb.n_topics, 1) * 16, dtype=torch.uint8, device=dev)
    d.sr = torch.zeros(max(S, 1) * 32, dtype=torch.uint8, device=dev)
    return d


def _device_outs(dev, n, rs, ms):
    import torch
    return SimpleNamespace(scen=torch.full(((n + 1) * 8,), FILL, dtype=torch.int32, device=dev),
                           recs=torch.full(((n * rs + 1) * 4,), FILL, dtype=torch.int32, device=dev),
                           rof=torch.full((n * ms + 1,), FILL, dtype=torch.int32, device=dev))


def _device_compare(o, want, n, rs, ms, what):
    scen, recs, rof = o.scen.cpu().numpy(), o.recs.cpu().numpy(), o.rof.cpu().numpy()
    assert (scen[8 * n:] == FILL).all() and (recs[4 * n * rs:] == FILL).all() and (rof[n * ms:] == FILL).all(), "written behind the arrays"
    assert_same_rounds(want, scen[:8 * n].view(abi.SCENARIO_ROUNDS_DTYPE), recs[:4 * n * rs].view(abi.MOVE_ROUND_DTYPE), rs, rof[:n * ms], ms,
                       fill=FILL, what=what)


@pytest.mark.parametrize("cells16", [False, True], ids=["int32", "cells16"])
def test_device_rounds_behind_a_choice_on_one_stream(ctx, cells16):
    """Plan + solve_device + impact_device + choose_device + rounds_device three times on one plan (fed the device chosen[] with its
    -1 tail; a list of its own under other caps; the counts only) on one non-default torch stream, sentinel-filled outputs"""
    import torch
    fb, cur, ho = reference("mixed42", cells16)
    S = fb.n_scenarios
    k = S                                                         # (a scenario that fails leaves a -1 tail in chosen[])
    plan = native.Plan(ctx, fb, cells16=cells16)
    try:
        d = _device_tables(ctx, fb, cur, cells16)
        dev = d.dev
        n_nodes = int(native.node_blocks(fb)[-1])
        d_nodes = torch.zeros(max(n_nodes, 1) * 32, dtype=torch.uint8, device=dev)
        d_scen = torch.zeros(max(S, 1) * 32, dtype=torch.uint8, device=dev)
        rows_cap, nodes_cap = k_largest(fb, k)
        d_rank = torch.zeros(S, dtype=torch.int32, device=dev)
        d_chosen = torch.full((k,), -9, dtype=torch.int32, device=dev)
        d_roff, d_noff = torch.zeros(k + 1, dtype=torch.int64, device=dev), torch.zeros(k + 1, dtype=torch.int64, device=dev)
        d_nok = torch.zeros(1, dtype=torch.int32, device=dev)
        d_rows = torch.zeros(rows_cap + 8, dtype=d.cdt, device=dev)
        d_cnodes = torch.zeros((nodes_cap + 1) * 32, dtype=torch.uint8, device=dev)
        own = [0, -1, S - 1, 0, S]                                # (S: no scenario of the tables, an empty slot on the device)
        d_own = torch.tensor(own, dtype=torch.int32, device=dev)
        c16 = dict(cells16=cells16, cur16=cur if cells16 else None)
        every = [w for caps in CAPS[:2] for w in rounds_ref(fb, ho, range(S), caps, **c16)]
        rs, ms = strides_for(every)                               # room for every record
        runs = ((CAPS[0], d_chosen, k, rs, ms), (CAPS[1], d_own, len(own), rs, ms), (CAPS[0], d_own, len(own), 0, 0))
        outs = [_device_outs(dev, n, r_, m_) for _, _, n, r_, m_ in runs]
        st = torch.cuda.Stream(dev)
        st.wait_stream(torch.cuda.current_stream(dev))
        plan.solve_device(d.cur.data_ptr(), d.out.data_ptr(), d.tr.data_ptr(), d.sr.data_ptr(), aux=d.aux, stream=st.cuda_stream)
        plan.impact_device(d.cur.data_ptr(), d.out.data_ptr(), d.tr.data_ptr(), d_nodes.data_ptr(), d_scen.data_ptr(), aux=d.aux, stream=st.cuda_stream)
        plan.choose_device(("moved_replicas", "leaders_moved"), k, d.out.data_ptr(), d.sr.data_ptr(), d_nodes.data_ptr(), d_scen.data_ptr(),
                           d_rank.data_ptr(), d_chosen.data_ptr(), d_roff.data_ptr(), d_noff.data_ptr(), d_nok.data_ptr(), d_rows.data_ptr(),
                           rows_cap, d_cnodes.data_ptr(), nodes_cap, stream=st.cuda_stream)
        for o, (caps, sel, n, r_, m_) in zip(outs, runs):
            plan.rounds_device(caps, sel.data_ptr(), n, d.cur.data_ptr(), d.out.data_ptr(), d.tr.data_ptr(), o.scen.data_ptr(),
                               o.recs.data_ptr() if r_ else 0, r_, o.rof.data_ptr() if m_ else 0, m_, aux=d.aux, stream=st.cuda_stream)
        st.synchronize()
        chosen = d_chosen.cpu().numpy()
        assert (chosen >= 0).any() and (chosen == -1).any() or (ho.scenario_results["status"][:S] == 0).all()
        for o, (caps, sel, n, r_, m_) in zip(outs, runs):
            listed = chosen.tolist() if sel is d_chosen else own
            _device_compare(o, rounds_ref(fb, ho, listed, caps, **c16), n, r_, m_, ("device", caps, cells16))
    finally:
        plan.close()


def test_device_rounds_on_a_stream_of_its_own_then_a_solve(ctx):
    """solve on stream A, the rounds pass on stream B (it waits for the solve), then a solve on A into the SAME out table full of a
    sentinel: that solve must wait for the pass, which would otherwise read rows half written"""
    import torch
    fb, cur, ho = reference("widths_4_5", False)
    S = fb.n_scenarios
    plan = native.Plan(ctx, fb)
    try:
        d = _device_tables(ctx, fb, cur, False)
        caps = {"inbound": 1}
        want = rounds_ref(fb, ho, range(S), caps)
        rs, ms = strides_for(want)
        o = _device_outs(d.dev, S, rs, ms)
        d_sel = torch.arange(S, dtype=torch.int32, device=d.dev)
        sa, sb = torch.cuda.Stream(d.dev), torch.cuda.Stream(d.dev)
        sa.wait_stream(torch.cuda.current_stream(d.dev))
        sb.wait_stream(torch.cuda.current_stream(d.dev))
        plan.solve_device(d.cur.data_ptr(), d.out.data_ptr(), d.tr.data_ptr(), d.sr.data_ptr(), aux=d.aux, stream=sa.cuda_stream)
        plan.rounds_device(caps, d_sel.data_ptr(), S, d.cur.data_ptr(), d.out.data_ptr(), d.tr.data_ptr(), o.scen.data_ptr(), o.recs.data_ptr(), rs,
                           o.rof.data_ptr(), ms, aux=d.aux, stream=sb.cuda_stream)
        plan.solve_device(d.cur.data_ptr(), d.out.data_ptr(), d.tr.data_ptr(), d.sr.data_ptr(), aux=d.aux, stream=sa.cuda_stream)
        sa.synchronize()
        sb.synchronize()
        _device_compare(o, want, S, rs, ms, "a stream of its own")
        sr = np.frombuffer(d.sr.cpu().numpy().tobytes(), abi.SCENARIO_RESULT_DTYPE)[:S]
        for f in RESULT_FIELDS:
            assert (sr[f] == ho.scenario_results[f][:S]).all(), f
    finally:
        plan.close()


def test_host_rounds_over_scenario_ranges(ctx, monkeypatch):
    """44 x 100k x 200 brokers with a `cur` per scenario: the planner cuts the call into two ranges, then (KAS_HOST_RANGES) three;
    the pass runs behind every range's done event, for a list that names scenarios of both halves.  Lists of thousands of moves:
    the walk crosses many tiles on hardware"""
    fb, ho, _, _ = tg._ranges_batch()
    S = fb.n_scenarios
    ok = np.nonzero(ho.scenario_results["status"][:S] == abi.KAS_OK)[0]
    lo, hi = ok[ok < S // 2], ok[ok >= S // 2]
    select = [int(hi[-1]), -1, int(lo[0]), int(hi[0]), int(hi[-1])]
    caps = {"inbound": 5}
    want = rounds_ref(fb, ho, select, caps)
    assert all(w.record["n_rounds"] >= 2 and w.record["n_moves"] > 1280 for w in want if w is not None)
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
    """n_select < 0 with both strides 0 and NULL arrays over the 302 variants: the counts only"""
    _, _, fb, ho, _ = whatif_solved()
    S = fb.n_scenarios
    for caps in ({"inbound": 5}, {"inbound": 1, "outbound": 2}):
        want, rl = host_check(ctx, fb, fb.cur, ho, None, caps, False, ("what-if counts", caps), strides=(0, 0))
        assert rl.rounds.size == 0 and rl.round_of.size == 0 and sum(w.record["n_rounds"] for w in want) >= 100
        solved = ho.scenario_results["status"][:S] == abi.KAS_OK
        assert (rl.scenarios["n_moves"][solved] == ho.scenario_results["moved_partitions"][:S][solved]).all()


def _caps_hold(w, v, r, caps):
    """every round respects the caps, recomputed from the rows the result returns: In / Out of a replica move from its new replica
    list against the plan's current one (a lost replica on a broker the variant removes is in neither set)"""
    sp = spec_of(caps)
    mv = r.moves(kinds=("replicas",))
    members = [rd["moves"] for rd in r.rounds()]
    assert sorted(i for m in members for i in m) == list(range(len(mv)))
    live = (set(w.brokers) - set(v.remove)) | set(v.add)
    row_of = [{int(p): i for i, p in enumerate(pids)} for pids in w.part_ids]
    for m in members:
        cin, cout = {}, {}
        for i in m:
            name, p, reps, _ = mv[i]
            t = w.topic_names.index(name)
            at = int(w.cur_off[t]) + row_of[t][p] * max(w.widths[t], 1)
            before = {int(b) for b in w.cur[at:at + w.widths[t]]}
            for b in (set(reps) - before) & live:
                cin[b] = cin.get(b, 0) + 1
            for b in (before - set(reps)) & live:
                cout[b] = cout.get(b, 0) + 1
        assert not sp.inbound or max(cin.values(), default=0) <= sp.inbound, (r.label, cin)
        assert not sp.outbound or max(cout.values(), default=0) <= sp.outbound, (r.label, cout)


def test_whatif_solve_best_and_front_with_rounds(ctx):
    w, vs, fb, ho, _ = whatif_solved()
    caps = {"inbound": 5, "outbound": 0}
    few = vs[:12]
    fbf = w.flat_batch(few)
    from oracle_lib import oracle_solve
    hof = oracle_solve(fbf)
    want = rounds_ref(fbf, hof, range(len(few)), caps)
    res = w.solve(few, moves=("replicas", "leader", "order"), rounds=caps, round_room=512)
    key = lambda p: (p["topic"], p["partition"])
    scheduled = 0
    for s, r in enumerate(res):
        rec = want[s].record
        assert (r.n_rounds, r.round_moves, r.round_replicas, r.max_round_moves, r.max_round_replicas, r.raised_by_inbound, r.raised_by_outbound) == \
            (rec["n_rounds"], rec["n_moves"], rec["replicas"], rec["max_round_moves"], rec["max_round_replicas"], rec["raised_by_inbound"], 0), r.label
        rd = r.rounds()
        assert len(rd) == rec["n_rounds"]
        for k_, (g, b) in enumerate(zip(rd, want[s].rounds)):
            assert g == dict(n_moves=b["n_moves"], replicas=b["replicas"], first_move=b["first_move"],
                             moves=[i for i, x in enumerate(want[s].round_of) if x == k_])
        _caps_hold(w, few[s], r, caps)
        objs = r.reassignment_rounds()
        assert len(objs) == max(r.n_rounds, 1 if r.moves() else 0)
        assert sorted((p for o in objs for p in o["partitions"]), key=key) == sorted(r.reassignment()["partitions"], key=key)
        assert [len(o["partitions"]) for o in r.reassignment_rounds(kinds=("replicas",))] == [g["n_moves"] for g in rd]
        split = r.reassignment_rounds(kinds=("replicas",), max_moves=7)
        assert all(1 <= len(o["partitions"]) <= 7 for o in split) and len(split) == sum(-(-g["n_moves"] // 7) for g in rd)
        assert [p for o in split for p in o["partitions"]] == [p for o in r.reassignment_rounds(kinds=("replicas",)) for p in o["partitions"]]
        scheduled += len(rd)
    assert scheduled >= 10
    tight = w.solve(few[2:4], moves=("replicas",), rounds={"inbound": 1}, round_room=2)
    assert any(r.n_rounds > 2 for r in tight)
    for r in tight:
        if r.n_rounds > 2:
            for f in (r.rounds, r.reassignment_rounds):
                with pytest.raises(ValueError):
                    f()
    plain = w.solve(few, moves=("replicas",))
    assert all(r.n_rounds is None for r in plain)
    for f in (plain[0].rounds, plain[0].reassignment_rounds):
        with pytest.raises(ValueError):
            f()
    with pytest.raises(ValueError):
        w.solve(few[:2], moves=("leader",), rounds=caps)[0].reassignment_rounds()    # the rounds index the replica move list
    # best() and front(): the winners' rounds are those of the same variants in the full what-if batch
    for winners in (w.best(vs, k=3, by=("max_inbound", "moved_replicas"), moves=("replicas",), rows=False, rounds=caps, round_room=512),
                    w.front(vs, by=("moved_replicas", "replica_spread"), k=4, moves=("replicas",), rows=False, rounds=caps, round_room=512)):
        assert len(winners) >= 2
        ref = rounds_ref(fb, ho, [r._index for r in winners], caps)
        for r, wnt in zip(winners, ref):
            assert r.n_rounds == wnt.record["n_rounds"] and r.round_moves == wnt.record["n_moves"] == r.moved_partitions
            assert [g["n_moves"] for g in r.rounds()] == [b["n_moves"] for b in wnt.rounds]
            objs = r.reassignment_rounds()
            assert sorted((p for o in objs for p in o["partitions"]), key=key) == sorted(r.reassignment()["partitions"], key=key)
            assert [len(o["partitions"]) for o in objs] == [b["n_moves"] for b in wnt.rounds]
            _caps_hold(w, vs[r._index], r, caps)
    both = {"inbound": 2, "outbound": 2}
    for v, r in zip(few[:4], w.solve(few[:4], moves=("replicas",), rounds=both, round_room=2048)):
        _caps_hold(w, v, r, both)

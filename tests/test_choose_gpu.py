"""Choosing the best scenarios on the MI355X (kas_rank_device, kas_choose_device / 16, kas_solve_host_choose / 16, WhatIf.best),
against the NumPy checker of tests/choose_ref.py."""
import ctypes as C
import time

import numpy as np
import pytest

from choose_ref import assert_same_choice, choose_ref, rank_ref
from impact_batches import solved
from impact_ref import assert_same_impact, impact_ref
from kafka_assigner_amd import abi, native
from kafka_assigner_amd import generator as G
from kafka_assigner_amd.flatten import batch_desc, host_tables, index_form, node_set_batch, to_cells16
from oracle_lib import oracle_solve
from test_choose_cpu import MULTI_SPECS, S_VALUES, SENTINEL, WHATIF_SPECS, k_largest, own_cur_form, synthetic, whatif_solved

pytestmark = pytest.mark.gpu

RESULT_FIELDS = ("status", "fail_topic", "fail_partition", "moved_replicas", "moved_partitions", "digest")


@pytest.fixture(scope="module")
def ctx():
    return native.DeviceContext(0)


# ---- synthetic ranks ------------------------------------------------------------------------------------------------------
def _rank_device(ctx, sr, si, keys, k):
    import torch
    dev = torch.device("cuda", ctx.device)
    S = int(sr.shape[0])
    d_sr = torch.from_numpy(sr.view(np.uint8).copy()).to(dev)
    d_si = torch.from_numpy(si.view(np.uint8).copy()).to(dev)
    d_rank = torch.full((S + 1,), SENTINEL, dtype=torch.int32, device=dev)
    d_chosen = torch.full((k + 1,), SENTINEL, dtype=torch.int32, device=dev)
    d_nok = torch.full((2,), SENTINEL, dtype=torch.int32, device=dev)
    st = torch.cuda.Stream(dev)
    st.wait_stream(torch.cuda.current_stream(dev))
    native.rank_device(d_sr.data_ptr(), d_si.data_ptr(), S, keys, k, d_rank.data_ptr(), d_chosen.data_ptr(), d_nok.data_ptr(),
                       stream=st.cuda_stream, ctx=ctx)
    st.synchronize()
    rank, chosen, nok = d_rank.cpu().numpy(), d_chosen.cpu().numpy(), d_nok.cpu().numpy()
    assert rank[S] == SENTINEL and chosen[k] == SENTINEL and nok[1] == SENTINEL     # (nothing behind the arrays is written)
    return rank[:S], chosen[:k], int(nok[0])


@pytest.mark.parametrize("S", S_VALUES + [5000])
def test_rank_device_on_synthetic_records(ctx, S):
    """criteria drawn from {0..3} ({0..7} at S = 5,000): most scenarios tie and the index decides; every second scenario failed,
    none, all; k at 0, around n_ok and at S"""
    values = 8 if S == 5000 else 4
    for failed, keys in (("random", MULTI_SPECS[2]), ("alternate", ("max_inbound",)), ("none", MULTI_SPECS[0]), ("all", ("leader_spread",))):
        sr, si = synthetic(S, 11, values=values, failed=failed)
        n_ok = int((sr["status"] == 0).sum())
        for k in sorted({k for k in (0, 1, n_ok - 1, n_ok, n_ok + 1, S) if 0 <= k <= S}):
            want = rank_ref(sr, si, keys, k)
            rank, chosen, nok = _rank_device(ctx, sr, si, keys, k)
            assert nok == want.n_ok and np.array_equal(rank, want.rank) and np.array_equal(chosen, want.chosen), (S, failed, keys, k)
    sr, si = synthetic(S, 12, values=[0, 2**31 - 1], failed="alternate")
    for keys in [(name,) for name in abi.KEY_NAMES]:
        want = rank_ref(sr, si, keys, S)
        rank, chosen, nok = _rank_device(ctx, sr, si, keys, S)
        assert nok == want.n_ok and np.array_equal(rank, want.rank) and np.array_equal(chosen, want.chosen), (S, keys)


def test_rank_device_refuses_bad_specs(ctx):
    import torch
    d = torch.zeros(64, dtype=torch.int32, device=torch.device("cuda", ctx.device))
    p = d.data_ptr()
    for keys, k, text in (((), 1, "n_keys"), (("moved_replicas",) * 5, 1, "n_keys"), ((10,), 1, "unknown criterion"), ((0,), -1, "k outside"),
                          ((0,), 3, "k outside")):
        with pytest.raises(native.KasError) as e:
            native.rank_device(p, p, 2, keys, k, p, p, p, ctx=ctx)
        assert e.value.code == abi.KAS_E_INVALID_ARG and text in e.value.detail, e.value.detail


# ---- the host call --------------------------------------------------------------------------------------------------------
def _reference(fb, ho, cells16):
    """(scenario records, out pool with every row in place) the host call of this cell width must reproduce: the oracle's solve,
    of the batch's index form for 16-bit cells"""
    if not cells16:
        return ho.scenario_results, ho.out
    h = oracle_solve(index_form(fb))
    return h.scenario_results, np.where(h.out < 0, abi.KAS_CELL16_NONE, h.out).astype(np.uint16)


_WHATIF16 = None


def _whatif16():
    """the what-if batch with a cur table per variant, and the oracle's solve of its index form: (fb, records, uint16 out pool)"""
    global _WHATIF16
    if _WHATIF16 is None:
        fb = own_cur_form(whatif_solved()[2])
        _WHATIF16 = (fb,) + _reference(fb, None, True)
    return _WHATIF16


def _check_host_choice(ctx, fb, sr, out, imp, keys, k, cells16, what):
    S = fb.n_scenarios
    got_ho, got = native.solve_host_choose(fb, keys, k, cells16=cells16, ctx=ctx)
    assert_same_choice(choose_ref(fb, sr, out, imp, keys, k), got, what)
    for f in RESULT_FIELDS:
        assert (got_ho.scenario_results[f][:S] == sr[f][:S]).all(), (what, f)
    for f in abi.SCENARIO_IMPACT_FIELDS:
        assert (got.scenarios[f] == imp[1][f]).all(), (what, f)
    return got_ho, got


@pytest.mark.parametrize("cells16", [False, True], ids=["int32", "cells16"])
@pytest.mark.parametrize("spec", range(len(WHATIF_SPECS)))
def test_whatif_host_call_with_variants_that_fail_and_tie(ctx, spec, cells16):
    """302 variants of one snapshot, 118 of which fail and most of which tie (whatif_solved holds the guard): rank, chosen,
    offsets, n_ok, packed rows, node blocks, every scenario record and every scenario impact record against the checker over the
    oracle's solve; and the records of kas_solve_host_impact on the same context are the same"""
    _, _, fb, ho, imp = whatif_solved()
    keys = WHATIF_SPECS[spec]
    if cells16:                                                  # (one cur table per variant: the shared one has no 16-bit form)
        fb, sr, out = _whatif16()
        assert np.array_equal(sr["status"], ho.scenario_results["status"]) and np.array_equal(sr["moved_replicas"], ho.scenario_results["moved_replicas"])
    else:
        sr, out = ho.scenario_results, ho.out
    n_ok = int((ho.scenario_results["status"][:fb.n_scenarios] == 0).sum())
    assert n_ok >= 100 and fb.n_scenarios == 302
    for k in (1, 5, 184, 185, 302):
        got_ho, got = _check_host_choice(ctx, fb, sr, out, imp, keys, k, cells16, f"what-if {keys} k {k} cells16 {cells16}")
    old_ho, old_nodes, old_scen = native.solve_host_impact(fb, select=[], cells16=cells16, ctx=ctx)
    for f in RESULT_FIELDS:
        assert (old_ho.scenario_results[f] == got_ho.scenario_results[f]).all(), f
    for f in ("status", "fail_partition", "moved_replicas", "moved_partitions"):
        assert (old_ho.topic_results[f] == got_ho.topic_results[f]).all(), f
    assert_same_impact(imp, (old_nodes, old_scen), "kas_solve_host_impact behind the new call")
    assert_same_impact((imp[0], got.scenarios), (old_nodes, old_scen), "scenario impact of the two calls")


@pytest.mark.parametrize("cells16", [False, True], ids=["int32", "cells16"])
@pytest.mark.parametrize("name", ["mixed42", "row_counts", "degenerate", "widths_4_5"])
def test_host_call_on_the_named_batches(ctx, name, cells16):
    """multi-topic scenarios of odd sizes, a scenario without topics and one that fails, and lists 5 wide — which a 16-bit call
    solves on int32 cells and still returns as 16-bit rows (the narrowing gather); every k from 0 to S"""
    fb, ho, imp = solved(name)
    sr, out = _reference(fb, ho, cells16)
    for k in range(fb.n_scenarios + 1):
        _check_host_choice(ctx, fb, sr, out, imp, ("max_inbound", "moved_replicas"), k, cells16, f"{name} k {k} cells16 {cells16}")


def test_host_call_refusals(ctx):
    fb, _, _ = solved("mixed42")
    with pytest.raises(native.KasError) as e:
        native.solve_host_choose(fb, ("moved_replicas",), fb.n_scenarios + 1, ctx=ctx)
    assert e.value.code == abi.KAS_E_INVALID_ARG and "k outside" in e.value.detail
    with pytest.raises(ValueError):
        native.solve_host_choose(fb, ("nonsense",), 1, ctx=ctx)
    # capacities one below the k-largest bound, and a NULL array, straight at the ABI
    L = native.load()
    bd = batch_desc(fb)
    t, ho = host_tables(fb, out_len=0)
    t.out = None
    rows, nodes = k_largest(fb, 2)
    S = fb.n_scenarios
    a = dict(rank=np.zeros(S, np.int32), chosen=np.zeros(2, np.int32), row_off=np.zeros(3, np.int64), node_off=np.zeros(3, np.int64),
             n_ok=np.zeros(1, np.int32), rows=np.zeros(rows, np.int32), nodes=np.zeros(nodes, abi.NODE_IMPACT_DTYPE))
    scen = np.zeros(S, abi.SCENARIO_IMPACT_DTYPE)
    imp = abi.ImpactTables(None, scen.ctypes.data)
    spec = abi.choose_spec(("moved_replicas",), 2)

    def call(rows_cap=rows, nodes_cap=nodes, null=None):
        p = {n: (None if n == null else v.ctypes.data) for n, v in a.items()}
        ch = abi.Choice(p["rank"], p["chosen"], p["row_off"], p["node_off"], p["n_ok"], p["rows"], rows_cap, p["nodes"], nodes_cap)
        rc = L.kas_solve_host_choose(ctx._h, C.byref(bd), C.byref(t), C.byref(spec), C.byref(ch), C.byref(imp))
        return rc, (L.kas_last_error() or b"").decode()
    assert call()[0] == 0
    rc, err = call(rows_cap=rows - 1)
    assert rc == abi.KAS_E_INVALID_ARG and "rows_cap below" in err
    rc, err = call(nodes_cap=nodes - 1)
    assert rc == abi.KAS_E_INVALID_ARG and "nodes_cap below" in err
    for n in a:
        rc, err = call(null=n)
        assert rc == abi.KAS_E_INVALID_ARG and "is NULL" in err, (n, err)


# ---- the device path ------------------------------------------------------------------------------------------------------
def _device_choose_twice(ctx, fb, cells16, specs):
    """Plan + solve_device + impact_device + choose_device (twice, one spec each, outputs of their own) on one non-default torch
    stream: (HostOutputs, (nodes, scenarios), [choice per spec])"""
    import torch
    from types import SimpleNamespace
    dev = torch.device("cuda", ctx.device)
    plan = native.Plan(ctx, fb, cells16=cells16)
    try:
        _, ho = host_tables(fb)
        S = fb.n_scenarios
        cur = to_cells16(fb).view(np.int16) if cells16 else fb.cur
        d_cur = torch.from_numpy(cur.copy()).to(dev)
        d_aux = torch.from_numpy(fb.aux).to(dev) if fb.aux.size else None
        d_out = torch.full((max(fb.out_len, 1),), -2, dtype=torch.int16 if cells16 else torch.int32, device=dev)
        d_tr = torch.zeros(max(fb.n_topics, 1) * 16, dtype=torch.uint8, device=dev)
        d_sr = torch.zeros(max(S, 1) * 32, dtype=torch.uint8, device=dev)
        n_nodes = int(native.node_blocks(fb)[-1])
        d_nodes = torch.full((max(n_nodes, 1) * 32,), 0x5A, dtype=torch.uint8, device=dev)
        d_scen = torch.full((max(S, 1) * 32,), 0x5A, dtype=torch.uint8, device=dev)
        st = torch.cuda.Stream(dev)
        st.wait_stream(torch.cuda.current_stream(dev))
        aux = d_aux.data_ptr() if d_aux is not None else 0
        plan.solve_device(d_cur.data_ptr(), d_out.data_ptr(), d_tr.data_ptr(), d_sr.data_ptr(), aux=aux, stream=st.cuda_stream)
        plan.impact_device(d_cur.data_ptr(), d_out.data_ptr(), d_tr.data_ptr(), d_nodes.data_ptr(), d_scen.data_ptr(), aux=aux,
                           stream=st.cuda_stream)
        held = []
        for keys, k in specs:
            rows_cap, nodes_cap = k_largest(fb, k)
            d = SimpleNamespace(rank=torch.full((S,), SENTINEL, dtype=torch.int32, device=dev),
                                chosen=torch.full((max(k, 1),), SENTINEL, dtype=torch.int32, device=dev),
                                row_off=torch.full((k + 1,), SENTINEL, dtype=torch.int64, device=dev),
                                node_off=torch.full((k + 1,), SENTINEL, dtype=torch.int64, device=dev),
                                n_ok=torch.full((1,), SENTINEL, dtype=torch.int32, device=dev),
                                rows=torch.full((rows_cap + 64,), 0x7B7B, dtype=torch.int16 if cells16 else torch.int32, device=dev),
                                nodes=torch.full(((nodes_cap + 2) * 32,), 0x7B, dtype=torch.uint8, device=dev))
            plan.choose_device(keys, k, d_out.data_ptr(), d_sr.data_ptr(), d_nodes.data_ptr(), d_scen.data_ptr(), d.rank.data_ptr(),
                               d.chosen.data_ptr(), d.row_off.data_ptr(), d.node_off.data_ptr(), d.n_ok.data_ptr(), d.rows.data_ptr(),
                               rows_cap, d.nodes.data_ptr(), nodes_cap, stream=st.cuda_stream)
            held.append((d, k, rows_cap, nodes_cap))
        st.synchronize()
        ho.out = d_out.cpu().numpy().view(np.uint16) if cells16 else d_out.cpu().numpy()
        ho.scenario_results = d_sr.cpu().numpy().view(abi.SCENARIO_RESULT_DTYPE)
        imp = (d_nodes.cpu().numpy().view(abi.NODE_IMPACT_DTYPE)[:n_nodes], d_scen.cpu().numpy().view(abi.SCENARIO_IMPACT_DTYPE)[:S])
        got = []
        for d, k, rows_cap, nodes_cap in held:
            rows = d.rows.cpu().numpy().view(np.uint16 if cells16 else np.int32)
            raw = d.nodes.cpu().numpy()
            g = SimpleNamespace(rank=d.rank.cpu().numpy(), chosen=d.chosen.cpu().numpy()[:k], row_off=d.row_off.cpu().numpy(),
                                node_off=d.node_off.cpu().numpy(), n_ok=int(d.n_ok.cpu().numpy()[0]), rows=rows,
                                nodes=raw.view(abi.NODE_IMPACT_DTYPE))
            used, recs = int(g.row_off[k]), int(g.node_off[k])
            assert 0 <= used <= rows_cap and 0 <= recs <= nodes_cap
            assert (rows[used:] == 0x7B7B).all() and (raw[32 * recs:] == 0x7B).all(), "written behind the offsets / the capacities"
            got.append(g)
        return ho, imp, got
    finally:
        plan.close()


@pytest.mark.parametrize("cells16", [False, True], ids=["int32", "cells16"])
@pytest.mark.parametrize("name", ["rows_10000", "mixed42"])
def test_device_choice_twice_on_one_plan(ctx, name, cells16):
    fb, _, want_imp = solved(name)
    S = fb.n_scenarios
    specs = [(("moved_replicas", "leaders_moved"), S), (("max_outbound", "replica_spread", "moved_partitions"), max(S - 1, 1))]
    ho, imp, got = _device_choose_twice(ctx, fb, cells16, specs)
    assert_same_impact(want_imp, imp, f"{name}: the impact pass the choice reads")
    for (keys, k), g in zip(specs, got):
        assert_same_choice(choose_ref(fb, ho.scenario_results, ho.out, want_imp, keys, k), g, f"{name} cells16 {cells16} {keys} k {k}")


# ---- a call cut into scenario ranges --------------------------------------------------------------------------------------
_RANGES = None


def _ranges_batch():
    """44 x 100k x 200 brokers with a `cur` per scenario, solved by the oracle once: (fb, HostOutputs, (nodes, scenarios) of the
    checker, the out pool as uint16 node indices)"""
    global _RANGES
    if _RANGES is None:
        S, P, N, R = 44, 100_000, 200, 10
        cur = np.stack([G.random_assignment(60 + s, P, N, R, 3) for s in range(S)])
        sets = [G.scenario_action(61, s, N, R, actions=G.BENCH_ACTIONS)[1] for s in range(S)]
        fb = node_set_batch([b.node_id for b in sets], [b.node_rack for b in sets], P, 3, 3, cur=cur)
        ho = oracle_solve(fb)
        out16 = np.full(ho.out.shape, abi.KAS_CELL16_NONE, np.uint16)
        for s in range(S):                                      # (a scenario's ids ascend: a cell's node index is its id's position)
            td = fb.topics[int(fb.scen["topic_begin"][s])]
            lo, n = int(td["out_off"]), int(td["n_partitions"]) * int(td["out_width"])
            ids = fb.node_id[int(fb.scen["node_off"][s]):][:int(fb.scen["n_nodes"][s])]
            cells = ho.out[lo:lo + n]
            out16[lo:lo + n] = np.where(cells >= 0, np.searchsorted(ids, cells), abi.KAS_CELL16_NONE)
        _RANGES = (fb, ho, impact_ref(fb, ho), out16)
    return _RANGES


@pytest.mark.parametrize("S", [40, 44])
def test_host_call_over_scenario_ranges(ctx, S):
    """test_host_path_cut_into_ranges' shape, S x 100k x 200 brokers with a `cur` per scenario (40: its tables as given there; 44:
    the 52.8 MB of cur alone, all a choice uploads, are cut into two ranges — tests/test_choose_cpu.py pins both counts; the
    first 40 scenarios of the 44 are the batch of 40): the ranking spans the whole call and the three winners' rows and node
    blocks are the checker's over the oracle's solve, in int32 and in 16-bit cells"""
    fb44, ho, (nodes, scen), out16 = _ranges_batch()
    P = 100_000
    sl = lambda a: a[int(fb44.scen["node_off"][0]):int(fb44.scen["node_off"][S - 1]) + int(fb44.scen["n_nodes"][S - 1])]
    fb = node_set_batch([fb44.node_id[int(o):int(o) + int(n)] for o, n in zip(fb44.scen["node_off"][:S], fb44.scen["n_nodes"][:S])],
                        [fb44.node_rack[int(o):int(o) + int(n)] for o, n in zip(fb44.scen["node_off"][:S], fb44.scen["n_nodes"][:S])],
                        P, 3, 3, cur=fb44.cur.reshape(44, P, 3)[:S])
    assert np.array_equal(fb.topics["out_off"], fb44.topics["out_off"][:S]) and np.array_equal(fb.node_id, sl(fb44.node_id))
    base = native.node_blocks(fb44)
    imp = (nodes[:int(base[S])], scen[:S])
    sr = ho.scenario_results[:S]
    keys = ("max_outbound", "moved_replicas")
    want = choose_ref(fb, sr, ho.out, imp, keys, 3)
    assert want.n_ok >= 3 and bool((want.chosen < S // 2).any()) and bool((want.chosen >= S // 2).any()), \
        ("the winners come from one half of the batch: the ranking would not have to span ranges", want.chosen)
    got_ho, got = native.solve_host_choose(fb, keys, 3, ctx=ctx)
    assert_same_choice(want, got, f"{S} scenarios over ranges")
    for f in RESULT_FIELDS:
        assert (got_ho.scenario_results[f][:S] == sr[f]).all(), f
    _, got16 = native.solve_host_choose(fb, keys, 3, cells16=True, ctx=ctx)
    assert_same_choice(choose_ref(fb, sr, out16, imp, keys, 3), got16, f"{S} scenarios over ranges, 16-bit cells")


# ---- WhatIf.best ----------------------------------------------------------------------------------------------------------
def test_whatif_best(ctx):
    from kafka_assigner_amd.whatif import Variant
    w, vs, _, _, _ = whatif_solved()
    vs = vs[:60]
    by = ("max_inbound", "moved_replicas")
    full = w.solve(vs, impact=True)
    ok = [i for i, r in enumerate(full) if r.status == abi.KAS_OK]
    order = sorted(ok, key=lambda i: (full[i].max_inbound, full[i].moved_replicas, i))
    assert len(ok) >= 20 and len(ok) < len(vs)
    best = w.best(vs, k=7, by=by)                                # (the same variant list: the same batch layout as `full`'s)
    assert [r.rank for r in best] == list(range(7))
    assert [r._index for r in best] == order[:7]
    for r in best:
        f = full[r._index]
        assert r.label == f.label and r.status == abi.KAS_OK and r.digest == f.digest
        for name in ("moved_replicas", "moved_partitions") + abi.SCENARIO_IMPACT_FIELDS:
            assert getattr(r, name) == getattr(f, name), name
        assert r.broker_impact() == f.broker_impact()
        for t in w.topic_names:
            assert r.assignment(t) == f.assignment(t) and len(r.assignment(t)) > 1000, (r._index, t)
    # "as is" twice: both tie on everything, the earlier one wins
    first = w.best(vs, k=1)
    assert len(first) == 1 and first[0]._index == 0 and first[0].label == "as is" and first[0].rank == 0
    assert [r._index for r in w.best(vs, k=2)] == [0, 1]
    assert len(w.best(vs, k=len(vs))) == len(ok)                 # fewer results than k when fewer variants solve
    with pytest.raises(ValueError):
        w.best(vs, k=1, by=("moved_replicas", "cheapest"))
    plain = w.solve(vs[:3])
    assert plain[0].rank is None and plain[1].assignment("orders")


# ---- the link guard -------------------------------------------------------------------------------------------------------
def test_choice_is_not_slower_than_downloading_every_node_record(ctx):
    """1,000 variants over one 10,000-row RF 3 snapshot on 1,000 brokers in 20 racks: kas_solve_host_choose (k = 1) against the
    existing kas_solve_host_impact with n_select = 0, alternately on one context, five calls each after a warm-up each, medians of
    the wall time of the library call.  The existing entry is unchanged code: it is the yardstick.  The new call leaves ~32 MB of
    node records on the device and adds two small kernels and a synchronisation."""
    S, P, N, R = 1000, 10_000, 1000, 20
    cur = G.random_assignment(5, P, N, R, 3)
    ids, racks = [], []
    for s in range(S):
        _, bs = G.scenario_action(5, s, N, R, actions=G.BENCH_ACTIONS)
        ids.append(bs.node_id); racks.append(bs.node_rack)
    fb = node_set_batch(ids, racks, P, 3, 3, shared_cur=True, cur=cur)
    L = native.load()
    bd = batch_desc(fb)
    t_old, ho_old = host_tables(fb, out_len=0)
    t_new, ho_new = host_tables(fb, out_len=0)
    t_new.out = None
    nodes, scen = native.impact_arrays(fb)
    imp_old = abi.ImpactTables(nodes.ctypes.data, scen.ctypes.data)
    scen_new = np.zeros(S, abi.SCENARIO_IMPACT_DTYPE)
    imp_new = abi.ImpactTables(None, scen_new.ctypes.data)
    rows_cap, nodes_cap = k_largest(fb, 1)
    a = dict(rank=np.zeros(S, np.int32), chosen=np.zeros(1, np.int32), row_off=np.zeros(2, np.int64), node_off=np.zeros(2, np.int64),
             n_ok=np.zeros(1, np.int32), rows=np.zeros(rows_cap, np.int32), nodes=np.zeros(nodes_cap, abi.NODE_IMPACT_DTYPE))
    ch = abi.Choice(a["rank"].ctypes.data, a["chosen"].ctypes.data, a["row_off"].ctypes.data, a["node_off"].ctypes.data,
                    a["n_ok"].ctypes.data, a["rows"].ctypes.data, rows_cap, a["nodes"].ctypes.data, nodes_cap)
    spec = abi.choose_spec(("moved_replicas", "leaders_moved"), 1)

    def old():
        t0 = time.perf_counter()
        rc = L.kas_solve_host_impact(ctx._h, C.byref(bd), C.byref(t_old), None, 0, C.byref(imp_old))
        dt = time.perf_counter() - t0
        assert rc == 0, L.kas_last_error()
        return dt

    def new():
        t0 = time.perf_counter()
        rc = L.kas_solve_host_choose(ctx._h, C.byref(bd), C.byref(t_new), C.byref(spec), C.byref(ch), C.byref(imp_new))
        dt = time.perf_counter() - t0
        assert rc == 0, L.kas_last_error()
        return dt
    old(); new()
    t_o, t_n = [], []
    for _ in range(5):
        t_o.append(old()); t_n.append(new())
    m_old, m_new = float(np.median(t_o)), float(np.median(t_n))
    print(f"link guard: kas_solve_host_impact (n_select = 0) {1e3 * m_old:.3f} ms, kas_solve_host_choose (k = 1) {1e3 * m_new:.3f} ms")
    # the same winner as the records of the old call give, with its rows' size
    want = rank_ref(ho_old.scenario_results[:S], scen, ("moved_replicas", "leaders_moved"), 1)
    assert int(a["chosen"][0]) == int(want.chosen[0]) and int(a["n_ok"][0]) == want.n_ok
    assert np.array_equal(a["rank"], want.rank) and int(a["row_off"][1]) == 3 * P
    base = native.node_blocks(fb)
    s = int(want.chosen[0])
    for f in abi.NODE_IMPACT_FIELDS:
        assert np.array_equal(a["nodes"][f][:int(a["node_off"][1])], nodes[f][base[s]:base[s + 1]]), f
    assert m_new <= m_old, (m_new, m_old)

"""The Pareto front of the scenarios on the GPU (include/kas_abi.h: kas_front_spec): kas_front_rank_device, kas_solve_host_front / 16,
kas_front_device / 16 and WhatIf.front against the NumPy checker (tests/front_ref.py) over the oracle's solves."""
import ctypes as C

import numpy as np
import pytest

import test_choose_gpu as tg
from choose_ref import assert_same_choice
from front_ref import DOMINATED, assert_same_front, cut, front_choice_ref, front_ref
from impact_batches import solved
from impact_ref import assert_same_impact
from kafka_assigner_amd import abi, native
from kafka_assigner_amd.flatten import batch_desc, host_tables, node_set_batch, to_cells16
from moves_ref import assert_same_moves, moves_ref
from test_choose_cpu import MULTI_SPECS, S_VALUES, SENTINEL, k_largest, synthetic, whatif_solved
from test_front_cpu import TOP, WHATIF_A, WHATIF_B, WHATIF_BOUND, _ks, _spec

pytestmark = pytest.mark.gpu

RESULT_FIELDS = tg.RESULT_FIELDS


@pytest.fixture(scope="module")
def ctx():
    return native.DeviceContext(0)


# ---- synthetic fronts -----------------------------------------------------------------------------------------------------
def _front_rank_device(ctx, sr, si, keys, k, within=()):
    import torch
    dev = torch.device("cuda", ctx.device)
    S = int(sr.shape[0])
    d_sr = torch.from_numpy(sr.view(np.uint8).copy()).to(dev)
    d_si = torch.from_numpy(si.view(np.uint8).copy()).to(dev)
    d_rank = torch.full((S + 1,), SENTINEL, dtype=torch.int32, device=dev)
    d_chosen = torch.full((k + 1,), SENTINEL, dtype=torch.int32, device=dev)
    d_counts = torch.full((5,), SENTINEL, dtype=torch.int32, device=dev)
    d_scratch = torch.full((S + 1,), SENTINEL, dtype=torch.int32, device=dev)
    st = torch.cuda.Stream(dev)
    st.wait_stream(torch.cuda.current_stream(dev))
    native.front_rank_device(d_sr.data_ptr(), d_si.data_ptr(), S, _spec(keys, k, within), d_rank.data_ptr(), d_chosen.data_ptr(),
                             d_counts.data_ptr(), d_scratch.data_ptr(), stream=st.cuda_stream, ctx=ctx)
    st.synchronize()
    rank, chosen, counts, scratch = d_rank.cpu().numpy(), d_chosen.cpu().numpy(), d_counts.cpu().numpy(), d_scratch.cpu().numpy()
    assert rank[S] == SENTINEL and chosen[k] == SENTINEL and counts[4] == SENTINEL and scratch[S] == SENTINEL   # (nothing behind the arrays)
    from types import SimpleNamespace
    return SimpleNamespace(rank=rank[:S], chosen=chosen[:k], counts=counts[:4])


def _device_every_k(ctx, sr, si, keys, what, within=()):
    want = front_ref(sr, si, keys, 0, within)
    for k in _ks(int(sr.shape[0]), int(want.order.size)):
        assert_same_front(cut(want, k), _front_rank_device(ctx, sr, si, keys, k, within), f"{what} k={k}")
    return want


@pytest.mark.parametrize("S", S_VALUES + [5000])
def test_front_rank_device_on_synthetic_records(ctx, S):
    """the families of tests/test_front_cpu.py: small values (ties everywhere), wide values (fronts of tens), an antichain, a chain,
    twins, extremes, bounds inside and outside the spec and one nobody meets; k at 0, around n_front and at S"""
    big = S >= 1500                                              # (the checker is O(S^2): fewer specs of each family there)
    sr, si = synthetic(S, 1, failed="random")
    for keys in [MULTI_SPECS[2]] if big else [("max_inbound",), MULTI_SPECS[0], MULTI_SPECS[2]]:
        _device_every_k(ctx, sr, si, keys, f"S={S} small {keys}")
    sr, si = synthetic(S, 1, values=64, failed="random")
    want = _device_every_k(ctx, sr, si, MULTI_SPECS[2], f"S={S} wide")
    assert S < 65 or want.order.size >= 10
    bounds = ({"max_inbound": 30}, {"max_outbound": 20, "moved_replicas": 40}, {"leader_spread": TOP},
              {"max_outbound": 30, "leaders_moved": 30, "moved_partitions": 30, "max_inbound": 50})
    for within in bounds[1::2] if big else bounds:
        _device_every_k(ctx, sr, si, ("max_inbound", "moved_replicas"), f"S={S} within {within}", within)
    sr["moved_partitions"] += 1
    got = _front_rank_device(ctx, sr, si, MULTI_SPECS[0], min(S, 3), {"moved_partitions": 0})
    assert got.counts[1] == 0 and got.counts[2] == 0 and (got.chosen == -1).all()
    for failed in ("alternate",) if big else ("none", "alternate", "all"):
        sr, si = synthetic(S, 2, failed=failed)
        perm = np.random.default_rng(S).permutation(S).astype(np.int32)
        keys = ("moved_replicas", "moved_partitions")
        sr["moved_replicas"], sr["moved_partitions"] = perm, S - perm               # an antichain
        want = _device_every_k(ctx, sr, si, keys, f"S={S} antichain {failed}")
        assert want.order.size == int((sr["status"] == 0).sum())
        sr["moved_replicas"], sr["moved_partitions"] = np.arange(S), 2 * np.arange(S)   # a chain
        want = _device_every_k(ctx, sr, si, keys, f"S={S} chain {failed}")
        assert want.order.size == (1 if failed != "all" else 0)
    half = (S + 1) // 2
    sr["status"] = 0
    sr["moved_replicas"], sr["moved_partitions"] = np.tile(perm[:half], 2)[:S] % half, half - np.tile(perm[:half], 2)[:S] % half
    want = _device_every_k(ctx, sr, si, keys, f"S={S} twins")
    assert (want.classes[half:] == DOMINATED).all()
    sr, si = synthetic(S, 4, values=[0, TOP], failed="alternate")
    for keys in MULTI_SPECS[1:] if big else [(name,) for name in abi.KEY_NAMES] + MULTI_SPECS:
        assert_same_front(front_ref(sr, si, keys, S), _front_rank_device(ctx, sr, si, keys, S), f"S={S} extremes {keys}")


def test_front_rank_device_refuses_bad_specs(ctx):
    import torch
    d = torch.zeros(64, dtype=torch.int32, device=torch.device("cuda", ctx.device))
    p = d.data_ptr()
    good = ("moved_replicas",)
    for spec, text in ((_spec(good, 1, n_keys=0), "n_keys outside"), (_spec((10,), 1), "unknown criterion"), (_spec(good, 1, n_limits=5), "n_limits outside"),
                       (_spec(good, 1, [(10, 1)]), "unknown limit criterion"), (_spec(good, 1, [(0, -1)]), "negative limit"),
                       (_spec(good, 3), "k outside")):
        with pytest.raises(native.KasError) as e:
            native.front_rank_device(p, p, 2, spec, p, p, p, p, ctx=ctx)
        assert e.value.code == abi.KAS_E_INVALID_ARG and text in e.value.detail, e.value.detail
    with pytest.raises(native.KasError) as e:
        native.front_rank_device(p, p, 2, _spec(good, 1), p, p, 0, p, ctx=ctx)
    assert "is NULL" in e.value.detail


# ---- the host call --------------------------------------------------------------------------------------------------------
def _check_host_front(ctx, fb, sr, out, imp, keys, k, within, cells16, what, mask=None, rows=True, moves_of=None, fields=RESULT_FIELDS):
    S = fb.n_scenarios
    got_ho, got, ml = native.solve_host_front(fb, _spec(keys, k, within), mask, rows=rows, cells16=cells16, ctx=ctx)
    want = front_choice_ref(fb, sr, out, imp, keys, k, within)
    got.counts = np.array([got.n_ok, got.n_eligible, got.n_front, 0], np.int32)
    assert_same_front(want, got, what)
    if rows:
        assert_same_choice(want, got, what)
    else:
        assert got.rows.size == 0
        want.rows = want.rows[:0]
        got.rows = np.zeros(int(want.row_off[k]), want.rows.dtype)[:0]
        for f in abi.NODE_IMPACT_FIELDS:
            assert np.array_equal(want.nodes[f], got.nodes[f][:int(want.node_off[k])]), (what, f)
    for f in fields:
        assert (got_ho.scenario_results[f][:S] == sr[f][:S]).all(), (what, f)
    for f in abi.SCENARIO_IMPACT_FIELDS:
        assert (got.scenarios[f] == imp[1][f]).all(), (what, f)
    if mask is not None:
        mfb, mho, cur16 = moves_of
        assert_same_moves(moves_ref(mfb, mho, want.chosen, mask, cells16=cells16, cur16=cur16), ml, what)
    return got_ho, got, want


@pytest.mark.parametrize("cells16", [False, True], ids=["int32", "cells16"])
@pytest.mark.parametrize("keys,n_front,n_bound", [(WHATIF_A, 6, 8), (WHATIF_B, 14, 16)], ids=["moved", "spread"])
def test_whatif_host_front(ctx, keys, n_front, n_bound, cells16):
    """302 variants of one snapshot: both specs with and without the bound, k at 1, n_front, n_front + 1 and 302, with moves (masks
    1 and 7) and without rows, against the checker over the oracle's solve; the records equal kas_solve_host_impact's"""
    from types import SimpleNamespace
    _, _, fb, ho, imp = whatif_solved()
    if cells16:                                                  # (one cur table per variant: the shared one has no 16-bit form)
        fb, sr, out = tg._whatif16()
        mho = SimpleNamespace(out=out, topic_results=ho.topic_results, scenario_results=sr)
        moves_of = (fb, mho, to_cells16(fb))
    else:
        sr, out = ho.scenario_results, ho.out
        moves_of = (fb, ho, None)
    for within, n in (((), n_front), (WHATIF_BOUND, n_bound)):
        for k in (1, n, n + 1, 302):
            got_ho, got, want = _check_host_front(ctx, fb, sr, out, imp, keys, k, within, cells16, f"what-if {keys} {within} k {k} cells16 {cells16}")
            assert want.counts[2] == n
        _check_host_front(ctx, fb, sr, out, imp, keys, n + 1, within, cells16, f"what-if moves 1 {keys} {within}", mask=1, moves_of=moves_of)
        _check_host_front(ctx, fb, sr, out, imp, keys, n, within, cells16, f"what-if moves 7 no rows {keys} {within}", mask=7, rows=False, moves_of=moves_of)
        _check_host_front(ctx, fb, sr, out, imp, keys, n, within, cells16, f"what-if no rows no moves {keys} {within}", rows=False)
    old_ho, old_nodes, old_scen = native.solve_host_impact(fb, select=[], cells16=cells16, ctx=ctx)
    for f in RESULT_FIELDS:
        assert (old_ho.scenario_results[f] == got_ho.scenario_results[f]).all(), f
    assert_same_impact((imp[0], got.scenarios), (old_nodes, old_scen), "scenario impact of the two calls")


@pytest.mark.parametrize("cells16", [False, True], ids=["int32", "cells16"])
@pytest.mark.parametrize("name", ["mixed42", "degenerate", "widths_4_5"])
def test_host_front_on_the_named_batches(ctx, name, cells16):
    import test_moves_cpu as tm
    fb, ho, imp = solved(name)
    sr, out = tg._reference(fb, ho, cells16)
    mfb, cur, mho = tm.forms(name)[1 if cells16 else 0]
    for k in range(fb.n_scenarios + 1):
        _check_host_front(ctx, fb, sr, out, imp, ("max_inbound", "moved_replicas"), k, (), cells16, f"{name} k {k} cells16 {cells16}",
                          mask=7 if k % 2 else None, moves_of=(mfb, mho, cur if cells16 else None))


def test_host_front_refusals(ctx):
    fb, _, _ = solved("mixed42")
    good = ("moved_replicas",)
    for spec, text in ((_spec(good, 1, n_keys=5), "n_keys outside"), (_spec((10,), 1), "unknown criterion"), (_spec(good, 1, n_limits=-1), "n_limits outside"),
                       (_spec(good, 1, [(10, 1)]), "unknown limit criterion"), (_spec(good, 1, [(0, -1)]), "negative limit"),
                       (_spec(good, fb.n_scenarios + 1), "k outside")):
        with pytest.raises(native.KasError) as e:
            native.solve_host_front(fb, spec, ctx=ctx)
        assert e.value.code == abi.KAS_E_INVALID_ARG and text in e.value.detail, e.value.detail
    # capacities one below the k-largest bound, and a NULL array (counts among them), straight at the ABI
    L = native.load()
    bd = batch_desc(fb)
    t, ho = host_tables(fb, out_len=0)
    t.out = None
    rows, nodes = k_largest(fb, 2)
    S = fb.n_scenarios
    a = dict(rank=np.zeros(S, np.int32), chosen=np.zeros(2, np.int32), row_off=np.zeros(3, np.int64), node_off=np.zeros(3, np.int64),
             n_ok=np.zeros(1, np.int32), rows=np.zeros(rows, np.int32), nodes=np.zeros(nodes, abi.NODE_IMPACT_DTYPE), counts=np.zeros(4, np.int32))
    scen = np.zeros(S, abi.SCENARIO_IMPACT_DTYPE)
    imp = abi.ImpactTables(None, scen.ctypes.data)
    spec = _spec(good, 2)

    def call(rows_cap=rows, nodes_cap=nodes, null=None):
        p = {n: (None if n == null else v.ctypes.data) for n, v in a.items()}
        ch = abi.Choice(p["rank"], p["chosen"], p["row_off"], p["node_off"], p["n_ok"], p["rows"], rows_cap, p["nodes"], nodes_cap)
        rc = L.kas_solve_host_front(ctx._h, C.byref(bd), C.byref(t), C.byref(spec), C.byref(ch), p["counts"], C.byref(imp), None)
        return rc, (L.kas_last_error() or b"").decode()
    assert call()[0] == 0
    rc, err = call(rows_cap=rows - 1)
    assert rc == abi.KAS_E_INVALID_ARG and "rows_cap below" in err
    rc, err = call(nodes_cap=nodes - 1)
    assert rc == abi.KAS_E_INVALID_ARG and "nodes_cap below" in err
    for n in a:
        rc, err = call(null=n)
        assert rc == abi.KAS_E_INVALID_ARG and "is NULL" in err, (n, err)
    assert call(rows_cap=0, null="rows")[0] == 0                  # rows == NULL with rows_cap == 0 gathers no rows


# ---- the device path ------------------------------------------------------------------------------------------------------
def _device_front_twice(ctx, fb, cells16, specs):
    """Plan + solve_device + impact_device + front_device (twice, one spec each, outputs of their own) on one non-default torch
    stream: (HostOutputs, (nodes, scenarios), [front per spec])"""
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
        for keys, within, k in specs:
            rows_cap, nodes_cap = k_largest(fb, k)
            d = SimpleNamespace(rank=torch.full((S + 1,), SENTINEL, dtype=torch.int32, device=dev),
                                chosen=torch.full((k + 1,), SENTINEL, dtype=torch.int32, device=dev),
                                row_off=torch.full((k + 2,), SENTINEL, dtype=torch.int64, device=dev),
                                node_off=torch.full((k + 2,), SENTINEL, dtype=torch.int64, device=dev),
                                n_ok=torch.full((2,), SENTINEL, dtype=torch.int32, device=dev),
                                counts=torch.full((5,), SENTINEL, dtype=torch.int32, device=dev),
                                rows=torch.full((rows_cap + 64,), 0x7B7B, dtype=torch.int16 if cells16 else torch.int32, device=dev),
                                nodes=torch.full(((nodes_cap + 2) * 32,), 0x7B, dtype=torch.uint8, device=dev))
            plan.front_device(_spec(keys, k, within), d_out.data_ptr(), d_sr.data_ptr(), d_nodes.data_ptr(), d_scen.data_ptr(),
                              d.rank.data_ptr(), d.chosen.data_ptr(), d.row_off.data_ptr(), d.node_off.data_ptr(), d.n_ok.data_ptr(),
                              d.rows.data_ptr(), rows_cap, d.nodes.data_ptr(), nodes_cap, d.counts.data_ptr(), stream=st.cuda_stream)
            held.append((d, k, rows_cap, nodes_cap))
        st.synchronize()
        ho.out = d_out.cpu().numpy().view(np.uint16) if cells16 else d_out.cpu().numpy()
        ho.scenario_results = d_sr.cpu().numpy().view(abi.SCENARIO_RESULT_DTYPE)
        imp = (d_nodes.cpu().numpy().view(abi.NODE_IMPACT_DTYPE)[:n_nodes], d_scen.cpu().numpy().view(abi.SCENARIO_IMPACT_DTYPE)[:S])
        got = []
        for d, k, rows_cap, nodes_cap in held:
            rows = d.rows.cpu().numpy().view(np.uint16 if cells16 else np.int32)
            raw = d.nodes.cpu().numpy()
            rank, chosen, row_off, node_off = d.rank.cpu().numpy(), d.chosen.cpu().numpy(), d.row_off.cpu().numpy(), d.node_off.cpu().numpy()
            n_ok, counts = d.n_ok.cpu().numpy(), d.counts.cpu().numpy()
            assert rank[S] == SENTINEL and chosen[k] == SENTINEL and row_off[k + 1] == SENTINEL and node_off[k + 1] == SENTINEL
            assert n_ok[1] == SENTINEL and counts[4] == SENTINEL
            g = SimpleNamespace(rank=rank[:S], chosen=chosen[:k], row_off=row_off[:k + 1], node_off=node_off[:k + 1], n_ok=int(n_ok[0]),
                                counts=counts[:4], rows=rows, nodes=raw.view(abi.NODE_IMPACT_DTYPE))
            used, recs = int(g.row_off[k]), int(g.node_off[k])
            assert 0 <= used <= rows_cap and 0 <= recs <= nodes_cap
            assert (rows[used:] == 0x7B7B).all() and (raw[32 * recs:] == 0x7B).all(), "written behind the offsets / the capacities"
            got.append(g)
        return ho, imp, got
    finally:
        plan.close()


@pytest.mark.parametrize("cells16", [False, True], ids=["int32", "cells16"])
@pytest.mark.parametrize("name", ["rows_10000", "mixed42"])
def test_device_front_twice_on_one_plan(ctx, name, cells16):
    fb, _, want_imp = solved(name)
    S = fb.n_scenarios
    specs = [(("moved_replicas", "leaders_moved"), (), S), (("max_outbound", "replica_spread", "moved_partitions"), {"max_inbound": 10**6}, max(S - 1, 1))]
    ho, imp, got = _device_front_twice(ctx, fb, cells16, specs)
    assert_same_impact(want_imp, imp, f"{name}: the impact pass the front reads")
    for (keys, within, k), g in zip(specs, got):
        want = front_choice_ref(fb, ho.scenario_results, ho.out, want_imp, keys, k, within)
        assert_same_front(want, g, f"{name} cells16 {cells16} {keys} k {k}")
        assert_same_choice(want, g, f"{name} cells16 {cells16} {keys} k {k}")


# ---- a call cut into scenario ranges --------------------------------------------------------------------------------------
def test_host_front_over_scenario_ranges(ctx):
    """test_choose_gpu's batch of 44 x 100k x 200 brokers with a `cur` per scenario, which a choice cuts into two ranges: the front
    spans the whole call.  By (max_outbound, moved_replicas) its members come from both halves of the batch (the guard below)."""
    fb, ho, imp, out16 = tg._ranges_batch()
    S = fb.n_scenarios
    sr = ho.scenario_results[:S]
    keys = ("max_outbound", "moved_replicas")
    want = front_choice_ref(fb, sr, ho.out, imp, keys, S)
    assert bool((want.order < S // 2).any()) and bool((want.order >= S // 2).any()), \
        ("the members come from one half of the batch: the front would not have to span ranges", want.order)
    k = min(int(want.order.size), 3)
    got_ho, got, _ = _check_host_front(ctx, fb, sr, ho.out, imp, keys, k, (), False, "44 scenarios over ranges")
    # (16-bit cells are node indices: the digest is the index form's, which this batch was not solved in)
    _check_host_front(ctx, fb, sr, out16, imp, keys, k, (), True, "44 scenarios over ranges, 16-bit cells", fields=RESULT_FIELDS[:-1])


# ---- WhatIf.front ---------------------------------------------------------------------------------------------------------
def test_whatif_front(ctx):
    w, vs, _, _, _ = whatif_solved()
    vs = vs[:60]
    by = ("moved_replicas", "leader_spread", "replica_spread")
    full = w.solve(vs, impact=True)
    crit = lambda r: (r.moved_replicas, r.max_leaders_after - r.min_leaders_after, r.max_replicas_after - r.min_replicas_after)

    def brute(within=None):
        elig = [i for i, r in enumerate(full) if r.status == abi.KAS_OK and all(getattr(r, n) <= v for n, v in (within or {}).items())]
        dom = lambda t, s: all(a <= b for a, b in zip(crit(full[t]), crit(full[s]))) and (crit(full[t]) != crit(full[s]) or t < s)
        members = [s for s in elig if not any(dom(t, s) for t in elig if t != s)]
        return elig, sorted(members, key=lambda i: crit(full[i]) + (i,))
    elig, members = brute()
    assert len(members) >= 3 and len(elig) < len(vs)
    front = w.front(vs, by=by, k=len(vs), moves=("replicas",))
    assert [r._index for r in front] == members and [r.rank for r in front] == list(range(len(members)))
    assert front.n_front == len(members) and front.n_eligible == front.n_ok == len(elig)
    for i, c in enumerate(front.classes):
        assert c == ("failed" if full[i].status != abi.KAS_OK else "member" if i in members else "dominated"), (i, c)
    for r in front:
        f = full[r._index]
        assert r.label == f.label and r.digest == f.digest and r.broker_impact() == f.broker_impact()
        for name in ("moved_replicas", "moved_partitions") + abi.SCENARIO_IMPACT_FIELDS:
            assert getattr(r, name) == getattr(f, name), name
        for t in w.topic_names:
            assert r.assignment(t) == f.assignment(t)
        moved = r.moves()
        assert moved and all(r.assignment(t)[p] == reps for t, p, reps, _ in moved)
    cut = w.front(vs, by=by, k=2)
    assert [r._index for r in cut] == members[:2] and cut.n_front == len(members) > len(cut)
    belig, bmembers = brute({"max_outbound": 24})
    bound = w.front(vs, by=by, within={"max_outbound": 24}, k=len(vs), rows=False, moves=("replicas",))
    assert [r._index for r in bound] == bmembers and bound.n_eligible == len(belig) and bound.classes.count("over_limit") == len(elig) - len(belig)
    with pytest.raises(ValueError):
        bound[0].assignment(w.topic_names[0])
    with pytest.raises(ValueError):
        w.front(vs, by=("moved_replicas", "cheapest"))

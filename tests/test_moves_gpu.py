"""The move list on the MI355X (kas_moves_device / 16, kas_solve_host_moves / 16, kas_solve_host_choose_moves / 16, WhatIf.best with
moves=...), against the Python checker of tests/moves_ref.py."""
from types import SimpleNamespace

import numpy as np
import pytest

from impact_batches import solved
from kafka_assigner_amd import abi, native
from kafka_assigner_amd.flatten import host_tables, index_form, to_cells16
from moves_ref import assert_same_moves, moves_ref, written_prefix
from oracle_lib import oracle_solve
from test_choose_cpu import k_largest, own_cur_form, whatif_solved, whatif_variants

pytestmark = pytest.mark.gpu

RESULT_FIELDS = ("status", "fail_topic", "fail_partition", "moved_replicas", "moved_partitions", "digest")
TOPIC_FIELDS = ("status", "fail_partition", "moved_replicas", "moved_partitions")
KEYS = ("moved_replicas", "leaders_moved")


@pytest.fixture(scope="module")
def ctx():
    return native.DeviceContext(0)


_REF = {}


def reference(name, cells16):
    """(fb, cur pool, solve with every row in place) the calls of this cell width must reproduce: the oracle's solve, of the
    batch's index form for 16-bit cells"""
    if (name, cells16) not in _REF:
        fb, ho, _ = solved(name)
        if cells16:
            h = oracle_solve(index_form(fb))
            ho = SimpleNamespace(out=np.where(h.out < 0, abi.KAS_CELL16_NONE, h.out).astype(np.uint16), topic_results=h.topic_results,
                                 scenario_results=h.scenario_results)
        _REF[(name, cells16)] = (fb, to_cells16(fb) if cells16 else fb.cur, ho)
    return _REF[(name, cells16)]


def want_of(fb, cur, ho, select, mask, cells16):
    return moves_ref(fb, ho, select, mask, cells16=cells16, cur16=cur if cells16 else None)


@pytest.mark.parametrize("cells16", [False, True], ids=["int32", "cells16"])
@pytest.mark.parametrize("name", ["mixed42", "degenerate", "row_counts", "widths_4_5", "sparse", "rows_4097", "rf_7_8"])
def test_host_moves_on_the_named_batches(ctx, name, cells16):
    fb, cur, ho = reference(name, cells16)
    S = fb.n_scenarios
    plain = native.solve_host16(fb, ctx=ctx) if cells16 else native.solve_host(fb, ctx=ctx)
    for mask in (1, 7):
        got_ho, got = native.solve_host_moves(fb, mask, cells16=cells16, ctx=ctx)
        want = want_of(fb, cur, ho, range(S), mask, cells16)
        assert want.n_moves.sum() >= 1 and want.n_rest.sum() >= 1
        assert_same_moves(want, got, f"{name} mask {mask} cells16 {cells16}")
        assert got.moves.size == want.moves.size and got.cells.size == want.cells.size and not got.truncated
        for f in RESULT_FIELDS:                                   # the solve's records are a plain solve_host's
            assert (got_ho.scenario_results[f][:S] == plain.scenario_results[f][:S]).all(), (name, f)
        for f in TOPIC_FIELDS:
            assert (got_ho.topic_results[f][:fb.n_topics] == plain.topic_results[f][:fb.n_topics]).all(), (name, f)
    # a host list with an empty slot and a repeated scenario; capacities one short of the list: offsets complete, a prefix written
    select = [S - 1, -1, 0, S - 1]
    want = want_of(fb, cur, ho, select, 7, cells16)
    _, got = native.solve_host_moves(fb, 7, select=select, cells16=cells16, ctx=ctx)
    assert_same_moves(want, got, f"{name} list {select}")
    M, Cc = int(want.move_off[-1]), int(want.cell_off[-1])
    for mc, cc in ((M - 1, Cc), (M, Cc - 1), (0, 0), (M // 2, Cc // 3)):
        _, got = native.solve_host_moves(fb, 7, select=select, cells16=cells16, moves_cap=mc, cells_cap=cc, ctx=ctx)
        n, used = assert_same_moves(want, got, f"{name} caps {mc} {cc}", mc, cc)
        assert (n, used) == written_prefix(want, mc, cc) and got.truncated == (M > 0)


def test_host_moves_refusals(ctx):
    fb, _, _ = solved("mixed42")
    for kw, text in ((dict(mask=0), "mask outside"), (dict(mask=8), "mask outside"), (dict(mask=7, select=[fb.n_scenarios]), "out of range"),
                     (dict(mask=7, moves_cap=-1), "negative capacity")):
        with pytest.raises(native.KasError) as e:
            native.solve_host_moves(fb, ctx=ctx, **kw)
        assert e.value.code == abi.KAS_E_INVALID_ARG and text in e.value.detail, e.value.detail
    with pytest.raises(ValueError):
        native.solve_host_moves(fb, ("sideways",), ctx=ctx)


# ---- the device path ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cells16", [False, True], ids=["int32", "cells16"])
@pytest.mark.parametrize("name", ["mixed42", "rows_4097"])
def test_device_moves_behind_a_choice_on_one_stream(ctx, name, cells16):
    """Plan + solve_device + impact_device + choose_device + moves_device (twice: fed the device chosen[] with its -1 tail, then a
    list of its own under another mask) on one non-default torch stream, sentinel-filled outputs with guards"""
    import torch
    fb, cur, ho = reference(name, cells16)
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
        own = [0, -1, S - 1, 0]
        d_own = torch.tensor(own, dtype=torch.int32, device=dev)
        room = native.moves_room(fb, range(S))                   # (a list of four entries needs at most four times this)
        outs = []
        for n in (k, len(own)):
            outs.append(SimpleNamespace(move_off=torch.full((n + 2,), -77, dtype=torch.int64, device=dev),
                                        cell_off=torch.full((n + 2,), -77, dtype=torch.int64, device=dev),
                                        moves=torch.full(((4 * room[0] + 1) * 16,), 0x7B, dtype=torch.uint8, device=dev),
                                        cells=torch.full((4 * room[1] + 1,), 0x7B7B, dtype=cdt, device=dev)))
        st = torch.cuda.Stream(dev)
        st.wait_stream(torch.cuda.current_stream(dev))
        aux = d_aux.data_ptr() if d_aux is not None else 0
        plan.solve_device(d_cur.data_ptr(), d_out.data_ptr(), d_tr.data_ptr(), d_sr.data_ptr(), aux=aux, stream=st.cuda_stream)
        plan.impact_device(d_cur.data_ptr(), d_out.data_ptr(), d_tr.data_ptr(), d_nodes.data_ptr(), d_scen.data_ptr(), aux=aux, stream=st.cuda_stream)
        plan.choose_device(KEYS, k, d_out.data_ptr(), d_sr.data_ptr(), d_nodes.data_ptr(), d_scen.data_ptr(), d_rank.data_ptr(),
                           d_chosen.data_ptr(), d_roff.data_ptr(), d_noff.data_ptr(), d_nok.data_ptr(), d_rows.data_ptr(), rows_cap,
                           d_cnodes.data_ptr(), nodes_cap, stream=st.cuda_stream)
        for o, (mask, sel, n) in zip(outs, ((1, d_chosen, k), (7, d_own, len(own)))):
            plan.moves_device(mask, sel.data_ptr(), n, d_cur.data_ptr(), d_out.data_ptr(), d_tr.data_ptr(), o.move_off.data_ptr(),
                              o.cell_off.data_ptr(), o.moves.data_ptr(), 4 * room[0], o.cells.data_ptr(), 4 * room[1], aux=aux, stream=st.cuda_stream)
        st.synchronize()
        chosen = d_chosen.cpu().numpy()
        status = d_sr.cpu().numpy().view(abi.SCENARIO_RESULT_DTYPE)["status"][:S]
        assert sorted(chosen[chosen >= 0].tolist()) == np.nonzero(status == 0)[0].tolist() and (chosen[int((status == 0).sum()):] == -1).all()
        for o, (mask, sel, n) in zip(outs, ((1, chosen.tolist(), k), (7, own, len(own)))):
            want = want_of(fb, cur, ho, sel, mask, cells16)
            mo, co = o.move_off.cpu().numpy(), o.cell_off.cpu().numpy()
            assert mo[n + 1] == -77 and co[n + 1] == -77, "the guard behind the offsets was written"
            raw = o.moves.cpu().numpy()
            cells = o.cells.cpu().numpy().view(np.uint16 if cells16 else np.int32)
            got = SimpleNamespace(move_off=mo[:n + 1], cell_off=co[:n + 1], moves=raw.view(abi.MOVE_DTYPE), cells=cells)
            assert_same_moves(want, got, f"{name} device mask {mask} cells16 {cells16}")
            assert (raw[16 * int(want.move_off[-1]):] == 0x7B).all() and (cells[int(want.cell_off[-1]):] == 0x7B7B).all(), "written behind the list"
    finally:
        plan.close()


# ---- the what-if batch ----------------------------------------------------------------------------------------------------
def _pool_of(fb, ch, got_ho, dtype, pad):
    """an out pool with the chosen scenarios' rows (that call's own) back where the descriptors put them"""
    out = np.full(fb.out_len, pad, dtype)
    for j, s in enumerate(ch.chosen):
        if s < 0:
            continue
        at = int(ch.row_off[j])
        b, c = int(fb.scen["topic_begin"][s]), int(fb.scen["topic_count"][s])
        for t in range(b, b + c):
            n = int(fb.topics["n_partitions"][t]) * int(fb.topics["out_width"][t])
            out[int(fb.topics["out_off"][t]):][:n] = ch.rows[at:at + n]
            at += n
    return SimpleNamespace(out=out, topic_results=got_ho.topic_results)


@pytest.mark.parametrize("cells16", [False, True], ids=["int32", "cells16"])
def test_choose_moves_on_the_whatif_batch(ctx, cells16):
    """302 variants, k = 3: rank / chosen of kas_solve_host_choose; moves equal to the checker run on that call's own rows; the
    rows == NULL form returns no rows and the same moves"""
    fb = whatif_solved()[2]
    if cells16:
        fb = own_cur_form(fb)                                     # (one cur table per variant: the shared one has no 16-bit form)
    cur = to_cells16(fb) if cells16 else fb.cur
    _, old = native.solve_host_choose(fb, KEYS, 3, cells16=cells16, ctx=ctx)
    for mask in (1, 7):
        got_ho, ch, ml = native.solve_host_choose_moves(fb, KEYS, 3, mask, cells16=cells16, ctx=ctx)
        assert np.array_equal(ch.rank, old.rank) and np.array_equal(ch.chosen, old.chosen) and ch.n_ok == old.n_ok
        assert np.array_equal(ch.rows, old.rows) and np.array_equal(ch.row_off, old.row_off) and ch.nodes.tobytes() == old.nodes.tobytes()
        pool = _pool_of(fb, ch, got_ho, np.uint16 if cells16 else np.int32, abi.KAS_CELL16_NONE if cells16 else -1)
        want = want_of(fb, cur, pool, ch.chosen, mask, cells16)
        assert want.n_moves.sum() >= 1 and want.n_rest.sum() >= 1
        assert_same_moves(want, ml, f"what-if mask {mask} cells16 {cells16}")
        assert ml.moves.size == want.moves.size and ml.cells.size == want.cells.size
        ho2, ch2, ml2 = native.solve_host_choose_moves(fb, KEYS, 3, mask, rows=False, cells16=cells16, ctx=ctx)
        assert ch2.rows.size == 0 and np.array_equal(ch2.chosen, ch.chosen) and np.array_equal(ch2.row_off, ch.row_off)
        assert ch2.nodes.tobytes() == ch.nodes.tobytes()
        for a, b in ((ml.moves, ml2.moves), (ml.cells, ml2.cells), (ml.move_off, ml2.move_off), (ml.cell_off, ml2.cell_off)):
            assert a.tobytes() == b.tobytes()


def test_whatif_best_with_moves(ctx):
    w, vs = whatif_variants()
    cur = {name: {int(p): [int(b) for b in w.cur[int(w.cur_off[t]):].reshape(-1, w.widths[t])[i]] for i, p in enumerate(w.part_ids[t])}
           for t, name in enumerate(w.topic_names)}
    with_rows = w.best(vs, k=3)
    sets = w.best(vs, k=3, moves=("replicas",), rows=False)
    lists = w.best(vs, k=3, moves=("replicas", "leader", "order"), rows=False)
    assert len(with_rows) == 3 and [r.label for r in sets] == [r.label for r in with_rows] == [r.label for r in lists]
    for f, a, b in zip(with_rows, sets, lists):
        with pytest.raises(ValueError):
            a.assignment(w.topic_names[0])
        assert a.broker_impact() == f.broker_impact() and a.rank == f.rank
        for name in w.topic_names:
            new = {p: list(r) for p, r in cur[name].items()}
            for t, p, reps, _ in a.moves(topic=name):
                new[p] = reps
            assert {p: set(r) for p, r in new.items()} == {p: set(r) for p, r in f.assignment(name).items()}, (f.label, name)
            new = {p: list(r) for p, r in cur[name].items()}
            for t, p, reps, _ in b.moves(topic=name):
                new[p] = reps
            assert new == f.assignment(name), (f.label, name)
        assert len(a.reassignment()["partitions"]) == f.moved_partitions

"""The move list on the MI355X (kas_moves_device / 16, kas_solve_host_moves / 16, kas_solve_host_choose_moves / 16, WhatIf.solve and
WhatIf.best with moves=...), against the Python checker of tests/moves_ref.py: the named batches, lists long enough to take the scan
kernel across its tiles of 256 entries (each behind moves_ref.assert_spans_tiles), and host calls cut into scenario ranges."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import test_choose_gpu as tg
from choose_ref import assert_same_choice, choose_ref
from impact_batches import solved
from kafka_assigner_amd import abi, native
from kafka_assigner_amd.flatten import batch_desc, host_tables, host_tables16, index_form, node_set_batch, to_cells16
from moves_ref import SCAN_TILE, assert_same_moves, assert_spans_tiles, moves_ref, moves_ref_long, scenario_items, written_prefix
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
    T = len(w.topic_names)
    # the snapshot topic by topic: its rows as an array, the row of each partition id, and as the dict assignment() returns
    snap = [w.cur[int(w.cur_off[t]):][:len(w.part_ids[t]) * w.widths[t]].reshape(-1, w.widths[t]) for t in range(T)]
    row_of = [{int(p): i for i, p in enumerate(w.part_ids[t])} for t in range(T)]
    cur = {name: {int(p): [int(b) for b in snap[t][i]] for i, p in enumerate(w.part_ids[t])} for t, name in enumerate(w.topic_names)}
    t_of = {name: t for t, name in enumerate(w.topic_names)}
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


# ---- lists beyond one tile of the scan kernel -----------------------------------------------------------------------------
def host_moves(ctx, fb, mask, select=None, cells16=False, moves_cap=None, cells_cap=None, cur16=None):
    """kas_solve_host_moves / 16 into arrays of the test's own, every one pre-filled with a sentinel and with one guard element
    behind it (capacities default to native.moves_room, as native.solve_host_moves' do): (the trimmed MoveList, the raw arrays)"""
    S = fb.n_scenarios
    bd = batch_desc(fb)
    if cells16:
        bd.node_id = None
        cur16 = to_cells16(fb) if cur16 is None else cur16       # (held until the call returns: the table only borrows it)
        t, ho = host_tables16(fb, cur16, out_len=0)
    else:
        t, ho = host_tables(fb, out_len=0)
    t.out = None
    sel = np.arange(S, dtype=np.int32) if select is None else np.ascontiguousarray(select, dtype=np.int32)
    n = int(sel.size)
    room = native.moves_room(fb, sel)
    mc, cc = room[0] if moves_cap is None else int(moves_cap), room[1] if cells_cap is None else int(cells_cap)
    raw = SimpleNamespace(move_off=np.full(n + 2, -77, np.int64), cell_off=np.full(n + 2, -77, np.int64), moves=np.zeros(mc + 1, abi.MOVE_DTYPE),
                          cells=np.full(cc + 1, 0x7B7B, np.uint16 if cells16 else np.int32), moves_cap=mc, cells_cap=cc)
    raw.moves.view(np.uint8)[...] = 0x7B
    mv = abi.Moves(abi.move_mask(mask), 0, raw.move_off.ctypes.data, raw.cell_off.ctypes.data, raw.moves.ctypes.data, mc, raw.cells.ctypes.data, cc)
    fn = native.load().kas_solve_host16_moves if cells16 else native.load().kas_solve_host_moves
    native._check(fn(ctx._h, C.byref(bd), C.byref(t), sel.ctypes.data_as(C.POINTER(C.c_int32)), n, C.byref(mv)))
    assert raw.move_off[n + 1] == -77 and raw.cell_off[n + 1] == -77, "the guard behind the offsets was written"
    ml = native._trim(native.MoveList(mask=abi.move_mask(mask), select=sel, move_off=raw.move_off[:n + 1], cell_off=raw.cell_off[:n + 1],
                                      moves=raw.moves[:mc], cells=raw.cells[:cc]))
    return ml, raw


def check_host_moves(ctx, fb, cur, ho, select, mask, cells16, what, caps=None, spans=True, want=None):
    """a host call's list against the checker's: offsets complete, exactly the written prefix there, nothing behind it touched.
    Returns (the checker's list, the call's, the records that were written)"""
    c16 = cur if cells16 else None
    select = list(range(fb.n_scenarios)) if select is None else list(select)
    want = moves_ref_long(fb, ho, select, mask, cells16=cells16, cur16=c16) if want is None else want
    if spans:
        assert_spans_tiles(fb, ho, select, mask, want, cells16=cells16, cur16=c16, what=what)
    M, Cc = int(want.move_off[-1]), int(want.cell_off[-1])
    ml, raw = host_moves(ctx, fb, mask, select, cells16, *(caps or (None, None)), cur16=c16)
    n, used = assert_same_moves(want, ml, what, raw.moves_cap, raw.cells_cap)
    assert (n, used) == written_prefix(want, raw.moves_cap, raw.cells_cap) and ml.truncated == (n < M or used < Cc), (what, n, used, M, Cc)
    assert ml.moves.size >= n and ml.cells.size >= used
    assert (raw.moves.view(np.uint8)[16 * n:] == 0x7B).all(), (what, "records beyond the written ones were touched")
    assert (raw.cells[used:] == 0x7B7B).all(), (what, "cells beyond the written lists were touched")
    return want, ml, n


def long_list(S, n):
    """n entries over scenarios 0 .. S - 1 and the empty slot, every one of them many times, in no order"""
    return [(5 * j + j // 7) % (S + 1) - 1 for j in range(n)]


@pytest.mark.parametrize("cells16", [False, True], ids=["int32", "cells16"])
@pytest.mark.parametrize("name,entries", [("mixed42", 300), ("rows_4097", 300)])
def test_host_moves_of_long_lists(ctx, name, entries, cells16):
    """host lists of 300 entries, repeats and empty slots mixed: several tiles of the scan (rows_4097: stride 5, six tiles), under
    masks 1 and 7, and capacities that cut the list in a later tile"""
    fb, cur, ho = reference(name, cells16)
    select = long_list(fb.n_scenarios, entries)
    assert select.count(-1) >= 10 and len(set(select)) == fb.n_scenarios + 1
    for mask in (1, 7):
        want, _, _ = check_host_moves(ctx, fb, cur, ho, select, mask, cells16, f"{name} long list mask {mask} cells16 {cells16}")
    if name == "rows_4097":
        assert assert_spans_tiles(fb, ho, select, 7, want, cells16=cells16, cur16=cur if cells16 else None) >= 5
    M, Cc = int(want.move_off[-1]), int(want.cell_off[-1])
    _, ml, n = check_host_moves(ctx, fb, cur, ho, select, 7, cells16, f"{name} long list, capacities", caps=(M - 1, Cc // 2), want=want)
    first_tile = -(-SCAN_TILE // max(int(scenario_items(fb).max()), 1))      # listings that reach into the scan's first tile
    assert ml.truncated and int(want.move_off[first_tile]) < n < M - 1, "the cut is not in a later tile"


def test_device_moves_of_a_long_list(ctx):
    """plan.moves_device over a device list of 513 entries with empty slots (-1, and exactly S: no scenario of the tables), on a
    non-default torch stream, twice on one plan under two masks; guards behind the offsets, the records and the cells"""
    import torch
    fb, cur, ho = reference("mixed42", False)
    S = fb.n_scenarios
    select = [(3 * j + j // 16) % (S + 2) - 1 for j in range(512)] + [0]      # -1 .. S; the last tile begins with the last entry
    assert select.count(-1) >= 10 and select.count(S) >= 10 and len(set(select)) == S + 2
    dev = torch.device("cuda", ctx.device)
    plan = native.Plan(ctx, fb)
    try:
        d_cur = torch.from_numpy(cur.copy()).to(dev)
        d_aux = torch.from_numpy(fb.aux).to(dev) if fb.aux.size else None
        d_out = torch.full((max(fb.out_len, 1),), -2, dtype=torch.int32, device=dev)
        d_tr = torch.zeros(max(fb.n_topics, 1) * 16, dtype=torch.uint8, device=dev)
        d_sr = torch.zeros(max(S, 1) * 32, dtype=torch.uint8, device=dev)
        d_sel = torch.tensor(select, dtype=torch.int32, device=dev)
        n = len(select)
        room = native.moves_room(fb, select)
        outs = [SimpleNamespace(move_off=torch.full((n + 2,), -77, dtype=torch.int64, device=dev),
                                cell_off=torch.full((n + 2,), -77, dtype=torch.int64, device=dev),
                                moves=torch.full(((room[0] + 1) * 16,), 0x7B, dtype=torch.uint8, device=dev),
                                cells=torch.full((room[1] + 1,), 0x7B7B, dtype=torch.int32, device=dev)) for _ in range(2)]
        st = torch.cuda.Stream(dev)
        st.wait_stream(torch.cuda.current_stream(dev))
        aux = d_aux.data_ptr() if d_aux is not None else 0
        plan.solve_device(d_cur.data_ptr(), d_out.data_ptr(), d_tr.data_ptr(), d_sr.data_ptr(), aux=aux, stream=st.cuda_stream)
        for o, mask in zip(outs, (7, 1)):
            plan.moves_device(mask, d_sel.data_ptr(), n, d_cur.data_ptr(), d_out.data_ptr(), d_tr.data_ptr(), o.move_off.data_ptr(),
                              o.cell_off.data_ptr(), o.moves.data_ptr(), room[0], o.cells.data_ptr(), room[1], aux=aux, stream=st.cuda_stream)
        st.synchronize()
        for o, mask in zip(outs, (7, 1)):
            want = moves_ref_long(fb, ho, select, mask)
            assert_spans_tiles(fb, ho, select, mask, want, what=f"device list mask {mask}")
            mo, co = o.move_off.cpu().numpy(), o.cell_off.cpu().numpy()
            assert mo[n + 1] == -77 and co[n + 1] == -77, "the guard behind the offsets was written"
            raw, cells = o.moves.cpu().numpy(), o.cells.cpu().numpy()
            got = SimpleNamespace(move_off=mo[:n + 1], cell_off=co[:n + 1], moves=raw.view(abi.MOVE_DTYPE), cells=cells)
            assert_same_moves(want, got, f"device list mask {mask}")
            assert (raw[16 * int(want.move_off[-1]):] == 0x7B).all() and (cells[int(want.cell_off[-1]):] == 0x7B7B).all(), "written behind the list"
            for j, s in enumerate(select):
                assert 0 <= s < S or mo[j] == mo[j + 1]
    finally:
        plan.close()


_WHATIF_RUNS = None


def _whatif_runs():
    """WhatIf.solve over the 302 variants through the library, each form once: every row, the moves of all three kinds, the
    replica moves"""
    global _WHATIF_RUNS
    if _WHATIF_RUNS is None:
        w, vs, _, _, _ = whatif_solved()
        _WHATIF_RUNS = (w.solve(vs), w.solve(vs, moves=("replicas", "leader", "order")), w.solve(vs, moves=("replicas",)))
    return _WHATIF_RUNS


def test_whatif_solve_moves_of_every_variant_equal_the_checkers(ctx):
    """WhatIf.solve(variants, moves=...) through the library, not a stand-in for it: 302 variants x stride 5 = 1510 entries, six
    tiles of the scan.  Every variant's records and cells are the checker's over the oracle's solve."""
    w, vs, fb, ho, _ = whatif_solved()
    S = fb.n_scenarios
    full, lists, sets = _whatif_runs()
    for mask, res in ((7, lists), (1, sets)):
        want = moves_ref_long(fb, ho, range(S), mask)
        assert assert_spans_tiles(fb, ho, range(S), mask, want, what=f"what-if mask {mask}") == 5
        for s, (f, r) in enumerate(zip(full, res)):
            recs, cells = r._moves
            lo, hi, clo, chi = (int(v) for v in (want.move_off[s], want.move_off[s + 1], want.cell_off[s], want.cell_off[s + 1]))
            assert r._moves_mask == mask and recs.tobytes() == want.moves[lo:hi].tobytes() and np.array_equal(cells, want.cells[clo:chi]), (s, f.label)
            assert (r.status, r.moved_replicas, r.digest) == (f.status, f.moved_replicas, f.digest) == \
                (int(ho.scenario_results["status"][s]), int(ho.scenario_results["moved_replicas"][s]), int(ho.scenario_results["digest"][s]))
            if mask == 1 and f.status == abi.KAS_OK:              # (every record of a replica list is a partition of the reassignment)
                assert recs.size == f.moved_partitions, f.label


def test_whatif_solve_moves_applied_to_the_snapshot_give_the_assignment(ctx):
    """for every variant that solves, VariantResult.moves() of all three kinds applied to the snapshot is the assignment of
    solve(variants), row for row (compared as arrays: assignment() is a Python loop over every row, taken for ten variants)"""
    w, vs, fb, ho, _ = whatif_solved()
    full, lists, sets = _whatif_runs()
    T = len(w.topic_names)
    snap = [w.cur[int(w.cur_off[t]):][:len(w.part_ids[t]) * w.widths[t]].reshape(-1, w.widths[t]) for t in range(T)]
    row_of = [{int(p): i for i, p in enumerate(w.part_ids[t])} for t in range(T)]
    cur = {name: {int(p): [int(b) for b in snap[t][i]] for i, p in enumerate(w.part_ids[t])} for t, name in enumerate(w.topic_names)}
    t_of = {name: t for t, name in enumerate(w.topic_names)}
    solves = 0
    for s, (f, r, a) in enumerate(zip(full, lists, sets)):
        if f.status != abi.KAS_OK:
            continue
        solves += 1
        moves = r.moves()
        new = [rows.copy() for rows in snap]                      # the rows of variant s as the out pool of solve(variants) holds them
        for name, p, reps, _ in moves:
            row = new[t_of[name]][row_of[t_of[name]][p]]
            row[:] = -1
            row[:len(reps)] = reps
        for t in range(T):
            td = fb.topics[s * T + t]
            assert int(td["out_width"]) == w.widths[t]
            rows = f._out[int(td["out_off"]):][:new[t].size].reshape(new[t].shape)
            assert np.array_equal(new[t], rows), (f.label, w.topic_names[t], np.nonzero((new[t] != rows).any(axis=1))[0][:4])
        if solves <= 10:
            as_dict = {name: dict(rows) for name, rows in cur.items()}
            for name, p, reps, _ in moves:
                as_dict[name][p] = reps
            for name in w.topic_names:
                assert as_dict[name] == f.assignment(name), (f.label, name)
            assert len(a.reassignment()["partitions"]) == f.moved_partitions, f.label
    assert solves >= 100


@pytest.mark.parametrize("cells16", [False, True], ids=["int32", "cells16"])
def test_host_moves_of_every_whatif_variant(ctx, cells16):
    """the raw call behind WhatIf.solve(variants, moves=...), n = S = 302, into guarded arrays; in 16-bit cells over the batch with
    a cur table per variant"""
    _, _, fb, ho, _ = whatif_solved()
    cur = fb.cur
    if cells16:
        fb, sr16, out16 = tg._whatif16()
        ho = SimpleNamespace(out=out16, topic_results=ho.topic_results, scenario_results=sr16)
        cur = to_cells16(fb)
    for mask in (1, 7):
        check_host_moves(ctx, fb, cur, ho, None, mask, cells16, f"what-if raw call, cells16 {cells16}, mask {mask}")


# ---- calls cut into scenario ranges ---------------------------------------------------------------------------------------
def _ranges_list(ho, S, shift=0):
    """a short list over test_choose_gpu's batch of 44 that names scenarios of both halves (the two ranges of a cut call), one of
    them twice, and an empty slot; only scenarios that solve: a failed one has no moves"""
    ok = np.nonzero(ho.scenario_results["status"][:S] == abi.KAS_OK)[0]
    lo, hi = ok[ok < S // 2], ok[ok >= S // 2]
    assert lo.size >= 1 and hi.size >= 1
    return [int(hi[-1]) + shift, -1, int(lo[0]), int(hi[0]) + shift, int(lo[-1]), int(hi[-1]) + shift]


def _assert_every_listed_moves(want, select, half):
    assert all(want.n_moves[j] >= 1 for j, s in enumerate(select) if s >= 0), "a listed scenario without moves"
    assert any(0 <= s < half for s in select) and any(s >= half for s in select), "the list names one range only"


def test_host_moves_over_scenario_ranges(ctx, monkeypatch):
    """44 x 100k x 200 brokers with a `cur` per scenario: 52.8 MB, which the planner cuts into two ranges (tests/test_moves_cpu.py
    pins the count).  The moves pass runs on the first range's stream behind both ranges' done events; stride 98, so the list of
    six is three tiles of the scan.  Then capacities that truncate (the marker memset and the probes behind a cut call), then three
    ranges (KAS_HOST_RANGES, read per call: the issue order with a lag of two)"""
    fb, ho, _, _ = tg._ranges_batch()
    S = fb.n_scenarios
    select = _ranges_list(ho, S)
    wants = {}
    for mask in (1, 7):
        hits = ctx.host_stats()[1]
        wants[mask], _, _ = check_host_moves(ctx, fb, fb.cur, ho, select, mask, False, f"two ranges, mask {mask}")
        _assert_every_listed_moves(wants[mask], select, S // 2)
        if mask == 7:                                             # (the second call: every range finds its plan)
            assert ctx.host_stats()[1] - hits == 2, "the call was not cut into two scenario ranges"
    M, Cc = int(wants[7].move_off[-1]), int(wants[7].cell_off[-1])
    hits = ctx.host_stats()[1]
    _, ml, n = check_host_moves(ctx, fb, fb.cur, ho, select, 7, False, "two ranges, capacities", caps=(M - 1, Cc // 2), want=wants[7])
    assert ml.truncated and int(wants[7].move_off[3]) < n < M - 1 and ctx.host_stats()[1] - hits == 2   # (the cut: behind the first tile)
    monkeypatch.setenv("KAS_HOST_RANGES", "3")
    for mask in (1, 7):
        hits = ctx.host_stats()[1]
        check_host_moves(ctx, fb, fb.cur, ho, select, mask, False, f"three ranges, mask {mask}", want=wants[mask])
        if mask == 7:
            assert ctx.host_stats()[1] - hits == 3, "the call was not cut into three scenario ranges"


def test_choose_moves_and_front_over_scenario_ranges(ctx):
    """the same batch through kas_solve_host_choose_moves (k = 3, with and without rows) and kas_solve_host_front with a mask: the
    waits for the ranges stand in front of the rank kernel, the moves pass behind it on the same stream"""
    from test_front_gpu import _check_host_front
    from front_ref import front_choice_ref
    fb, ho, imp, _ = tg._ranges_batch()
    S = fb.n_scenarios
    sr = ho.scenario_results[:S]
    keys = ("max_outbound", "moved_replicas")
    want_ch = choose_ref(fb, sr, ho.out, imp, keys, 3)
    assert want_ch.n_ok >= 3 and bool((want_ch.chosen < S // 2).any()) and bool((want_ch.chosen >= S // 2).any()), \
        ("the winners come from one half of the batch", want_ch.chosen)
    native.solve_host_choose_moves(fb, keys, 3, 1, ctx=ctx)      # (a first call: the ranges' plans)
    for mask, rows in ((1, True), (7, True), (7, False)):
        hits = ctx.host_stats()[1]
        got_ho, ch, ml = native.solve_host_choose_moves(fb, keys, 3, mask, rows=rows, ctx=ctx)
        assert ctx.host_stats()[1] - hits == 2, "the call was not cut into two scenario ranges"
        if rows:
            assert_same_choice(want_ch, ch, f"choice over ranges, mask {mask}")
        else:
            assert ch.rows.size == 0 and np.array_equal(ch.chosen, want_ch.chosen) and np.array_equal(ch.rank, want_ch.rank)
        want = moves_ref_long(fb, ho, want_ch.chosen, mask)
        _assert_every_listed_moves(want, list(want_ch.chosen), S // 2)
        assert_spans_tiles(fb, ho, want_ch.chosen, mask, want, what="the winners over ranges")
        assert_same_moves(want, ml, f"choice over ranges, mask {mask}, rows {rows}")
        assert ml.moves.size == want.moves.size and ml.cells.size == want.cells.size and not ml.truncated
    front = front_choice_ref(fb, sr, ho.out, imp, keys, S)
    assert bool((front.order < S // 2).any()) and bool((front.order >= S // 2).any())
    k = min(int(front.order.size), 3)
    for mask in (1, 7):
        _check_host_front(ctx, fb, sr, ho.out, imp, keys, k, (), False, f"front over ranges, mask {mask}", mask=mask, moves_of=(fb, ho, None))


def test_host16_moves_over_scenario_ranges(ctx):
    """16-bit cells: 44 scenarios are 26.4 MB and stay one range, so the batch is laid out twice — scenario 44 + s is scenario s
    again with a cur table and a node range of its own, and the oracle's records and rows of the copy are the original's — and the
    52.8 MB of the 88 are cut into two ranges"""
    fb44, ho44, _, out16 = tg._ranges_batch()
    S, P = 88, 100_000
    ids = [fb44.node_id[int(o):int(o) + int(n)] for o, n in zip(fb44.scen["node_off"], fb44.scen["n_nodes"])]
    racks = [fb44.node_rack[int(o):int(o) + int(n)] for o, n in zip(fb44.scen["node_off"], fb44.scen["n_nodes"])]
    fb = node_set_batch(ids + ids, racks + racks, P, 3, 3, cur=np.concatenate([fb44.cur, fb44.cur]))
    assert np.array_equal(fb.topics["out_off"][:44], fb44.topics["out_off"]) and fb.out_len == 2 * fb44.out_len
    ho = SimpleNamespace(out=np.concatenate([out16, out16]), topic_results=np.concatenate([ho44.topic_results[:44], ho44.topic_results[:44]]),
                         scenario_results=np.concatenate([ho44.scenario_results[:44], ho44.scenario_results[:44]]))
    cur16 = to_cells16(fb)
    select = _ranges_list(ho44, 44, shift=44)
    for mask in (1, 7):
        hits = ctx.host_stats()[1]
        want, _, _ = check_host_moves(ctx, fb, cur16, ho, select, mask, True, f"88 scenarios of 16-bit cells, mask {mask}")
        _assert_every_listed_moves(want, select, S // 2)
        if mask == 7:
            assert ctx.host_stats()[1] - hits == 2, "the call was not cut into two scenario ranges"

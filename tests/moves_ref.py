"""NumPy / Python restatement of the move list (include/kas_abi.h: kas_move / kas_moves) over a FlatBatch, the HostOutputs of a
solve with every row in place, a list of scenarios and a mask.  The checker of tests/test_moves_*.py, written from the header's
text, not a product path.

For each listed scenario, over each of its topics whose status is KAS_OK, in descriptor order, and each row p ascending:
C = the first clen cells of cur[p] (clen = cur_len[p], or cur_width), O = the cells of out[p] up to the first pad.  Flags:
REPLICAS 1 = olen > 0 and set(O) != set(C); LEADER 2 = olen > 0 and (clen == 0 or O[0] != C[0]); ORDER 4 = olen > 0, set(O) ==
set(C) and O != C as lists.  A row is a move under mask m iff flags & m.  A record is (topic within the scenario, part_id[p] or p,
flags, olen, cells of O not in C, cells of C not in O, where its list starts in the scenario's block of cells).
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from kafka_assigner_amd import abi

REPLICAS, LEADER, ORDER = abi.KAS_MOVE_REPLICAS, abi.KAS_MOVE_LEADER, abi.KAS_MOVE_ORDER
_NO = -(1 << 40)                        # no cell has this value


def topic_rows(fb, ho, t: int, cells16: bool = False, cur16=None):
    """(flags, olen, gained, lost, O, partition ids) of every row of topic t, whatever its status"""
    td = fb.topics[t]
    P, cw, ow = max(int(td["n_partitions"]), 0), int(td["cur_width"]), int(td["out_width"])
    co, oo = int(td["cur_off"]), int(td["out_off"])
    cur = cur16 if cells16 else fb.cur
    pad = abi.KAS_CELL16_NONE if cells16 else -1
    C = cur[co:co + P * cw].astype(np.int64).reshape(P, cw)
    O = ho.out[oo:oo + P * ow].astype(np.int64).reshape(P, ow)
    lo = int(td["cur_len_off"])
    clen = np.clip(fb.aux[lo:lo + P].astype(np.int64), 0, cw) if lo >= 0 else np.full(P, cw, dtype=np.int64)
    cmask = np.arange(cw)[None, :] < clen[:, None]
    omask = np.cumprod(O != pad, axis=1).astype(bool)
    olen = omask.sum(axis=1)
    in_c = ((O[:, :, None] == C[:, None, :]) & cmask[:, None, :]).any(axis=2)       # [p, k]: O[k] is a cell of C
    in_o = ((C[:, :, None] == O[:, None, :]) & omask[:, None, :]).any(axis=2)       # [p, j]: C[j] is a cell of O
    gained = (omask & ~in_c).sum(axis=1)
    lost = (cmask & ~in_o).sum(axis=1)
    same_sets = (gained == 0) & (lost == 0)
    w = max(cw, ow)
    Cp = np.full((P, w), _NO, np.int64); Cp[:, :cw] = np.where(cmask, C, _NO)
    Op = np.full((P, w), _NO, np.int64); Op[:, :ow] = np.where(omask, O, _NO)
    same_lists = (Cp == Op).all(axis=1)
    first_differs = (clen == 0) | (Op[:, 0] != Cp[:, 0]) if w else np.ones(P, bool)
    some = olen > 0
    flags = (some & ~same_sets) * REPLICAS + (some & first_differs) * LEADER + (some & same_sets & ~same_lists) * ORDER
    po = int(td["part_id_off"])
    part = fb.aux[po:po + P].astype(np.int64) if po >= 0 else np.arange(P, dtype=np.int64)
    return flags.astype(np.int64), olen, gained, lost, O, part


def scenario_rows(fb, ho, s: int, cells16: bool = False, cur16=None):
    """[(topic within the scenario, flags, olen, gained, lost, O, partition ids)] over the scenario's KAS_OK topics"""
    b, c = int(fb.scen["topic_begin"][s]), max(int(fb.scen["topic_count"][s]), 0)
    return [(k,) + topic_rows(fb, ho, b + k, cells16, cur16) for k in range(c) if int(ho.topic_results["status"][b + k]) == abi.KAS_OK]


def moves_ref(fb, ho, select, mask: int, cells16: bool = False, cur16=None):
    """The complete move list of `select` under `mask`: move_off / cell_off int64 [n + 1], moves abi.MOVE_DTYPE, cells (int32, or
    uint16 with cells16), and per listed scenario the rows that are moves / are not (`n_moves`, `n_rest`)."""
    if cells16 and cur16 is None:
        from kafka_assigner_amd.flatten import to_cells16
        cur16 = to_cells16(fb)
    recs, cells, move_off, cell_off, n_rest = [], [], [0], [0], []
    n_recs = n_cells = 0
    for s in [int(x) for x in select]:
        at, rest = 0, 0
        if 0 <= s < fb.n_scenarios:
            for k, flags, olen, gained, lost, O, part in scenario_rows(fb, ho, s, cells16, cur16):
                hit = (flags & mask) != 0
                rest += int((~hit).sum())
                rows = np.nonzero(hit)[0]                           # the topic's moves, rows ascending
                lens = olen[rows]
                r = np.zeros(rows.size, abi.MOVE_DTYPE)
                r["topic"], r["partition"], r["flags"], r["len"], r["gained"], r["lost"] = k, part[rows], flags[rows], lens, gained[rows], lost[rows]
                r["cell_at"] = at + np.cumsum(lens) - lens          # lists lie back to back, in row order
                recs.append(r)
                cells.append(O[rows][np.arange(O.shape[1])[None, :] < lens[:, None]])      # each row's first olen cells
                at += int(lens.sum())
                n_recs += int(rows.size)
            n_cells += at
        move_off.append(n_recs); cell_off.append(n_cells); n_rest.append(rest)
    return SimpleNamespace(move_off=np.asarray(move_off, np.int64), cell_off=np.asarray(cell_off, np.int64),
                           moves=np.concatenate(recs) if recs else np.zeros(0, abi.MOVE_DTYPE),
                           cells=(np.concatenate(cells) if cells else np.zeros(0, np.int64)).astype(np.uint16 if cells16 else np.int32),
                           n_moves=np.diff(np.asarray(move_off, np.int64)), n_rest=np.asarray(n_rest, np.int64))


def moves_ref_long(fb, ho, select, mask: int, cells16: bool = False, cur16=None):
    """moves_ref of a long list with repeats: each distinct entry's block is moves_ref of the one-entry list, computed once and
    repeated behind shifted offsets (a record's cell_at counts from its block's first cell, so a block is the same wherever it
    lies; that repeated listings hold equal contents is the contract, and test_select_lists pins it)"""
    select = [int(s) for s in select]
    if cells16 and cur16 is None:
        from kafka_assigner_amd.flatten import to_cells16
        cur16 = to_cells16(fb)
    blocks = {s: moves_ref(fb, ho, [s], mask, cells16, cur16) for s in sorted(set(select))}
    n_moves = np.array([blocks[s].moves.size for s in select], np.int64)
    n_cells = np.array([blocks[s].cells.size for s in select], np.int64)
    some = [s for s in select if blocks[s].moves.size]
    return SimpleNamespace(move_off=np.concatenate([[0], np.cumsum(n_moves)]).astype(np.int64),
                           cell_off=np.concatenate([[0], np.cumsum(n_cells)]).astype(np.int64),
                           moves=np.concatenate([blocks[s].moves for s in some]) if some else np.zeros(0, abi.MOVE_DTYPE),
                           cells=np.concatenate([blocks[s].cells for s in some]) if some else np.zeros(0, np.uint16 if cells16 else np.int32),
                           n_moves=n_moves, n_rest=np.array([int(blocks[s].n_rest[0]) for s in select], np.int64))


# ---- the guard of the tests that take the scan kernel across its tiles ---------------------------------------------------------
ITEM_ROWS = 1024                        # KAS_MOVES_ITEM_ROWS: rows of an item
SCAN_TILE = 256                         # KAS_MOVES_BLOCK: entries the scan kernel takes per step of its loop


def scenario_items(fb) -> np.ndarray:
    """int64 [S]: items of each scenario — every topic's ceil(P / ITEM_ROWS), whatever its status; the launch stride is the
    largest of them, at least 1"""
    per_topic = -(-np.clip(fb.topics["n_partitions"], 0, None).astype(np.int64) // ITEM_ROWS)
    return np.array([int(per_topic[int(b):int(b) + max(int(c), 0)].sum()) for b, c in zip(fb.scen["topic_begin"], fb.scen["topic_count"])], np.int64)


def scan_entries(fb, ho, select, mask: int, cells16: bool = False, cur16=None) -> np.ndarray:
    """int64 [n * stride]: the moves of every (listed scenario, item) entry of the table the scan kernel walks, from the checker's
    flags alone; entries of empty slots and of items a scenario does not have hold 0"""
    items = scenario_items(fb)
    stride = max(int(items.max()) if items.size else 0, 1)
    select = [int(s) for s in select]
    per = {}
    for s in set(select):
        row = np.zeros(stride, np.int64)
        if 0 <= s < fb.n_scenarios:
            b, c = int(fb.scen["topic_begin"][s]), max(int(fb.scen["topic_count"][s]), 0)
            at = 0
            for k in range(c):
                P = max(int(fb.topics["n_partitions"][b + k]), 0)
                blocks = -(-P // ITEM_ROWS)
                if int(ho.topic_results["status"][b + k]) == abi.KAS_OK and P:
                    hit = (topic_rows(fb, ho, b + k, cells16, cur16)[0] & mask) != 0
                    row[at:at + blocks] = np.add.reduceat(hit.astype(np.int64), np.arange(0, P, ITEM_ROWS))
                at += blocks
        per[s] = row
    return np.concatenate([per[s] for s in select]) if select else np.zeros(0, np.int64)


def assert_spans_tiles(fb, ho, select, mask: int, want, cells16: bool = False, cur16=None, what: str = "") -> int:
    """The guard: the table has more than SCAN_TILE entries, and at every multiple of SCAN_TILE below its size the list has a move
    in an entry before the boundary and one at or behind it — a carry lost or doubled there changes move_off or the records.
    Returns the number of boundaries."""
    if cells16 and cur16 is None:
        from kafka_assigner_amd.flatten import to_cells16
        cur16 = to_cells16(fb)
    per = scan_entries(fb, ho, select, mask, cells16, cur16)
    n = len(select)
    assert n and per.size % n == 0
    assert np.array_equal(per.reshape(n, -1).sum(axis=1), np.diff(want.move_off)), (what, "the entries do not add up to the checker's list")
    assert per.size > SCAN_TILE, (what, "one tile", per.size)
    before = np.cumsum(per)
    edges = list(range(SCAN_TILE, per.size, SCAN_TILE))
    for b in edges:
        assert before[b - 1] >= 1 and before[-1] - before[b - 1] >= 1, (what, "no move on one side of entry", b)
    return len(edges)


def written_prefix(want, moves_cap: int, cells_cap: int):
    """(records, cells) that the capacities let through: a move is written iff its index is below moves_cap and its list ends at
    or before cells_cap; list ends grow with the index, so these are prefixes"""
    m = min(int(want.move_off[-1]), max(int(moves_cap), 0))
    if m == 0:
        return 0, 0
    block = np.searchsorted(want.move_off, np.arange(m), side="right") - 1     # the listed scenario whose block holds record i
    ends = want.cell_off[block] + want.moves["cell_at"][:m].astype(np.int64) + want.moves["len"][:m].astype(np.int64)
    over = np.nonzero(ends > cells_cap)[0]
    n = int(over[0]) if over.size else m
    return n, int(ends[n - 1]) if n else 0


def assert_same_moves(want, got, what: str = "", moves_cap=None, cells_cap=None):
    """`got` (move_off, cell_off, moves, cells: arrays at least as long as what was written) against the checker's list"""
    assert np.array_equal(want.move_off, got.move_off), (what, "move_off", want.move_off[:8], got.move_off[:8])
    assert np.array_equal(want.cell_off, got.cell_off), (what, "cell_off", want.cell_off[:8], got.cell_off[:8])
    n, used = int(want.move_off[-1]), int(want.cell_off[-1])
    if moves_cap is not None:
        n, used = written_prefix(want, moves_cap, cells_cap)
    for f in abi.MOVE_DTYPE.names:
        bad = np.nonzero(want.moves[f][:n] != got.moves[f][:n])[0]
        assert bad.size == 0, f"{what}: record {bad[0]} field {f}: want {want.moves[f][bad[0]]}, got {got.moves[f][bad[0]]}"
    bad = np.nonzero(want.cells[:used].astype(np.int64) != got.cells[:used].astype(np.int64))[0]
    assert bad.size == 0, f"{what}: cell {bad[0] if bad.size else 0}"
    return n, used

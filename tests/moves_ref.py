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
    for s in [int(x) for x in select]:
        at, rest = 0, 0
        if 0 <= s < fb.n_scenarios:
            for k, flags, olen, gained, lost, O, part in scenario_rows(fb, ho, s, cells16, cur16):
                hit = (flags & mask) != 0
                rest += int((~hit).sum())
                for p in np.nonzero(hit)[0]:
                    recs.append((k, int(part[p]), int(flags[p]), int(olen[p]), int(gained[p]), int(lost[p]), at))
                    cells.extend(int(v) for v in O[p, :int(olen[p])])
                    at += int(olen[p])
        move_off.append(len(recs)); cell_off.append(len(cells)); n_rest.append(rest)
    return SimpleNamespace(move_off=np.asarray(move_off, np.int64), cell_off=np.asarray(cell_off, np.int64),
                           moves=np.array(recs, dtype=abi.MOVE_DTYPE) if recs else np.zeros(0, abi.MOVE_DTYPE),
                           cells=np.asarray(cells, dtype=np.uint16 if cells16 else np.int32),
                           n_moves=np.diff(np.asarray(move_off, np.int64)), n_rest=np.asarray(n_rest, np.int64))


def written_prefix(want, moves_cap: int, cells_cap: int):
    """(records, cells) that the capacities let through: a move is written iff its index is below moves_cap and its list ends at
    or before cells_cap; list ends grow with the index, so these are prefixes"""
    n = 0
    used = 0
    j = 0
    for i in range(min(int(want.move_off[-1]), moves_cap)):
        while want.move_off[j + 1] <= i:
            j += 1
        end = int(want.cell_off[j]) + int(want.moves["cell_at"][i]) + int(want.moves["len"][i])
        if end > cells_cap:
            break
        n, used = i + 1, end
    return n, used


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

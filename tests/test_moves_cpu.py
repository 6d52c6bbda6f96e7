"""The move list (include/kas_abi.h: kas_move / kas_moves) without a GPU.

- The three kernel bodies of the moves pass (kafka-assigner_amd/csrc/kas_moves_body.h) compiled with g++ against tests/emu/kas_wave.h
  and stepped on CPU fibers (tests/emu/moves_driver.cpp), against the Python checker (tests/moves_ref.py): oracle-solved batches of
  tests/impact_batches.py in both cell layouts under masks 1, 2, 4, 3 and 7, with the guard that keeps them meaningful; synthetic
  cur / out tables around every row count at which the code takes another path; select lists; capacities; invariants; determinism;
  lists that take the scan kernel across its tiles of 256 entries (tile edges exactly, an edge inside one scenario's items, a tile
  of full items, capacities that cut in a later tile), each behind a guard that a lost or doubled carry would show.
- The host call planner (csrc/kas_host_call.h) with the moves arguments: refusals in order, buffer sizes, unchanged plans, the
  scenario ranges of the calls the GPU tests cut.
- The ABI: entries declared and exported, struct layouts against a compiled probe, version still 6.
- WhatIf.solve / best with moves=..., the library's host calls replaced by the oracle and the checker.
"""
import ctypes as C
import dataclasses
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from impact_batches import solved, whatif_inputs
from kafka_assigner_amd import abi, native
from kafka_assigner_amd.flatten import FlatBatch, batch_desc, index_form, to_cells16
from moves_ref import (ITEM_ROWS, LEADER, ORDER, REPLICAS, SCAN_TILE, assert_same_moves, assert_spans_tiles, moves_ref, moves_ref_long,
                       scenario_items, scenario_rows, written_prefix)
from oracle_lib import oracle_solve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "kafka-assigner_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "kas_abi.h")
E_INVALID, E_UNSUPPORTED = abi.KAS_E_INVALID_ARG, abi.KAS_E_UNSUPPORTED
ORACLE_BATCHES = ["mixed7", "mixed42", "row_counts", "degenerate", "widths_4_5", "widths_6_8", "sparse", "shared_node_range", "rows_4097"]
MASKS = [1, 2, 4, 3, 7]
GUARD = 1                               # elements behind every output array
_LIB = None


# ---- the emulator ---------------------------------------------------------------------------------------------------------
def _emu_lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    so = os.path.join(EMU, "libkas_emu_moves.so")
    srcs = [os.path.join(EMU, "moves_driver.cpp"), os.path.join(EMU, "emu_driver.cpp")]
    deps = srcs + [os.path.join(EMU, "kas_wave.h"), HEADER] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        tmp = so + ".tmp%d" % os.getpid()
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unused-parameter", "-Wno-unknown-pragmas",
                               "-I" + os.path.join(ROOT, "tests"), "-I" + CSRC, "-I" + os.path.join(ROOT, "include"),
                               "-o", tmp] + srcs)
        os.replace(tmp, so)
    L = C.CDLL(so)
    L.kas_emu_moves.restype = C.c_int
    L.kas_emu_moves.argtypes = [C.POINTER(abi.BatchDesc), C.POINTER(abi.Tables), C.c_int, C.c_void_p, C.c_int32, C.POINTER(abi.Moves),
                                C.c_uint32, C.c_char_p, C.c_int]
    L.kas_emu_moves_room.restype = None
    L.kas_emu_moves_room.argtypes = [C.POINTER(abi.BatchDesc), C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int64)]
    L.kas_emu_moves_host_call.restype = C.c_int
    L.kas_emu_moves_host_call.argtypes = [C.POINTER(abi.BatchDesc), C.POINTER(C.c_int64), C.c_uint, C.c_int, C.POINTER(abi.ChooseSpec),
                                          C.c_void_p, C.c_int32, C.POINTER(abi.Moves), C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                          C.c_char_p, C.c_int]
    L.kas_emu_moves_buffers.restype = C.c_int
    L.kas_emu_moves_item_rows.restype = C.c_int
    _LIB = L
    return L


def ITEM():
    return _emu_lib().kas_emu_moves_item_rows()


def emu_moves_raw(fb, cur, out, tr, select, mask, mode=0, moves_cap=0, cells_cap=0, lds_fill=0xCDCDCDCD):
    """kas_emu_moves: (rc, error text, arrays) — every output pre-filled with a sentinel, one guard element behind every array"""
    sel = np.ascontiguousarray(select, np.int32)
    n = int(sel.size)
    got = SimpleNamespace(move_off=np.full(n + 1 + GUARD, -77, np.int64), cell_off=np.full(n + 1 + GUARD, -77, np.int64),
                          moves=np.zeros(moves_cap + GUARD, abi.MOVE_DTYPE), cells=np.full(cells_cap + GUARD, 0x7B7B, np.int32 if mode == 0 else np.uint16))
    got.moves.view(np.uint8)[...] = 0x7B
    t = abi.Tables()
    t.cur, t.out, t.aux, t.topic_results = cur.ctypes.data, out.ctypes.data, fb.aux.ctypes.data if fb.aux.size else None, tr.ctypes.data
    mv = abi.Moves(mask, 0, got.move_off.ctypes.data, got.cell_off.ctypes.data, got.moves.ctypes.data, moves_cap, got.cells.ctypes.data, cells_cap)
    bd = batch_desc(fb)
    err = C.create_string_buffer(512)
    rc = _emu_lib().kas_emu_moves(C.byref(bd), C.byref(t), mode, sel.ctypes.data if n else None, n, C.byref(mv), lds_fill, err, 512)
    return rc, err.value.decode(), got


def emu_moves(fb, cur, out, tr, select, mask, want, mode=0, moves_cap=None, cells_cap=None, lds_fill=0xCDCDCDCD, what=""):
    """... compared with the checker's list `want`: offsets complete, the written prefix equal, nothing else touched.
    Capacities default to exactly what the list needs."""
    n = len(select)
    moves_cap = int(want.move_off[-1]) if moves_cap is None else moves_cap
    cells_cap = int(want.cell_off[-1]) if cells_cap is None else cells_cap
    rc, err, got = emu_moves_raw(fb, cur, out, tr, select, mask, mode, moves_cap, cells_cap, lds_fill)
    assert rc == 0, (what, rc, err)
    assert got.move_off[n + 1] == -77 and got.cell_off[n + 1] == -77, (what, "the guard behind the offsets was written")
    got.move_off, got.cell_off = got.move_off[:n + 1], got.cell_off[:n + 1]
    written, used = assert_same_moves(want, got, what, moves_cap, cells_cap)
    assert (got.moves.view(np.uint8)[16 * written:] == 0x7B).all(), (what, "records beyond the written ones were touched")
    assert (got.cells[used:] == 0x7B7B).all(), (what, "cells beyond the written lists were touched")
    got.moves, got.cells = got.moves[:written], got.cells[:used]
    return got


# ---- oracle-solved batches ------------------------------------------------------------------------------------------------
_FORMS = {}


def forms(name):
    """mode -> (fb, cur pool, ho with the out pool in that cell layout) of a named batch: int32 cells (0) and 16-bit cells (1)"""
    if name not in _FORMS:
        fb, ho, _ = solved(name)
        ho_idx = oracle_solve(index_form(fb))                                   # int32 node indices, -1 pads
        out16 = np.where(ho_idx.out < 0, abi.KAS_CELL16_NONE, ho_idx.out).astype(np.uint16)
        ho16 = SimpleNamespace(out=out16, topic_results=ho_idx.topic_results, scenario_results=ho_idx.scenario_results)
        assert np.array_equal(ho_idx.topic_results["status"], ho.topic_results["status"])
        _FORMS[name] = {0: (fb, fb.cur, ho), 1: (fb, to_cells16(fb), ho16)}
    return _FORMS[name]


def check(fb, cur, ho, select, mask, mode, what, **kw):
    want = moves_ref(fb, ho, select, mask, cells16=mode == 1, cur16=cur if mode == 1 else None)
    return want, emu_moves(fb, cur, ho.out, ho.topic_results, select, mask, want, mode=mode, what=what, **kw)


@pytest.mark.parametrize("mode", [0, 1], ids=["int32", "cells16"])
@pytest.mark.parametrize("name", ORACLE_BATCHES)
def test_emulated_moves_of_oracle_batches(name, mode):
    fb, cur, ho = forms(name)[mode]
    select = list(range(fb.n_scenarios))
    for mask in MASKS:
        want = moves_ref(fb, ho, select, mask, cells16=mode == 1, cur16=cur if mode == 1 else None)
        if mask in (1, 4, 7):                                      # the guard, on the oracle's result alone
            assert want.n_moves.sum() >= 1 and want.n_rest.sum() >= 1, (name, mask, int(want.n_moves.sum()), int(want.n_rest.sum()))
        emu_moves(fb, cur, ho.out, ho.topic_results, select, mask, want, mode=mode, what=f"{name} mode {mode} mask {mask}")


def test_emulated_moves_narrowing_form():
    """int32 node-index cells in cur / out, 16-bit list cells out: the widened 16-bit host call"""
    fb, cur16, ho16 = forms("mixed42")[1]
    fbi = index_form(fb)
    hoi = oracle_solve(fbi)
    want = moves_ref(fb, ho16, range(fb.n_scenarios), 7, cells16=True, cur16=cur16)
    emu_moves(fbi, fbi.cur, hoi.out, hoi.topic_results, list(range(fb.n_scenarios)), 7, want, mode=2, what="narrowing")


@pytest.mark.parametrize("name", ORACLE_BATCHES)
def test_invariants_against_the_solve_records(name):
    """mask 7: sum of gained == moved_replicas, LEADER flags == the impact checker's leaders_moved, REPLICAS flags ==
    moved_partitions where no row of the scenario has olen == 0"""
    fb, ho, imp = solved(name)
    S = fb.n_scenarios
    _, got = check(fb, fb.cur, ho, list(range(S)), 7, 0, name)
    for s in range(S):
        recs = got.moves[int(got.move_off[s]):int(got.move_off[s + 1])]
        assert int(recs["gained"].sum()) == int(ho.scenario_results["moved_replicas"][s]), (name, s)
        assert int(((recs["flags"] & LEADER) != 0).sum()) == int(imp[1]["leaders_moved"][s]) or int(fb.scen["n_nodes"][s]) <= 0, (name, s)
        if all((olen > 0).all() for _, _, olen, _, _, _, _ in scenario_rows(fb, ho, s)):
            assert int(((recs["flags"] & REPLICAS) != 0).sum()) == int(ho.scenario_results["moved_partitions"][s]), (name, s)
        assert not ((recs["flags"] & REPLICAS) != 0)[(recs["flags"] & ORDER) != 0].any()


# ---- synthetic tables -----------------------------------------------------------------------------------------------------
class _Tables:
    """cur / out tables with no solve, lists `w` wide, topic by topic; rows of the kinds: unchanged, reordered, replaced, out all
    pad, ragged cur, a lost replica ("mixed": all of them at random)"""

    def __init__(self, w, rng):
        self.w, self.rng = w, rng
        self.cur, self.out, self.aux, self.topics, self.status = [], [], [], [], []

    def topic(self, P, kind, part_ids=False, ok=True):
        w, rng, cur, out, aux, topics, status = self.w, self.rng, self.cur, self.out, self.aux, self.topics, self.status
        O = np.full((P, w), -1, np.int64)
        Cc = np.full((P, w), -1, np.int64)
        clen = np.zeros(P, np.int64)
        for p in range(P):
            k = {"mixed": int(rng.integers(0, 6)), "all": 2, "none": 0, "order": 1, "allpad": 3}[kind]
            olen = w if kind != "mixed" else int(rng.integers(1, w + 1))
            o = rng.choice(40, olen, replace=False)
            c, cl = o.copy(), olen                                   # 0: unchanged
            if k == 1 and olen > 1:                                  # reordered only
                c = np.roll(o, 1)
            elif k == 2:                                             # replaced: some cells from another id range
                c = o.copy(); cut = int(rng.integers(0, olen)); c[cut:] = 100 + rng.choice(40, olen - cut, replace=False)
            elif k == 3:                                             # out all pad: never a move, whatever cur holds
                olen = 0
            elif k == 4:                                             # ragged cur: clen 0 .. w of random cells
                cl = int(rng.integers(0, w + 1)); c = rng.choice(45, max(cl, 1), replace=False)[:cl]
            elif k == 5 and olen > 1:                                # same leader, another follower order or a lost replica
                cl = olen - 1; c = o[:cl]
            O[p, :olen] = o[:olen]
            Cc[p, :len(c)] = c; clen[p] = min(cl, len(c))
        t = np.zeros(1, abi.TOPIC_DESC_DTYPE)[0]
        t["n_partitions"], t["cur_width"], t["out_width"], t["rf"] = P, w, w, w
        t["cur_off"], t["out_off"] = sum(x.size for x in cur), sum(x.size for x in out)
        t["cur_len_off"] = sum(x.size for x in aux); aux.append(clen)
        t["in_partitions_off"] = -1
        t["part_id_off"] = -1
        if part_ids:
            t["part_id_off"] = sum(x.size for x in aux); aux.append(np.cumsum(rng.integers(1, 4, P)) + 5)
        cur.append(Cc.reshape(-1)); out.append(O.reshape(-1)); topics.append(t)
        status.append(abi.KAS_OK if ok else abi.KAS_FAIL_UNASSIGNABLE)

    def batch(self, scen):
        """(fb, the tables a solve would have left) over scenario descriptors `scen`"""
        fb = FlatBatch(scen=scen, topics=np.array(self.topics, dtype=abi.TOPIC_DESC_DTYPE), node_id=np.arange(50, dtype=np.int32),
                       node_rack=np.zeros(50, np.int32), cur=np.concatenate(self.cur).astype(np.int32),
                       aux=np.concatenate(self.aux).astype(np.int32), ctx=np.zeros(0, np.int32), out_len=sum(x.size for x in self.out))
        tr = np.zeros(len(self.topics), abi.TOPIC_RESULT_DTYPE)
        tr["status"] = self.status
        return fb, SimpleNamespace(out=np.concatenate(self.out).astype(np.int32), topic_results=tr)


def synthetic(w, seed=0):
    """Scenario 0: one topic per row count around the wavefront, the workgroup and the item, rows of every kind mixed, alternately
    with a part_id array with gaps.  Scenario 1: a topic whose every row is a move, one with none, a failed topic between two OK
    ones, a topic of reordered rows only, one whose out is all pad, one without rows.  Scenario 2: no topics.  Scenario 3: one
    small topic."""
    I = ITEM()
    tb = _Tables(w, np.random.default_rng([seed, w]))
    topic, topics = tb.topic, tb.topics
    scen = np.zeros(4, abi.SCENARIO_DESC_DTYPE)
    sizes = [1, 63, 64, 65, 255, 256, 257, I - 1, I, I + 1, 2 * I + 1]
    for i, P in enumerate(sizes):
        topic(P, "mixed", part_ids=i % 2 == 1)
    scen[0] = (50, 0, len(sizes), 0, 0, -1)
    first = len(topics)
    topic(70, "all"); topic(130, "none", part_ids=True); topic(90, "mixed", ok=False); topic(66, "order"); topic(40, "allpad"); topic(0, "mixed")
    topic(200, "mixed")
    scen[1] = (50, first, len(topics) - first, 0, 0, -1)
    scen[2] = (50, len(topics), 0, 0, 0, -1)
    topic(300, "mixed", part_ids=True)
    scen[3] = (50, len(topics) - 1, 1, 0, 0, -1)
    return tb.batch(scen)


_SYN = {}


def syn(w):
    if w not in _SYN:
        _SYN[w] = synthetic(w)
    return _SYN[w]


def syn16(w):
    """the same tables as 16-bit cells (ids below 0xFFFF as they are, -1 -> KAS_CELL16_NONE)"""
    fb, ho = syn(w)
    c16 = lambda a: np.where(a < 0, abi.KAS_CELL16_NONE, a).astype(np.uint16)
    return fb, c16(fb.cur), SimpleNamespace(out=c16(ho.out), topic_results=ho.topic_results)


@pytest.mark.parametrize("w", [1, 3, 5, 8])
def test_emulated_moves_of_synthetic_tables(w):
    fb, ho = syn(w)
    everything = list(range(fb.n_scenarios))
    for mask in (7, 1) if w != 3 else MASKS:
        want, got = check(fb, fb.cur, ho, everything, mask, 0, f"w {w} mask {mask}")
        if w > 1:
            assert want.n_moves[0] >= 100 and want.n_rest[0] >= 100
        assert want.n_moves[2] == 0 and want.move_off[2] == want.move_off[3]        # the scenario without topics
    # rows whose out is all pad are never moves, a failed topic contributes nothing, every row of "all" is a move, none of "none"
    rows1 = {k: flags for k, flags, *_ in scenario_rows(fb, ho, 1)}
    assert sorted(rows1) == [0, 1, 3, 4, 5, 6] and (rows1[0] & 1).all() and not rows1[1].any() and not rows1[4].any()
    if w > 1:
        assert ((rows1[3] & ORDER) != 0).all() and not (rows1[3] & REPLICAS).any()      # (rolled lists: the leader moves too)
    want, got = check(fb, fb.cur, ho, [1], 7, 0, f"w {w} scenario 1")
    assert set(np.unique(got.moves["topic"])) <= {0, 3, 6} and (got.moves["topic"] == 0).sum() == 70
    # a part_id array with gaps: the records carry its ids
    want, got = check(fb, fb.cur, ho, [3], 7, 0, f"w {w} scenario 3")
    po = int(fb.topics["part_id_off"][-1])
    assert po >= 0 and set(got.moves["partition"]) <= set(fb.aux[po:po + 300].tolist()) and got.moves["partition"].max() > 300
    # 16-bit cells
    fb, cur16, ho16 = syn16(w)
    check(fb, cur16, ho16, everything, 7, 1, f"w {w} cells16")


@pytest.mark.parametrize("select", [[], [0, 1, 2, 3], [3, 2, 1, 0], [-1, 1, -1, -1, 3, -1], [3, 3, 1, 3], [-1], [2], [1, 0, 1]],
                         ids=["empty", "all", "reversed", "empty_slots", "repeated", "one_empty_slot", "no_topics", "repeated_2"])
def test_select_lists(select):
    fb, ho = syn(3)
    want, got = check(fb, fb.cur, ho, select, 7, 0, f"select {select}")
    for j, s in enumerate(select):
        if s < 0:
            assert want.move_off[j] == want.move_off[j + 1] and want.cell_off[j] == want.cell_off[j + 1]
    if select == [3, 3, 1, 3]:                                     # each listing gets a block of its own, with equal contents
        a, b = got.moves[int(got.move_off[0]):int(got.move_off[1])], got.moves[int(got.move_off[3]):int(got.move_off[4])]
        assert a.size > 0 and np.array_equal(a, b)


def test_capacities_offsets_stay_complete_and_nothing_else_is_written():
    fb, ho = syn(3)
    select = [1, 0, 3]
    for mode, (f, cur, h) in ((0, (fb, fb.cur, ho)), (1, syn16(3))):
        want = moves_ref(f, h, select, 7, cells16=mode == 1, cur16=cur if mode == 1 else None)
        M, Cc = int(want.move_off[-1]), int(want.cell_off[-1])
        assert M > 1000 and Cc > M
        for mc, cc in [(0, 0), (0, Cc), (M, 0), (M - 1, Cc), (M, Cc - 1), (M, Cc), (M + 1, Cc + 1), (M // 2, Cc), (M, Cc // 2), (M - 1, Cc - 1)]:
            got = emu_moves(f, cur, h.out, h.topic_results, select, 7, want, mode=mode, moves_cap=mc, cells_cap=cc, what=f"caps {mc} {cc}")
            n, used = written_prefix(want, mc, cc)
            assert got.moves.size == n and got.cells.size == used
            if (mc, cc) == (M, Cc - 1):
                assert n == M - 1
            if (mc, cc) in ((M, Cc), (M + 1, Cc + 1)):
                assert n == M and used == Cc


@pytest.mark.parametrize("fill", [0, 0xFFFFFFFF, 0x00000001, 0xCDCDCDCD])
def test_same_bytes_run_after_run_whatever_the_lds_holds(fill):
    fb, ho = syn(5)
    want = moves_ref(fb, ho, [0, 1, 3], 7)
    a = emu_moves(fb, fb.cur, ho.out, ho.topic_results, [0, 1, 3], 7, want, lds_fill=fill)
    b = emu_moves(fb, fb.cur, ho.out, ho.topic_results, [0, 1, 3], 7, want, lds_fill=fill ^ 0x5A5A5A5A)
    for x, y in ((a.moves, b.moves), (a.cells, b.cells), (a.move_off, b.move_off), (a.cell_off, b.cell_off)):
        assert x.tobytes() == y.tobytes()
    f2, h2, _ = solved("mixed42")
    want = moves_ref(f2, h2, range(f2.n_scenarios), 3)
    a = emu_moves(f2, f2.cur, h2.out, h2.topic_results, list(range(f2.n_scenarios)), 3, want, lds_fill=fill)
    b = emu_moves(f2, f2.cur, h2.out, h2.topic_results, list(range(f2.n_scenarios)), 3, want, lds_fill=fill)
    assert a.moves.tobytes() == b.moves.tobytes() and a.cells.tobytes() == b.cells.tobytes()


# ---- the scan across its tiles --------------------------------------------------------------------------------------------
# scan_all walks the n x stride table of (listed scenario, item) entries in tiles of SCAN_TILE and carries the totals from tile to
# tile.  Every list below is checked by assert_spans_tiles first: more than one tile, and moves on both sides of every tile
# boundary, so that a carry lost or doubled there shows in move_off and in where the records lie.
def check_long(fb, cur, ho, select, mask, mode, what, spans=True, **kw):
    """check() for a long list with repeats (moves_ref_long), behind the guard"""
    c16 = cur if mode == 1 else None
    want = moves_ref_long(fb, ho, select, mask, cells16=mode == 1, cur16=c16)
    if spans:
        assert_spans_tiles(fb, ho, select, mask, want, cells16=mode == 1, cur16=c16, what=what)
    return want, emu_moves(fb, cur, ho.out, ho.topic_results, select, mask, want, mode=mode, what=what, **kw)


def test_the_guard_knows_the_kernels_sizes_and_the_long_checker_the_short_one():
    src = open(os.path.join(CSRC, "kas_moves.h")).read()
    assert int(re.search(r"#define KAS_MOVES_BLOCK (\d+)", src).group(1)) == SCAN_TILE and ITEM() == ITEM_ROWS
    fb, ho = syn(3)
    select = [3, 3, -1, 1, 0, 2, 3, 1]
    a, b = moves_ref(fb, ho, select, 7), moves_ref_long(fb, ho, select, 7)
    for f in ("move_off", "cell_off", "moves", "cells", "n_moves", "n_rest"):
        assert getattr(a, f).dtype == getattr(b, f).dtype and getattr(a, f).tobytes() == getattr(b, f).tobytes(), f
    with pytest.raises(AssertionError):                            # 8 x 14 entries: one tile
        assert_spans_tiles(fb, ho, select, 7, a)
    with pytest.raises(AssertionError):                            # nothing moves behind the first boundary
        assert_spans_tiles(fb, ho, [0] * 10 + [2] * 20, 7, moves_ref_long(fb, ho, [0] * 10 + [2] * 20, 7))
    assert assert_spans_tiles(fb, ho, [0] * 19, 7, moves_ref_long(fb, ho, [0] * 19, 7)) == 1


_ONE = {}


def one_item_scenarios(w=3):
    """Stride 1: scenarios of one topic of at most an item's rows.  0: mixed rows; 1: a full item of mixed rows under part ids with
    gaps; 2: no topics; 3: its only topic failed; 4: every row a move; 5: reordered rows only."""
    if w not in _ONE:
        tb = _Tables(w, np.random.default_rng([7, w]))
        scen = np.zeros(6, abi.SCENARIO_DESC_DTYPE)
        tb.topic(300, "mixed"); scen[0] = (50, 0, 1, 0, 0, -1)
        tb.topic(ITEM(), "mixed", part_ids=True); scen[1] = (50, 1, 1, 0, 0, -1)
        scen[2] = (50, 2, 0, 0, 0, -1)
        tb.topic(100, "mixed", ok=False); scen[3] = (50, 2, 1, 0, 0, -1)
        tb.topic(70, "all"); scen[4] = (50, 3, 1, 0, 0, -1)
        tb.topic(65, "order"); scen[5] = (50, 4, 1, 0, 0, -1)
        _ONE[w] = tb.batch(scen)
    return _ONE[w]


EDGE_ENTRIES = (255, 256, 511, 512)      # a tile's last lane and the next tile's first, of the first two boundaries


@pytest.mark.parametrize("n", [255, 256, 257, 511, 512, 513, 769])
def test_scan_tile_edges_exactly(n):
    """stride 1, so entry e is listed scenario e: lists that end one short of a tile, on it and one behind it; an empty slot, the
    scenario without topics, the failed one and a scenario with moves on each of the edge entries in turn"""
    fb, ho = one_item_scenarios()
    base = [(0, 4, 1, 5, 4, 0, 1)[j % 7] for j in range(n)]                   # every one of them has moves under mask 7
    kinds = (-1, 2, 3, None)
    edges = [e for e in EDGE_ENTRIES if e < n]
    for turn in range(4 if edges else 1):
        select = list(base)
        for q, e in enumerate(EDGE_ENTRIES):
            if e < n and kinds[(q + turn) % 4] is not None:
                select[e] = kinds[(q + turn) % 4]
        # the guard cannot hold where the list ends on a tile's first entry and that entry is the empty one: nothing moves behind the
        # boundary.  The entry's own move_off is then the carry (an empty slot's offsets are written too), and must not be 0.
        alone = (n - 1) % SCAN_TILE == 0 and select[n - 1] in (-1, 2, 3)
        for mask in (1, 7) if (n, turn) == (513, 0) else (7,):
            want, _ = check_long(fb, fb.cur, ho, select, mask, 0, f"{n} entries, turn {turn}, mask {mask}", spans=n > SCAN_TILE and not alone)
            if n <= SCAN_TILE or alone:
                assert want.move_off[n - 1] > 0                                 # (one tile, full or one short of it: the edge itself)
        for q, e in enumerate(EDGE_ENTRIES):
            if e < n:
                assert (want.move_off[e + 1] > want.move_off[e]) == (kinds[(q + turn) % 4] is None), (n, turn, e)


LIST_19 = [1, 3, 0, -1, 0, 2, 0, 0, 1, 3, 0, 0, -1, 0, 1, 0, 3, 0, 0]           # x stride 14 = 266 entries
LIST_300 = [(3, 0, -1, 0, 1)[j % 5] for j in range(300)]                        # x stride 14 = 4200 entries, 16 boundaries


def _boundaries_inside(fb, select, s):
    """tile boundaries that fall between two items of a listing of scenario s"""
    items = scenario_items(fb)
    stride = int(items.max())
    return [b for b in range(SCAN_TILE, len(select) * stride, SCAN_TILE) if select[b // stride] == s and 1 <= b % stride < items[s]]


@pytest.mark.parametrize("form", ["w3", "w8", "w3_cells16"])
def test_scan_tile_edge_inside_one_scenarios_items(form):
    """stride 14: scenario 0 has fourteen items, and the lists put it across tile boundaries — the carry arrives in the middle of
    its block of records"""
    w = int(form[1])
    mode = 1 if form.endswith("cells16") else 0
    fb, cur, ho = syn16(w) if mode else (syn(w)[0], syn(w)[0].cur, syn(w)[1])
    assert _boundaries_inside(fb, LIST_19, 0) == [256] and len(_boundaries_inside(fb, LIST_300, 0)) >= 5
    assert len(_boundaries_inside(fb, LIST_300, 1)) >= 1 and any(LIST_300[b // 14] == -1 for b in range(256, 4200, 256))
    for select in (LIST_19, LIST_300):
        for mask in (7, 1):
            want, got = check_long(fb, cur, ho, select, mask, mode, f"{form}, {len(select)} entries, mask {mask}")
            assert want.move_off[-1] > 1000 * len(select) // 5


def test_scan_tile_of_full_items():
    """one scenario of one topic of 1024 rows, lists 8 wide, every row a move, listed 257 times: every entry of the first tile
    holds 1024 moves and 8192 cells, the most a tile's int32 sums have to take"""
    tb = _Tables(8, np.random.default_rng(8))
    tb.topic(ITEM(), "all")
    scen = np.zeros(1, abi.SCENARIO_DESC_DTYPE)
    scen[0] = (50, 0, 1, 0, 0, -1)
    fb, ho = tb.batch(scen)
    select = [0] * (SCAN_TILE + 1)
    for mask in (7, 1):
        want, got = check_long(fb, fb.cur, ho, select, mask, 0, f"full items, mask {mask}")
        assert (np.diff(want.move_off) == ITEM()).all() and (np.diff(want.cell_off) == 8 * ITEM()).all()
        assert got.move_off[SCAN_TILE] == SCAN_TILE * ITEM() and got.cell_off[SCAN_TILE] == SCAN_TILE * ITEM() * 8


def test_capacities_that_cut_in_a_later_tile():
    fb, ho = syn(3)
    select = LIST_300
    want = moves_ref_long(fb, ho, select, 7)
    assert_spans_tiles(fb, ho, select, 7, want)
    M, Cc = int(want.move_off[-1]), int(want.cell_off[-1])
    first_tile = int(want.move_off[-(-SCAN_TILE // 14)])                       # moves of the listings that reach into the first tile
    for mc, cc in ((M // 2, Cc), (M, Cc // 3), (M - 1, Cc - 1)):
        got = emu_moves(fb, fb.cur, ho.out, ho.topic_results, select, 7, want, moves_cap=mc, cells_cap=cc, what=f"caps {mc} {cc}")
        n, used = written_prefix(want, mc, cc)
        assert got.moves.size == n and got.cells.size == used and first_tile < n < M, (mc, cc, n, first_tile)


def test_same_bytes_across_tiles_whatever_the_lds_holds():
    fb, ho = syn(3)
    runs = [check_long(fb, fb.cur, ho, LIST_19, 7, 0, f"lds {fill:#x}", lds_fill=fill)[1] for fill in (0, 0xFFFFFFFF)]
    for f in ("moves", "cells", "move_off", "cell_off"):
        assert getattr(runs[0], f).tobytes() == getattr(runs[1], f).tobytes(), f


def test_refusals_of_the_arguments():
    fb, ho = syn(3)
    ok = lambda **kw: emu_moves_raw(fb, fb.cur, ho.out, ho.topic_results, [0], kw.pop("mask", 7), moves_cap=4, cells_cap=16, **kw)
    for mask in (0, 8, -1):
        rc, err, _ = ok(mask=mask)
        assert rc == E_INVALID and "mask outside 1..7" in err
    L = _emu_lib()
    bd = batch_desc(fb)
    t = abi.Tables()
    t.cur, t.out, t.aux, t.topic_results = fb.cur.ctypes.data, ho.out.ctypes.data, fb.aux.ctypes.data, ho.topic_results.ctypes.data
    buf = np.zeros(64, np.int64)
    base = buf.ctypes.data
    sel = np.zeros(1, np.int32)
    cases = [(abi.Moves(7, 0, None, base, base, 1, base, 1), "is NULL"), (abi.Moves(7, 0, base, None, base, 1, base, 1), "is NULL"),
             (abi.Moves(7, 0, base, base, None, 1, base, 1), "is NULL"), (abi.Moves(7, 0, base, base, base, 1, None, 1), "is NULL"),
             (abi.Moves(7, 0, base, base, base, -1, base, 1), "negative capacity"),
             (abi.Moves(7, 0, base + 4, base, base, 1, base, 1), "aligned"), (abi.Moves(7, 0, base, base, base + 2, 1, base, 1), "aligned"),
             (abi.Moves(7, 0, base, base, base, 1, base + 2, 1), "aligned"),
             (abi.Moves(9, 0, None, None, None, -1, None, 1), "mask outside")]          # the order: the mask first
    for mv, text in cases:
        err = C.create_string_buffer(256)
        rc = L.kas_emu_moves(C.byref(bd), C.byref(t), 0, sel.ctypes.data, 1, C.byref(mv), 0, err, 256)
        assert rc == E_INVALID and text in err.value.decode(), (rc, err.value.decode(), text)
    # NULL arrays are fine where the capacity is 0
    rc, err, got = emu_moves_raw(fb, fb.cur, ho.out, ho.topic_results, [0, 1], 7)
    assert rc == 0 and got.move_off[2] > 0, err
    # a scenario of 2^31 packed cells
    big = dataclasses.replace(fb, topics=fb.topics.copy())
    big.topics["n_partitions"][0] = 2**28 + 1
    big.topics["out_width"][0] = 8
    mv = abi.Moves(7, 0, base, base, base, 1, base, 1)
    err = C.create_string_buffer(256)
    bd = batch_desc(big)
    rc = L.kas_emu_moves(C.byref(bd), C.byref(t), 0, sel.ctypes.data, 1, C.byref(mv), 0, err, 256)
    assert rc == E_UNSUPPORTED and "2^31" in err.value.decode()


def test_room_helpers():
    fb, _ = syn(3)
    L = _emu_lib()
    bd = batch_desc(fb)
    rows = [int(np.clip(fb.topics["n_partitions"][int(b):int(b) + int(c)], 0, None).sum()) for b, c in zip(fb.scen["topic_begin"], fb.scen["topic_count"])]
    cells = native.packed_cells(fb)
    out = (C.c_int64 * 5)()
    for select in ([0, 1], [3, 3, -1, 2], []):
        sel = np.asarray(select + [0], np.int32)                                # (never NULL: that means every scenario)
        L.kas_emu_moves_room(C.byref(bd), sel.ctypes.data, len(select), 2, out)
        live = [s for s in select if s >= 0]
        assert (out[0], out[1]) == (sum(rows[s] for s in live), sum(int(cells[s]) for s in live)) == native.moves_room(fb, select)
    L.kas_emu_moves_room(C.byref(bd), None, 0, 2, out)                        # select == NULL: every scenario
    assert (out[0], out[1]) == (sum(rows), int(cells.sum()))
    assert (out[2], out[3]) == (sum(sorted(rows)[-2:]), int(np.sort(cells)[-2:].sum()))
    I = ITEM()
    assert out[4] == max(sum(-(-int(p) // I) for p in fb.topics["n_partitions"][int(b):int(b) + int(c)])
                         for b, c in zip(fb.scen["topic_begin"], fb.scen["topic_count"]))


# ---- the planner ----------------------------------------------------------------------------------------------------------
HOST_BUFS = ("cur", "out", "aux", "ctx", "cur16", "out16", "tr", "sr", "tr_pin", "sr_pin", "imp_nodes", "imp_scen",
             "ch_sizes", "ch_segs", "ch_head", "ch_rows", "ch_nodes", "ch_head_pin", "ch_rows_pin", "ch_nodes_pin",
             "mv_scen", "mv_segs", "mv_select", "mv_scratch", "mv_head", "mv_moves", "mv_cells", "mv_sizes0", "mv_head_pin")
HEAD = ("listed", "room_moves", "room_cells", "moves_cap", "cells_cap", "K", "stride", "gather_rows", "rows_need", "scenarios", "segments", "native16")
_BUF = np.zeros(16, np.int64)


def moves_host_call(fb, mv=None, select=None, spec=None, rows_cap=0, nodes_cap=None, missing=0, cells16=False, ranges_override=0):
    L = _emu_lib()
    assert L.kas_emu_moves_buffers() == len(HOST_BUFS)
    bd = batch_desc(fb)
    if cells16:
        bd.node_id = None
    b = _BUF.ctypes.data
    mv = abi.Moves(7, 0, b, b, b, 10**6, b, 10**7) if mv is None else mv
    sel = None if select is None else np.ascontiguousarray(select, np.int32)
    if nodes_cap is None:
        nodes_cap = int(np.sort(np.clip(fb.scen["n_nodes"], 0, None))[::-1][:spec.k if spec else 0].sum())
    lens = (C.c_int64 * 5)(int(fb.cur.shape[0]), int(fb.aux.shape[0]), int(fb.ctx.shape[0]), rows_cap, nodes_cap)
    head, nbytes = (C.c_int64 * len(HEAD))(), (C.c_int64 * len(HOST_BUFS))()
    err = C.create_string_buffer(512)
    rc = L.kas_emu_moves_host_call(C.byref(bd), lens, missing, int(cells16), None if spec is None else C.byref(spec),
                                   None if sel is None or not sel.size else sel.ctypes.data, -1 if sel is None else int(sel.size), C.byref(mv),
                                   ranges_override, head, nbytes, err, 512)
    if rc != 0:
        return rc, None, err.value.decode()
    plan = dict(zip(HEAD, [int(v) for v in head]))
    plan["bytes"] = dict(zip(HOST_BUFS, [int(v) for v in nbytes]))
    return rc, plan, ""


def _choose_spec(k, keys=("moved_replicas",)):
    return abi.choose_spec(keys, k)


def test_planner_refuses_in_order_each_with_its_text():
    fb, _, _ = solved("mixed42")
    S = fb.n_scenarios
    b = _BUF.ctypes.data
    M = lambda *a: abi.Moves(*a)
    # what the host call refuses anyway comes first, then the mask, the capacities, the arrays, the alignment, the list
    order = [(dict(mv=M(9, 0, None, b, b + 2, -1, b, 1), select=[S], missing=16), "is NULL"),
             (dict(mv=M(9, 0, None, b, b + 2, -1, b, 1), select=[S]), "mask outside 1..7"),
             (dict(mv=M(7, 0, None, b, b + 2, -1, b, 1), select=[S]), "negative capacity"),
             (dict(mv=M(7, 0, None, b, b + 2, 1, b, 1), select=[S]), "an array the call writes is NULL"),
             (dict(mv=M(7, 0, b, b, b + 2, 1, b, 1), select=[S]), "aligned"),
             (dict(mv=M(7, 0, b, b, b, 1, b, 1), select=[S]), "scenario index out of range"),
             (dict(mv=M(7, 0, b, b, b, 1, b, 1), select=[-2]), "scenario index out of range")]
    for kw, text in order:
        rc, _, err = moves_host_call(fb, **kw)
        assert rc == E_INVALID and text in err, (kw, rc, err)
    # a choice: its own refusals come before the moves'
    rc, _, err = moves_host_call(fb, mv=M(9, 0, b, b, b, 1, b, 1), spec=_choose_spec(S + 1))
    assert rc == E_INVALID and "k outside" in err
    rc, _, err = moves_host_call(fb, mv=M(9, 0, b, b, b, 1, b, 1), spec=_choose_spec(2), missing=8192)
    assert rc == E_INVALID and "mask outside" in err
    # rows: NULL with rows_cap == 0 is the form without rows; NULL with a capacity, or room below the k largest, is refused as before
    rows2 = int(np.sort(native.packed_cells(fb))[::-1][:2].sum())
    rc, plan, err = moves_host_call(fb, spec=_choose_spec(2), rows_cap=0, missing=8192)
    assert rc == 0 and plan["gather_rows"] == 0 and plan["rows_need"] == 0, err
    rc, plan, err = moves_host_call(fb, spec=_choose_spec(2), rows_cap=rows2)
    assert rc == 0 and plan["gather_rows"] == 1 and plan["rows_need"] == rows2, err
    assert moves_host_call(fb, spec=_choose_spec(2), rows_cap=rows2 - 1)[0] == E_INVALID
    assert moves_host_call(fb, spec=_choose_spec(2), rows_cap=rows2, missing=8192)[0] == E_INVALID
    assert moves_host_call(fb, spec=_choose_spec(2), rows_cap=0)[0] == E_INVALID       # an array with no room: below the k largest


@pytest.mark.parametrize("cells16", [False, True], ids=["int32", "cells16"])
def test_planner_buffer_sizes(cells16):
    fb, _, _ = solved("mixed42")
    S, T = fb.n_scenarios, fb.n_topics
    cell = 2 if cells16 else 4
    b = _BUF.ctypes.data
    select = [2, -1, 0, 2]
    room = native.moves_room(fb, select)
    rc, plan, err = moves_host_call(fb, mv=abi.Moves(1, 0, b, b, b, 10**9, b, 10**9), select=select, cells16=cells16)
    assert rc == 0, err
    assert (plan["listed"], plan["room_moves"], plan["room_cells"]) == (4,) + room
    assert (plan["moves_cap"], plan["cells_cap"]) == room and plan["scenarios"] == S and plan["segments"] == T     # no more than the room
    by = plan["bytes"]
    assert by["mv_scen"] == 32 * (S + 1) and by["mv_segs"] == 56 * (T + 1) and by["mv_select"] == 4 * 5
    assert by["mv_scratch"] == 16 * (4 * plan["stride"] + 1) and by["mv_head"] == by["mv_head_pin"] == 16 * 5
    assert by["mv_moves"] == 16 * (room[0] + 1) and by["mv_cells"] == cell * (room[1] + 8) and by["mv_sizes0"] == 0
    assert all(by[n] == 0 for n in HOST_BUFS[10:20]), "a moves call reserves no impact or choice buffer"
    # capacities below the room are the device's capacities; n_select < 0 lists every scenario
    rc, plan, err = moves_host_call(fb, mv=abi.Moves(1, 0, b, b, b, 7, b, 9), select=None, cells16=cells16)
    assert rc == 0 and (plan["listed"], plan["moves_cap"], plan["cells_cap"]) == (S, 7, 9), err
    assert (plan["room_moves"], plan["room_cells"]) == native.moves_room(fb, range(S))
    # a choice: the room of the k largest, the list is the choice's own (no list buffer), the size table without cells only without rows
    rc, plan, err = moves_host_call(fb, spec=_choose_spec(3), rows_cap=0, missing=8192, cells16=cells16)
    rows = sorted(native.moves_room(fb, [s])[0] for s in range(S))[-3:]
    assert rc == 0 and plan["listed"] == 3 and plan["room_moves"] == sum(rows) and plan["room_cells"] == int(np.sort(native.packed_cells(fb))[-3:].sum()), err
    assert plan["bytes"]["mv_select"] == 0 and plan["bytes"]["mv_sizes0"] == 32 * (S + 1) and plan["bytes"]["ch_rows"] == cell * 8
    # the plans of the other calls are what they were: no moves buffer, everything else equal
    import emu_lib
    import test_choose_cpu as tc
    rc, other, _ = emu_lib.host_call(fb, select=[], cells16=cells16)
    rc2, mine, _ = moves_host_call(fb, select=[], cells16=cells16)
    assert rc == 0 and rc2 == 0 and {n: mine["bytes"][n] for n in HOST_BUFS[:12]} == other["bytes"] and mine["K"] == other["K"]
    rc, theirs, _ = tc.choose_host_call(fb, tc._spec(("moved_replicas",), 3), cells16=cells16)
    rc2, mine, _ = moves_host_call(fb, spec=_choose_spec(3), rows_cap=theirs["rows_need"], cells16=cells16)
    assert rc == 0 and rc2 == 0 and {n: mine["bytes"][n] for n in HOST_BUFS[:20]} == theirs["bytes"] and mine["K"] == theirs["K"]


def test_planner_scenario_ranges_of_a_moves_call():
    """S x 100k x 3 cells with a `cur` per scenario (descriptors only): a moves call uploads cur and downloads no out table, as a
    choice does.  The counts tests/test_moves_gpu.py relies on when it asks for a call cut into ranges: 52.8 MB (44 scenarios of
    int32 cells, 88 of 16-bit cells) are two ranges, 26.4 MB (44 of 16-bit cells, below KAS_HOST_SPLIT_MIN_BYTES) one, and the
    KAS_HOST_RANGES override the library passes in decides otherwise"""
    from kafka_assigner_amd import generator as G
    from kafka_assigner_amd.flatten import node_set_batch
    P, N, R = 100_000, 200, 10
    sets = [G.scenario_action(61, s, N, R, actions=G.BENCH_ACTIONS)[1] for s in range(44)]

    def shape(S):
        return node_set_batch([sets[s % 44].node_id for s in range(S)], [sets[s % 44].node_rack for s in range(S)], P, 3, 3,
                              cur=np.zeros((S, P, 3), np.int32))
    fb44, fb88 = shape(44), shape(88)
    select = [43, -1, 0, 22, 21, 43]
    K = lambda fb, **kw: (lambda rc, plan, err: plan["K"] if rc == 0 else (rc, err))(*moves_host_call(fb, **kw))
    assert K(fb44, select=select) == 2 and K(fb44) == 2
    spec = _choose_spec(3, ("max_outbound", "moved_replicas"))
    assert K(fb44, spec=spec, rows_cap=9 * P) == 2 and K(fb44, spec=spec, rows_cap=0, missing=8192) == 2
    assert K(fb88, select=select + [87, 44], cells16=True) == 2
    assert K(fb44, select=select, cells16=True) == 1
    assert K(fb44, select=select, ranges_override=3) == 3
    rc, plan, err = moves_host_call(fb44, select=select)
    assert plan["stride"] == -(-P // ITEM()) == 98 and plan["listed"] * plan["stride"] > 2 * SCAN_TILE   # the list spans three tiles


# ---- ABI ------------------------------------------------------------------------------------------------------------------
def test_abi_declares_the_moves_entries_and_layouts(tmp_path):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(kas_[a-z_0-9]+)\s*\(", src))
    assert len(abi.MOVES_ENTRIES) == 6
    for name in abi.MOVES_ENTRIES:
        assert name in declared and name in native.SYMBOLS, name
    assert re.search(r"#define KAS_ABI_VERSION (\d+)", src).group(1) == str(abi.KAS_ABI_VERSION) == "6"
    mf = ["topic", "partition", "flags", "len", "gained", "lost", "cell_at"]
    sf = ["mask", "reserved", "move_off", "cell_off", "moves", "moves_cap", "cells", "cells_cap"]
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kas_abi.h"\nint main(void) {\n'
                     '  printf("%zu %zu %d %d %d\\n", sizeof(kas_move), sizeof(kas_moves), KAS_MOVE_REPLICAS, KAS_MOVE_LEADER, KAS_MOVE_ORDER);\n'
                     + "".join('  printf("%%zu\\n", offsetof(kas_move, %s));\n' % f for f in mf)
                     + "".join('  printf("%%zu\\n", offsetof(kas_moves, %s));\n' % f for f in sf) + '  return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c11", "-I" + os.path.join(ROOT, "include"), str(probe), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)], text=True).splitlines()
    assert lines[0].split() == [str(C.sizeof(abi.Move)), str(C.sizeof(abi.Moves)), "1", "2", "4"] and C.sizeof(abi.Move) == 16
    assert [int(v) for v in lines[1:8]] == [getattr(abi.Move, f).offset for f in mf] == [abi.MOVE_DTYPE.fields[f][1] for f in mf]
    assert [int(v) for v in lines[8:16]] == [getattr(abi.Moves, f).offset for f in sf]
    assert (abi.KAS_MOVE_REPLICAS, abi.KAS_MOVE_LEADER, abi.KAS_MOVE_ORDER) == (1, 2, 4)
    assert abi.move_mask(("replicas", "order")) == 5 and abi.move_mask("leader") == 2 and abi.move_mask(7) == 7
    with pytest.raises(ValueError):
        abi.move_mask(("replicas", "sideways"))


def test_library_exports_the_moves_entries():
    from kafka_assigner_amd import build
    build.build()
    L = native.load()
    for name in abi.MOVES_ENTRIES:
        assert hasattr(L, name), name
    assert L.kas_abi_version() == 6
    blob = open(build.LIB, "rb").read()
    assert b"kas_moves_count_kernel" in blob and b"kas_moves_scan_kernel" in blob and b"kas_moves_emit_kernel" in blob
    assert "kas_moves.hip" in build.SOURCES


# ---- WhatIf: the library's host calls replaced by the oracle and the checker ---------------------------------------------
def _fake_native(monkeypatch):
    def trimmed(ml):
        return native.MoveList(mask=ml.mask, select=ml.select, move_off=ml.move_off, cell_off=ml.cell_off, moves=ml.moves, cells=ml.cells)

    def solve_host_moves(fb, mask=("replicas",), select=None, **kw):
        ho = oracle_solve(fb)
        sel = list(range(fb.n_scenarios)) if select is None else list(select)
        w = moves_ref(fb, ho, sel, abi.move_mask(mask))
        ho_norows = dataclasses.replace(ho, out=ho.out[:0])
        return ho_norows, trimmed(SimpleNamespace(mask=abi.move_mask(mask), select=np.asarray(sel, np.int32), move_off=w.move_off, cell_off=w.cell_off,
                                                  moves=w.moves, cells=w.cells))

    def solve_host_choose_moves(fb, keys, k, mask=("replicas",), rows=True, **kw):
        from choose_ref import choose_ref
        from impact_ref import impact_ref
        ho = oracle_solve(fb)
        imp = impact_ref(fb, ho)
        c = choose_ref(fb, ho.scenario_results, ho.out, imp, keys, k)
        w = moves_ref(fb, ho, c.chosen, abi.move_mask(mask))
        ch = native.Choice(rank=c.rank, chosen=c.chosen, row_off=c.row_off, node_off=c.node_off, n_ok=c.n_ok,
                           rows=c.rows if rows else c.rows[:0], nodes=c.nodes, scenarios=imp[1])
        return dataclasses.replace(ho, out=ho.out[:0]), ch, trimmed(SimpleNamespace(mask=abi.move_mask(mask), select=c.chosen, move_off=w.move_off,
                                                                                    cell_off=w.cell_off, moves=w.moves, cells=w.cells))
    monkeypatch.setattr(native, "solve_host_moves", solve_host_moves)
    monkeypatch.setattr(native, "solve_host_choose_moves", solve_host_choose_moves)


def _small_whatif():
    from kafka_assigner_amd.whatif import Variant, WhatIf
    brokers, topics = whatif_inputs()
    topics = {n: {p: r for p, r in t.items() if p < 400} for n, t in topics.items()}
    return WhatIf(brokers, topics), [Variant(label="as is"), Variant(remove=[5], label="-5"), Variant(remove=[7, 11], add={60: "r0"}, label="swap")], topics


def apply_moves(current, moves):
    new = {t: {p: list(r) for p, r in rows.items()} for t, rows in current.items()}
    for t, p, reps, _ in moves:
        new[t][p] = list(reps)
    return new


def test_whatif_solve_and_best_with_moves(monkeypatch):
    _fake_native(monkeypatch)
    w, vs, topics = _small_whatif()
    full = w.solve(vs, solve_fn=oracle_solve)
    res = w.solve(vs, moves=("replicas", "leader", "order"))
    assert all(r.status == 0 for r in res)
    for r, f in zip(res, full):
        with pytest.raises(ValueError):
            r.assignment("orders")
        new = apply_moves(topics, r.moves())
        for t in topics:
            assert new[t] == f.assignment(t), (r.label, t)                  # all three kinds: the lists exactly
        only = r.moves(kinds=("replicas",))
        assert 0 < len(only) < len(r.moves()) or r.label == "as is"
        assert all("replicas" in kinds for *_, kinds in only)
        assert r.moves(topic="clicks") == [m for m in r.moves() if m[0] == "clicks"]
        j = r.reassignment(kinds=("replicas",))
        assert j["version"] == 1 and [(e["topic"], e["partition"], e["replicas"]) for e in j["partitions"]] == [m[:3] for m in only]
    sets = w.solve(vs, moves=("replicas",))
    for r, f in zip(sets, full):
        new = apply_moves(topics, r.moves())
        for t in topics:
            assert {p: set(v) for p, v in new[t].items()} == {p: set(v) for p, v in f.assignment(t).items()}
        assert sum(len(set(reps) - set(topics[t][p])) for t, p, reps, _ in r.moves()) == r.moved_replicas
        with pytest.raises(ValueError):
            r.moves(kinds=("order",))
    with pytest.raises(ValueError):
        w.solve(vs, moves=("replicas",), impact=True)
    with pytest.raises(ValueError):
        w.solve(vs, moves=("sideways",))
    # best: winners with their moves, with and without rows
    best = w.best(vs, k=2, moves=("replicas",), rows=False)
    with_rows = w.best(vs, k=2, moves=("replicas", "leader", "order"))
    assert [r.label for r in best] == [r.label for r in with_rows] and len(best) == 2 and best[0].rank == 0
    for r, f in zip(best, with_rows):
        with pytest.raises(ValueError):
            r.assignment("orders")
        for t in topics:
            assert apply_moves(topics, f.moves())[t] == f.assignment(t)
            assert {p: set(v) for p, v in apply_moves(topics, r.moves())[t].items()} == {p: set(v) for p, v in f.assignment(t).items()}
        assert r.broker_impact() == f.broker_impact()
    with pytest.raises(ValueError):
        w.best(vs, k=1, rows=False)
    with pytest.raises(ValueError):
        full[0].moves()

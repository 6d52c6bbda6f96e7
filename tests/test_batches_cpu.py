"""Execution batches (include/kas_abi.h: kas_batch_spec / kas_move_batch / kas_scenario_batches / kas_batches) without a GPU.

- The kernel body (kafka-assigner_amd/csrc/kas_batches_body.h) compiled with g++ against tests/emu/kas_wave.h and stepped on CPU
  fibers (tests/emu/batches_driver.cpp) against the checker (tests/batches_ref.py: the header's loop in plain Python): over
  oracle-solved batches of tests/impact_batches.py, and over crafted out tables that put moves exactly where the kernel's group of
  KAS_BATCH_GROUP moves, its tile of 1,024 rows and a topic end.
- The crafted cases of tests/crafted_cases.py, which tests/test_batches_crafted_gpu.py runs on the GPU.
- The refusals in their order, the node limit, the host call planner's bytes, the ABI, WhatIf's argument handling.
"""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import batches_ref as R
import crafted_cases as CC
from batches_ref import GROUP, ITEM_ROWS, assert_same_batches, batches_ref, check_invariants, cut, replay, scenario_moves
from impact_batches import STALE_ID, T, scenario, solved
from kafka_assigner_amd import abi, native
from kafka_assigner_amd.flatten import Scenario, Topic, batch_desc, flatten, index_form, to_cells16
from moves_ref import moves_ref
from oracle_lib import oracle_solve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "kafka-assigner_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "kas_abi.h")
E_INVALID, E_UNSUPPORTED = abi.KAS_E_INVALID_ARG, abi.KAS_E_UNSUPPORTED
FILL = 0x5A5A5A5A                                   # what the output arrays hold before a call
BIG = 10 ** 6
_LIB = None


# ---- the emulator ---------------------------------------------------------------------------------------------------------
def _emu_lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    so = os.path.join(EMU, "libkas_emu_batches.so")
    srcs = [os.path.join(EMU, f) for f in ("batches_driver.cpp", "emu_driver.cpp")]
    deps = srcs + [os.path.join(EMU, "kas_wave.h"), HEADER] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        tmp = so + ".tmp%d" % os.getpid()
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unused-parameter", "-Wno-unknown-pragmas",
                               "-I" + os.path.join(ROOT, "tests"), "-I" + CSRC, "-I" + os.path.join(ROOT, "include"),
                               "-o", tmp] + srcs)
        os.replace(tmp, so)
    L = C.CDLL(so)
    L.kas_emu_batches.restype = C.c_int
    L.kas_emu_batches.argtypes = [C.POINTER(abi.BatchDesc), C.POINTER(abi.Tables), C.c_int, C.c_void_p, C.c_int32, C.POINTER(abi.BatchSpec),
                                  C.POINTER(abi.Batches), C.c_uint32, C.POINTER(C.c_int32), C.c_char_p, C.c_int]
    L.kas_emu_batches_host_call.restype = C.c_int
    L.kas_emu_batches_host_call.argtypes = [C.POINTER(abi.BatchDesc), C.POINTER(C.c_int64), C.c_int, C.c_void_p, C.c_int32, C.c_void_p,
                                            C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_char_p, C.c_int]
    L.kas_emu_batches_const.restype = C.c_int
    L.kas_emu_batches_const.argtypes = [C.c_int]
    L.kas_emu_batches_lds.restype = None
    L.kas_emu_batches_lds.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]
    _LIB = L
    return L


def const(name):
    names = ("HB_FINAL", "HB_EVERY", "GROUP", "ITEM_ROWS", "NODE_LIMIT", "QUEUE", "BT_SDESC", "BT_NODE_ID", "BT_SELECT", "BT_SCEN", "BT_BATCHES",
             "MV_SCEN", "MV_SEGS")
    return _emu_lib().kas_emu_batches_const(names.index(name))


def emu_rc(fb, ho, select, caps, stride, cells16=False, cur16=None, lds_fill=0xCDCDCDCD, spec=None, null_batches=False, raw_out=None):
    """kas_emu_batches over the tables a solve left in `ho`: (rc, text, scenario records, batch records, info)"""
    L = _emu_lib()
    bd = batch_desc(fb)
    t = abi.Tables()
    if cells16:
        bd.node_id = None
        cur16 = to_cells16(fb) if cur16 is None else cur16
        t.cur = cur16.ctypes.data
    else:
        t.cur = fb.cur.ctypes.data
    t.out = ho.out.ctypes.data
    t.aux = fb.aux.ctypes.data if fb.aux.size else None
    t.topic_results = ho.topic_results.ctypes.data
    sel = None if select is None else np.ascontiguousarray(select, dtype=np.int32)
    n = fb.n_scenarios if sel is None else int(sel.size)
    scen = np.full(max(n, 1), FILL, np.int32).repeat(8).view(abi.SCENARIO_BATCHES_DTYPE)[:n]
    recs = np.full(max(n * max(stride, 0), 1) * 8, FILL, np.int32).view(abi.MOVE_BATCH_DTYPE)[:n * max(stride, 0)]
    o = raw_out if raw_out is not None else abi.Batches(scen.ctypes.data if n else None, None if null_batches or not recs.size else recs.ctypes.data, stride)
    sp = spec if spec is not None else abi.batch_spec(caps)
    info = (C.c_int32 * 4)()
    err = C.create_string_buffer(512)
    rc = L.kas_emu_batches(C.byref(bd), C.byref(t), int(cells16), None if sel is None else sel.ctypes.data, -1 if sel is None else n,
                           C.byref(sp), C.byref(o), lds_fill, info, err, 512)
    return rc, err.value.decode(), scen, recs, dict(lds=int(info[0]), n_cap=int(info[1]), W=int(info[2]), collectives=int(info[3]))


def emu(fb, ho, select, caps, stride, **kw):
    rc, err, scen, recs, info = emu_rc(fb, ho, select, caps, stride, **kw)
    assert rc == 0, (rc, err)
    return scen, recs, info


def solved16(fb):
    """The oracle's solve of the batch's 16-bit form: (HostOutputs with uint16 out, cur16)."""
    ho = oracle_solve(index_form(fb))
    ho.out = np.where(ho.out < 0, abi.KAS_CELL16_NONE, ho.out).astype(np.uint16)
    return ho, to_cells16(fb)


def check(fb, ho, select, caps, what, stride=None, solve_records=True, want=None, **kw):
    """One call on the emulator against the checker, with the invariants; returns the checker's list (want: that list, where the
    caller has it already)"""
    select = list(range(fb.n_scenarios)) if select is None else list(select)
    want = want or batches_ref(fb, ho, select, caps, cells16=kw.get("cells16", False), cur16=kw.get("cur16"))
    most = max([w.record["n_batches"] for w in want if w is not None] + [1])
    stride = most + 2 if stride is None else stride
    scen, recs, _ = emu(fb, ho, select, caps, stride, **kw)
    assert_same_batches(want, scen, recs, stride, fill=FILL, what=what)
    for j, s in enumerate(select):
        if want[j] is not None:
            sr = ho.scenario_results
            check_invariants(want[j], caps, sr["moved_partitions"][s] if solve_records else None, sr["moved_replicas"][s] if solve_records else None,
                             what=(what, j))
    return want


# ---- crafted tables: rows whose out lists are written by the test, so that moves lie exactly where a case wants them ------------
def crafted(topics, N=12, n_cur=None, extra_cur=0, width=3, ids=None):
    """One scenario on brokers 0..N-1.  topics: [(P, {row: out list})]: row p holds [p, p+1, p+2 mod n_cur] (n_cur <= N brokers hold
    replicas; + extra_cur: ids N.. that are not in the set, departed) and comes out as it is unless the dict names it.  Every
    topic is KAS_OK.  Returns (fb, ho).
    width: rows hold [p, p+1, ... p+width-1 mod n_cur] (a topic that is (P, {row: out list}, width) has a width of its own): lists 5
    or 8 wide put the plan in that width class.  ids: the scenario's node id table, N ids ascending: broker b is known as ids[b]
    in the set, in the rows and in the out lists (a number from N on stays outside the set: an id above the table)."""
    n_cur = n_cur or N
    if ids is None:
        known = lambda b: b
    else:
        assert len(ids) == N and all(int(a) < int(b) for a, b in zip(ids, ids[1:])), "N node ids, ascending"
        known = lambda b: b if b < 0 else (int(ids[b]) if b < N else int(ids[-1]) + 1 + b - N)
    tps = []
    for k, tp in enumerate(topics):
        P, w = tp[0], (tp[2] if len(tp) > 2 else width)
        rows = {p: [known((p + i) % n_cur if (p + i) % (n_cur + extra_cur) < n_cur else N + (p + i) % (n_cur + extra_cur) - n_cur) for i in range(w)]
                for p in range(P)}
        tps.append(Topic("c%d" % k, rows, 3))
    fb = flatten([Scenario([known(b) for b in range(N)], {known(b): "r%d" % (b % 4) for b in range(N)}, tps)])
    from kafka_assigner_amd.flatten import host_tables
    _, ho = host_tables(fb)
    ho.topic_results["status"][:] = abi.KAS_OK
    for k, tp in enumerate(topics):
        P, moved = tp[0], tp[1]
        td = fb.topics[k]
        co, oo, cw, ow = int(td["cur_off"]), int(td["out_off"]), int(td["cur_width"]), int(td["out_width"])
        out = np.full((P, ow), -1, np.int32)
        out[:, :cw] = fb.cur[co:co + P * cw].reshape(P, cw)
        for p, lst in moved.items():
            out[p, :] = -1
            out[p, :len(lst)] = [known(b) for b in lst]
        ho.out[oo:oo + P * ow] = out.reshape(-1)
    return fb, ho


def swap_in(p, node, n_cur=12, width=3):
    """out list of crafted row p that replaces its first replica by `node` (In = {node}, Out = {p mod n_cur})"""
    return [node] + [(p + i) % n_cur for i in range(1, width)]


def random_moves(P, n_moves, N, n_cur, seed, width=3, most=2):
    """{row: out list} for n_moves rows of a crafted topic of P rows (`width` replicas a row): one or two (one to `most`) replicas
    replaced by brokers the row does not hold"""
    rng = np.random.default_rng([seed, 0xB7])
    moved = {}
    for p in sorted(int(x) for x in rng.choice(P, n_moves, replace=False)):
        row = [(p + i) % n_cur for i in range(width)]
        free = [b for b in range(N) if b not in row]
        new = [int(b) for b in rng.choice(free, 1 + int(rng.integers(0, min(most, len(free)))), replace=False)]
        moved[p] = new + row[len(new):]
    return moved


# ---- group, tile and topic boundaries ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_moves", [GROUP - 1, GROUP, GROUP + 1])
def test_group_boundaries(n_moves):
    """move counts around KAS_BATCH_GROUP: the clean path (no cap binds), the mixed one, and the replay of every group"""
    assert GROUP == const("GROUP") and ITEM_ROWS == const("ITEM_ROWS")
    fb, ho = crafted([(700, random_moves(700, n_moves, 12, 12, n_moves))])
    mv = scenario_moves(fb, ho, 0)
    assert len(mv) == n_moves
    for caps in ({"inbound": BIG, "outbound": BIG, "max_moves": BIG}, {"inbound": 8}, {"inbound": 1}, {"max_moves": GROUP}):
        check(fb, ho, None, caps, ("group boundary", n_moves, caps), solve_records=False)
    r = replay(mv, {"inbound": BIG, "outbound": BIG, "max_moves": BIG})
    assert r.replayed == 0 and r.clean == -(-n_moves // GROUP)


def test_tile_and_topic_boundaries():
    """rows 1,023, 1,024 and 1,025 of a topic move (both sides of a tile), a batch spans the topic's end into the next topic, and a
    row that comes out empty is no move"""
    moved = {p: swap_in(p, (p + 5) % 12) for p in (3, 1022, 1023, 1024, 1025)}
    moved[7] = []                                                            # olen == 0: no flags, never a move
    fb, ho = crafted([(1026, moved), (40, {0: swap_in(0, 7), 39: swap_in(39, 9 if 39 % 12 != 9 else 10)})])
    mv = scenario_moves(fb, ho, 0)
    assert [(t, p) for t, p, _, _ in mv] == [(0, 3), (0, 1022), (0, 1023), (0, 1024), (0, 1025), (1, 0), (1, 39)]
    want = check(fb, ho, None, {"max_moves": 4}, "tile and topic boundaries", solve_records=False)
    bt = want[0].batches
    assert [(b["first_move"], b["n_moves"], b["topic"], b["partition"]) for b in bt] == [(0, 4, 0, 3), (4, 3, 0, 1025)]   # the second spans the topic end
    check(fb, ho, None, {"inbound": 1}, "tile and topic boundaries, inbound 1", solve_records=False)
    # the moves pass's list under the REPLICAS mask is this list: a batch's (topic, partition) is its record at first_move
    ml = moves_ref(fb, ho, [0], abi.KAS_MOVE_REPLICAS)
    for b in bt:
        assert (int(ml.moves["topic"][b["first_move"]]), int(ml.moves["partition"][b["first_move"]])) == (b["topic"], b["partition"])


def test_cap_reached_by_the_last_move_of_a_group():
    """node 11 is taken by moves 100 and 255 (the group's last): cap 2 is reached and the group is clean; move 256 takes it again
    and closes.  The other moves gain a broker outside the set (ids 100..: In is empty), so node 11 is the only receiver."""
    rows = list(range(0, 600, 2))                                           # 300 moves on even rows, cur over brokers 0..10
    moved = {p: [p % 11, (p + 1) % 11, 11] if i in (100, 255, 256) else [p % 11, (p + 1) % 11, (p + 2) % 11 + 100] for i, p in enumerate(rows)}
    fb, ho = crafted([(600, moved)], N=12, n_cur=11)
    mv = scenario_moves(fb, ho, 0)
    assert len(mv) == 300 and [i for i, m in enumerate(mv) if m[2]] == [100, 255, 256]
    caps = {"inbound": 2}
    want = check(fb, ho, None, caps, "cap reached by the last move of a group", solve_records=False)
    assert [(b["first_move"], b["n_moves"], b["max_inbound"], b["closed_by"]) for b in want[0].batches] == [(0, 256, 2, R.INBOUND), (256, 44, 1, R.END)]
    r = replay(mv, caps)
    assert (r.clean, r.replayed) == (1, 1)


def test_cap_exceeded_by_a_lane_that_is_not_lane_0():
    moved = {p: [p % 11, (p + 1) % 11, 11] if p in (10, 20, 30) else [p % 11, (p + 1) % 11, 200] for p in range(64)}
    fb, ho = crafted([(64, moved)], N=12, n_cur=11)
    want = check(fb, ho, None, {"inbound": 2}, "lane 30 exceeds", solve_records=False)
    assert [(b["first_move"], b["n_moves"], b["closed_by"]) for b in want[0].batches] == [(0, 30, R.INBOUND), (30, 34, R.END)]


def test_many_closes_in_one_group_and_reset():
    """cap_inbound 1 on 12 brokers: 13 consecutive moves must repeat a receiver (pigeonhole), so a group of 256 closes many times;
    the same for cap_outbound 1 where every lost cell names a node; a node at its cap in batch k is taken again in batch k + 1"""
    fb, ho = crafted([(900, random_moves(900, 400, 12, 12, 5)), (300, random_moves(300, 120, 12, 12, 6))])
    mv = scenario_moves(fb, ho, 0)
    for caps in ({"inbound": 1}, {"outbound": 1}):
        assert replay(mv, caps).most_closes >= 4
        want = check(fb, ho, None, caps, ("many closes", caps), solve_records=False)
        side = 2 if "inbound" in caps else 3
        resets = 0
        for a, b in zip(want[0].batches, want[0].batches[1:]):
            closer = mv[b["first_move"]]                                     # the move that closed batch a names a node at its cap ...
            assert any(sum(1 for m in mv[a["first_move"]:b["first_move"]] if n in m[side]) == 1 for n in closer[side])
            resets += 1                                                      # ... and is in batch b: the counters were reset
        assert resets >= 4
    # every closed_by value in one call
    want = check(fb, ho, None, {"inbound": 2, "outbound": 2, "max_moves": 5}, "every reason", solve_records=False)
    assert {b["closed_by"] for b in want[0].batches} == {R.END, R.MAX_MOVES, R.INBOUND, R.OUTBOUND}
    rec = want[0].record
    assert min(rec["closed_by_max_moves"], rec["closed_by_inbound"], rec["closed_by_outbound"]) >= 1


def test_clean_and_mixed_paths():
    fb, ho = crafted([(1100, random_moves(1100, 700, 100, 100, 9))], N=100)
    mv = scenario_moves(fb, ho, 0)
    r = replay(mv, {"inbound": BIG, "outbound": BIG, "max_moves": BIG})
    assert r.groups == 3 and r.replayed == 0                                # every group passes clean
    check(fb, ho, None, {"inbound": BIG, "outbound": BIG, "max_moves": BIG}, "clean", solve_records=False)
    r = replay(mv, {"inbound": 8})
    assert r.clean >= 1 and r.replayed >= 1, (r.clean, r.replayed)          # both paths occur
    check(fb, ho, None, {"inbound": 8}, "mixed", solve_records=False)


@pytest.mark.parametrize("max_moves", [1, 64, 65])
def test_max_moves(max_moves):
    fb, ho = crafted([(700, random_moves(700, 300, 12, 12, 3))])
    want = check(fb, ho, None, {"max_moves": max_moves}, ("max_moves", max_moves), solve_records=False)
    sizes = [b["n_moves"] for b in want[0].batches]
    assert sizes == [max_moves] * (300 // max_moves) + ([300 % max_moves] if 300 % max_moves else [])
    assert all(b["closed_by"] == R.MAX_MOVES for b in want[0].batches[:-1]) and want[0].batches[-1]["closed_by"] == R.END


def test_departed_cells_are_in_neither_set():
    """a remove-brokers variant: lost cells on brokers outside the set are departed, so cap_outbound 1 closes nothing for them"""
    fb, ho = crafted([(300, {p: [p % 10, (p + 1) % 10, (p + 5) % 10] for p in range(300) if (p + 2) % 12 >= 10})], N=10, n_cur=10, extra_cur=2)
    mv = scenario_moves(fb, ho, 0)
    assert len(mv) >= 40 and all(not m[3] for m in mv)                       # every lost cell is departed
    want = check(fb, ho, None, {"outbound": 1}, "departed", solve_records=False)
    assert want[0].record["n_batches"] == 1 and want[0].batches[0]["max_outbound"] == 0


# ---- the crafted cases the MI355X runs too (tests/crafted_cases.py, tests/test_batches_crafted_gpu.py) ---------------------------
@pytest.mark.parametrize("run", CC.runs(CC.BATCH_CASES), ids=CC.run_id)
def test_crafted_case(run):
    """every case under each of its caps, on int32 cells and (where the form exists) 16-bit cells; the case's own claims about
    what the checker shows are held first (Case.wants)"""
    name, cells16 = run
    case = CC.batches_case(name)
    fb, ho, cur16 = case.tables(cells16)
    kw = dict(cells16=True, cur16=cur16) if cells16 else {}
    for caps, w in zip(case.caps, case.wants(cells16)):
        check(fb, ho, case.select, caps, (name, caps, cells16), solve_records=False, want=case.listed(w), **kw)


def test_a_group_that_reaches_its_cap_is_not_replayed():
    """a counter AT its cap fits ("if no counter read back exceeds its cap ... the whole group is in"): the one group of
    `cap_reached_in_group` runs through the wave collectives of a call whose cap nobody reaches, and a call that closes inside the
    group through more (the replay's ballots).  The records cannot tell: a needless replay gives the same ones."""
    case = CC.batches_case("cap_reached_in_group")
    assert replay(case.wants(False)[0].moves, case.caps[0]).clean == 1
    clean = emu(case.fb, case.ho, [0], CC.ALL_BIG, 4)[2]["collectives"]
    got = emu(case.fb, case.ho, [0], case.caps[0], 4)[2]["collectives"]
    replayed = emu(case.fb, case.ho, [0], {"inbound": 1}, 4)[2]["collectives"]
    assert 0 < clean == got < replayed, (clean, got, replayed)


def test_crafted_cases_without_a_16_bit_form():
    """exactly the cases whose out lists name an id outside the broker set have none, and the helper refuses them; the 16-bit
    form of every other case holds the move list of its int32 form"""
    for name in CC.BATCH_CASES:
        case = CC.batches_case(name)
        if name in CC.INT32_ONLY:
            with pytest.raises(ValueError):
                CC.cells16_form(case.fb, case.ho)
        else:
            _, ho16, cur16 = case.tables(True)
            assert scenario_moves(case.fb, ho16, 0, True, cur16) == scenario_moves(case.fb, case.ho, 0), name


def test_crafted_cases_the_plan_refuses():
    """what CC.plan_refusal says of every run is what the planner says: lists 8 wide at the passes' node limits and 16-bit cells
    beyond lists 3 wide reach the kernel bodies on the emulator only"""
    import emu_lib
    for get, names in ((CC.batches_case, CC.BATCH_CASES), (CC.rounds_case, CC.ROUND_CASES)):
        for name, cells16 in CC.runs(names):
            case = get(name)
            rc, text = emu_lib.describe(case.fb, 0, cells16)
            why = CC.plan_refusal(name, case, cells16)
            assert (rc == 0 and not why) or (rc == E_UNSUPPORTED and why and why in text), (name, cells16, rc, text, why)
    # ... and the ceilings are the last counts the plan takes at those widths
    for W, N in ((8, CC.W8_CEILING), (5, CC.W5_CEILING)):
        for sparse in (False, True):
            ids = lambda n: [7 + 3 * i for i in range(n)] if sparse else None
            assert emu_lib.describe(crafted([(40, {})], N=N, width=W, ids=ids(N))[0])[0] == 0
            assert emu_lib.describe(crafted([(40, {})], N=N + 1, width=W, ids=ids(N + 1))[0])[0] == E_UNSUPPORTED


# ---- oracle-solved batches: rows and cells, widths, cell types, lookups -------------------------------------------------------
CAPS = ({"inbound": 1}, {"inbound": 3, "outbound": 2, "max_moves": 50})


@pytest.mark.parametrize("name", ["mixed7", "mixed42", "widths_4_5", "widths_6_8", "sparse", "dense_and_sparse", "degenerate", "many_brokers"])
def test_solved_batches(name):
    """OK and failed topics, olen == 0 rows, ragged cur_len, widths 2-3 / 4-5 / 6-8, dense and sparse ids, scenarios without topics
    and without brokers: int32 and 16-bit cells against the checker, and the sums against the solve's scenario records"""
    fb, ho, _ = solved(name)
    ho16, cur16 = solved16(fb)
    for caps in CAPS:
        want = check(fb, ho, None, caps, (name, caps))
        assert sum(w.record["n_moves"] for w in want) > 0
        want16 = check(fb, ho16, None, caps, (name, caps, "16-bit"), cells16=True, cur16=cur16, solve_records=False)
        if np.array_equal(np.where(ho16.out == abi.KAS_CELL16_NONE, -1, ho16.out.astype(np.int64)), index_form_out(fb, ho)):
            assert [w.record for w in want16] == [w.record for w in want]


def index_form_out(fb, ho):
    """ho.out as node indices (the 16-bit form's cells), where the int32 solve and the 16-bit solve agree row by row"""
    from kafka_assigner_amd.flatten import _topic_scenarios
    out = np.full(ho.out.shape, -1, np.int64)
    owner = _topic_scenarios(fb)
    for t in range(fb.n_topics):
        td, s = fb.topics[t], int(owner[t])
        if s < 0:
            continue
        n, off = int(fb.scen["n_nodes"][s]), int(fb.scen["node_off"][s])
        ids = fb.node_id[off:off + n]
        oo, cells = int(td["out_off"]), max(int(td["n_partitions"]), 0) * int(td["out_width"])
        v = ho.out[oo:oo + cells].astype(np.int64)
        idx = np.searchsorted(ids, v) if n else np.zeros(v.shape, np.int64)
        ok = (v >= 0) & (idx < n)
        ok[ok] &= ids[idx[ok]] == v[ok]
        out[oo:oo + cells] = np.where(ok, idx, -1)
    return out


def test_statuses_and_widths_are_exercised():
    """the guard of test_solved_batches: some OK topic has ragged rows, and each width class occurs"""
    ragged = False
    for name in ("mixed7", "mixed42"):
        fb, ho, _ = solved(name)
        st = ho.topic_results["status"][:fb.n_topics]
        ragged |= bool(((fb.topics["cur_len_off"] >= 0) & (st == abi.KAS_OK)).any())
    assert ragged
    widths = set()
    for name in ("mixed7", "widths_4_5", "widths_6_8"):
        fb, ho, _ = solved(name)
        widths |= {max(int(a), int(b)) for a, b in zip(fb.topics["cur_width"], fb.topics["out_width"])}
    assert widths & {2, 3} and widths & {4, 5} and widths & {6, 7, 8}


def test_ok_failed_and_skipped_topics_in_one_scenario():
    fb, ho, _ = solved("mixed7")
    st = ho.topic_results["status"].copy()
    # make it certain: the second topic of the first scenario with several topics is marked failed, the third skipped (any status
    # but KAS_OK contributes nothing, whatever its rows hold)
    s = next(s for s in range(fb.n_scenarios) if int(fb.scen["topic_count"][s]) >= 2)
    b = int(fb.scen["topic_begin"][s])
    from copy import copy
    ho2 = copy(ho)
    ho2.topic_results = ho.topic_results.copy()
    ho2.topic_results["status"][b + 1] = abi.KAS_OK + 1
    if int(fb.scen["topic_count"][s]) >= 3:
        ho2.topic_results["status"][b + 2] = abi.KAS_OK + 2
    want = check(fb, ho2, None, {"inbound": 2}, "a failed topic between OK ones", solve_records=False)
    full = batches_ref(fb, ho, [s], {"inbound": 2})[0]
    assert want[s].record["n_moves"] < full.record["n_moves"] or st[b + 1] != abi.KAS_OK
    assert all(m[0] != 1 for m in want[s].moves)


def test_stale_id_stays_departed():
    """sparse ids, the removed broker above every id of the set: with its id all over the LDS before the launch, its replicas still
    name no node"""
    fb, ho, _ = solved("beyond_the_table")
    for fill in (0xCDCDCDCD, STALE_ID, 0):
        check(fb, ho, None, {"outbound": 1}, ("stale id", fill), lds_fill=fill)


def test_listing_and_stride():
    fb, ho, _ = solved("degenerate")                                         # scenario 1 has no topics: no moves
    caps = {"inbound": 1}
    want = check(fb, ho, [0, -1, 1, 0, 2, -1], caps, "listing")
    assert want[1] is None and want[2].record["n_batches"] == 0 and want[0].record == want[3].record
    nb = want[0].record["n_batches"]
    assert nb >= 3
    check(fb, ho, [0, 0], caps, "stride exactly n_batches", stride=nb)
    check(fb, ho, [0, 0], caps, "stride n_batches - 1: the guard stays", stride=nb - 1)
    # counts only: stride 0 with batches == NULL
    rc, err, scen, _, _ = emu_rc(fb, ho, [0, -1], caps, 0, null_batches=True)
    assert rc == 0, err
    assert_same_batches(batches_ref(fb, ho, [0, -1], caps), scen, np.zeros(0, abi.MOVE_BATCH_DTYPE), 0)
    # the same inputs give the same bytes
    a = emu(fb, ho, [0, 2], caps, nb + 1)
    b = emu(fb, ho, [0, 2], caps, nb + 1)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_chaos_schedules():
    """the wavefronts released at random (KAS_EMU_CHAOS): the barriers still meet, the records are the same"""
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_batches_cpu as t\n"
            "fb, ho = t.crafted([(1100, t.random_moves(1100, 600, 12, 12, 4)), (200, t.random_moves(200, 90, 12, 12, 8))])\n"
            "for caps in ({'inbound': 1}, {'inbound': 8, 'outbound': 6}, {'max_moves': 65}, {'inbound': t.BIG}):\n"
            "    t.check(fb, ho, [0, -1, 0], caps, ('chaos', caps), solve_records=False)\n"
            "fb, ho, _ = t.solved('widths_4_5')\n"
            "t.check(fb, ho, None, {'inbound': 1}, 'chaos, lists 5 wide')\n" % (ROOT, os.path.join(ROOT, "tests")))
    for seed in ("1", "7"):
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, KAS_EMU_CHAOS=seed), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr


# ---- refusals, the node limit, the planner ----------------------------------------------------------------------------------
def test_refusals_in_order():
    fb, ho, _ = solved("degenerate")
    S = fb.n_scenarios
    ok = {"inbound": 1}
    scen = np.zeros(4, abi.SCENARIO_BATCHES_DTYPE)
    recs = np.zeros(64, abi.MOVE_BATCH_DTYPE)

    def call(spec=None, out=None, select=(0,)):
        rc, err, *_ = emu_rc(fb, ho, list(select), ok, 4, spec=spec, raw_out=out)
        return rc, err

    good = abi.Batches(scen.ctypes.data, recs.ctypes.data, 4)
    for bad in (abi.BatchSpec(-1, 0, 0, 0), abi.BatchSpec(0, -1, 0, 0), abi.BatchSpec(0, 0, -1, 0), abi.BatchSpec(0, 0, 0, 0), abi.BatchSpec(1, 0, 0, 7)):
        rc, err = call(spec=bad, out=abi.Batches(None, None, -1), select=(S,))      # everything behind the spec is wrong too
        assert rc == E_INVALID and "kas_batch_spec" in err, (rc, err)
    rc, err = call(out=abi.Batches(None, None, -1), select=(S,))
    assert rc == E_INVALID and "negative stride" in err
    for o in (abi.Batches(None, recs.ctypes.data + 1, 4), abi.Batches(scen.ctypes.data + 2, None, 4)):
        rc, err = call(out=o, select=(S,))
        assert rc == E_INVALID and "NULL" in err
    for o in (abi.Batches(scen.ctypes.data + 2, recs.ctypes.data, 4), abi.Batches(scen.ctypes.data, recs.ctypes.data + 1, 4)):
        rc, err = call(out=o, select=(S,))
        assert rc == E_INVALID and "aligned" in err
    for sel in ((S,), (-2,), (0, S + 5)):
        rc, err = call(out=good, select=sel)
        assert rc == E_INVALID and "out of range" in err
    rc, err = call(out=abi.Batches(scen.ctypes.data, recs.ctypes.data, (1 << 31) // 32 + 1), select=(0,))
    assert rc == E_UNSUPPORTED and "2^31" in err
    rc, err = call(out=abi.Batches(scen.ctypes.data, recs.ctypes.data, (1 << 31) // 32 // 2 + 1), select=(0, 1))
    assert rc == E_UNSUPPORTED and "2^31" in err
    assert call(out=good)[0] == 0


def test_node_limit():
    """KAS_BATCH_NODE_LIMIT is what the widest kernel's LDS layout leaves; a listed scenario above it is refused before the room is
    looked at, an unlisted one is not"""
    L = _emu_lib()
    limit = const("NODE_LIMIT")
    assert limit == abi.KAS_BATCH_NODE_LIMIT == int(re.search(r"#define KAS_BATCH_NODE_LIMIT (\d+)", open(HEADER).read()).group(1))
    lay = (C.c_int32 * 5)()
    for W in (3, 5, 8):
        for c16 in (0, 1):
            L.kas_emu_batches_lds(limit, W, c16, lay)
            assert lay[4] <= 160 * 1024 and lay[0] >= 8 * limit and lay[1] >= lay[0] + (0 if c16 else 4 * limit)
            assert lay[3] + 8 * const("QUEUE") == lay[4] and lay[3] - lay[2] >= 4 * W * const("QUEUE")
    # 12 bytes a node (two counters, 4 bytes of lookup) beside the queue of lists 8 wide, the misc words and the alignment slack
    assert limit == (160 * 1024 - const("QUEUE") * (4 * 8 + 8) - 256 - 32) // 12
    big = Scenario(list(range(limit + 1)), {}, [Topic("t", {0: [0, 1, 2]}, 3)])
    small = scenario(5, 30, 5, [T(100)], remove=[4])
    fb = flatten([small, big])
    from kafka_assigner_amd.flatten import host_tables
    _, ho = host_tables(fb)
    ho.out[:fb.cur.size] = fb.cur[:ho.out.size] if ho.out.size <= fb.cur.size else np.resize(fb.cur, ho.out.size)
    rc, err, *_ = emu_rc(fb, ho, [0, 1], {"inbound": 1}, (1 << 31) // 32)
    assert rc == E_UNSUPPORTED and "KAS_BATCH_NODE_LIMIT" in err
    rc, err, *_ = emu_rc(fb, ho, None, {"inbound": 1}, 2)
    assert rc == E_UNSUPPORTED and "KAS_BATCH_NODE_LIMIT" in err
    rc, err, *_ = emu_rc(fb, ho, [0, -1], {"inbound": 1}, 2)
    assert rc == 0, err


def _plan(fb, select, spec, out, cells16=False, ranges=0):
    L = _emu_lib()
    bd = batch_desc(fb)
    if cells16:
        bd.node_id = None
    lens = (C.c_int64 * 4)(int(fb.cur.size), int(fb.out_len), int(fb.aux.size), int(fb.ctx.size))
    head = (C.c_int64 * 4)()
    nb = const("HB_FINAL")
    by = (C.c_int64 * nb)()
    err = C.create_string_buffer(512)
    sel = None if select is None else np.ascontiguousarray(select, dtype=np.int32)
    rc = L.kas_emu_batches_host_call(C.byref(bd), lens, int(cells16), None if sel is None else sel.ctypes.data, -1 if sel is None else int(sel.size),
                                     C.addressof(spec) if spec is not None else None, C.addressof(out) if out is not None else None, ranges, head, by,
                                     err, 512)
    return rc, err.value.decode(), list(head), list(by)


def test_planner_bytes():
    """the buffers of a batches call lie behind KAS_HB_EVERY (+ the moves pass's two tables); a plain call plans what it planned"""
    fb, ho, _ = solved("mixed7")
    S, T_ = fb.n_scenarios, fb.n_topics
    scen = np.zeros(8, abi.SCENARIO_BATCHES_DTYPE)
    recs = np.zeros(64, abi.MOVE_BATCH_DTYPE)
    spec = abi.batch_spec({"inbound": 5})
    out = abi.Batches(scen.ctypes.data, recs.ctypes.data, 7)
    every, final = const("HB_EVERY"), const("HB_FINAL")
    assert final == every + 5
    rc, err, head, by = _plan(fb, [0, -1, 2], spec, out)
    assert rc == 0, err
    n_max = max(int(fb.scen["n_nodes"][0]), int(fb.scen["n_nodes"][2]))
    assert head[:2] == [3, n_max]
    assert by[const("BT_SDESC")] == 32 * (S + 1) and by[const("BT_NODE_ID")] == 4 * (fb.node_id.size + 1)
    assert by[const("BT_SELECT")] == 4 * 4 and by[const("BT_SCEN")] == 32 * 4 and by[const("BT_BATCHES")] == 32 * (3 * 7 + 1)
    assert by[const("MV_SCEN")] == 32 * (S + 1) and by[const("MV_SEGS")] == 56 * (T_ + 1)
    rc, err, head, by_all = _plan(fb, None, spec, abi.Batches(scen.ctypes.data, None, 0))
    assert rc == 0 and head[0] == S and by_all[const("BT_BATCHES")] == 32
    # the same batch without a batches pass: nothing behind KAS_HB_EVERY, no moves tables, and everything else as in the batches call
    rc, err, _, plain = _plan(fb, [], None, None)
    assert rc == 0, err
    assert plain[every:] == [0] * 5 and plain[const("MV_SCEN")] == 0 and plain[const("MV_SEGS")] == 0
    same = [i for i in range(every) if i not in (const("MV_SCEN"), const("MV_SEGS"))]
    assert [plain[i] for i in same] == [by[i] for i in same]
    # a 16-bit call solved on its own cells uploads no node ids
    fb3 = flatten([scenario(5, 30, 5, [T(100)], remove=[4])])
    rc, err, head, by16 = _plan(fb3, None, spec, out, cells16=True)
    assert rc == 0, err
    assert by16[const("BT_NODE_ID")] == (0 if head[3] else 4 * (fb3.node_id.size + 1))
    # refusals of the planner come in the documented order, behind the solve's own
    rc, err, *_ = _plan(fb, [S], abi.BatchSpec(0, 0, 0, 0), out)
    assert rc == E_INVALID and "kas_batch_spec" in err
    rc, err, *_ = _plan(fb, [S], spec, out)
    assert rc == E_INVALID and "out of range" in err


def test_header_and_library():
    """the header declares the four entries and the records; the library exports them (where it is built)"""
    text = open(HEADER).read()
    for name in abi.BATCHES_ENTRIES:
        assert re.search(r"\bint %s\(" % name, text), name
        assert name in native.SYMBOLS
    for name in ("kas_batch_spec", "kas_move_batch", "kas_scenario_batches", "kas_batches", "KAS_BATCH_END_OF_LIST", "KAS_BATCH_OUTBOUND"):
        assert name in text
    assert "#define KAS_ABI_VERSION 6" in text
    for f in abi.MOVE_BATCH_FIELDS + abi.SCENARIO_BATCHES_FIELDS:
        assert re.search(r"\b%s\b" % f, text), f
    lib = os.path.join(CSRC, "libkas_hip.so")
    if os.path.exists(lib):
        syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
        for name in abi.BATCHES_ENTRIES:
            assert re.search(r"\bT %s\b" % name, syms), name


def test_batch_spec_mirror():
    sp = abi.batch_spec({"inbound": 5, "max_moves": 9})
    assert (sp.cap_inbound, sp.cap_outbound, sp.max_moves, sp.reserved) == (5, 0, 9, 0)
    assert abi.batch_spec(sp) is sp
    with pytest.raises(ValueError):
        abi.batch_spec({"inbound": 1, "outbond": 2})
    assert abi.BATCH_CLOSED_BY[abi.KAS_BATCH_INBOUND] == "inbound" and abi.BATCH_CLOSED_BY[abi.KAS_BATCH_END_OF_LIST] == "end_of_list"


# ---- WhatIf, without a GPU ----------------------------------------------------------------------------------------------------
def test_whatif_argument_handling():
    """batches= / batch_room= are checked before anything is solved; batches() and reassignment_batches() over hand-made records"""
    from kafka_assigner_amd.whatif import Variant, VariantResult, WhatIf
    plan = WhatIf({b: "r%d" % (b % 3) for b in range(6)}, {"a": {0: [0, 1, 2], 1: [1, 2, 3]}, "b": {0: [2, 3, 4], 5: [3, 4, 5]}})
    vs = [Variant(remove=[5])]
    for call in (plan.solve, plan.best, plan.front):
        for bad in ({"inbound": -1}, {}, {"inbound": 0, "outbound": 0, "max_moves": 0}, {"inbund": 3}):
            with pytest.raises(ValueError):
                call(vs, batches=bad)
        with pytest.raises(ValueError):
            call(vs, batches={"inbound": 1}, batch_room=-1)
    with pytest.raises(ValueError):
        plan.solve(vs, batches={"inbound": 1}, solve_fn=lambda fb: None)
    R_, L_, O_ = abi.KAS_MOVE_REPLICAS, abi.KAS_MOVE_LEADER, abi.KAS_MOVE_ORDER
    recs = np.array([(0, 0, R_ | L_, 3, 1, 1, 0), (0, 1, L_, 3, 0, 0, 3), (1, 0, R_, 3, 1, 1, 6), (1, 5, O_, 3, 0, 0, 9)], abi.MOVE_DTYPE)
    cells = np.array([4, 1, 2, 2, 1, 3, 0, 3, 4, 4, 3, 5], np.int32)
    bt = np.array([(0, 1, 0, 0, 1, 1, 1, abi.KAS_BATCH_INBOUND), (1, 1, 1, 0, 1, 1, 1, abi.KAS_BATCH_END_OF_LIST)], abi.MOVE_BATCH_DTYPE)
    r = VariantResult(label="x", status=0, fail_topic=None, fail_partition=-1, moved_replicas=2, moved_partitions=2, digest=0, _plan=plan,
                      _moves=(recs, cells), _moves_mask=7, n_batches=2, _batches=bt)
    assert [b["closed_by"] for b in r.batches()] == ["inbound", "end_of_list"] and [b["topic"] for b in r.batches()] == ["a", "b"]
    objs = r.reassignment_batches()
    assert [[(p["topic"], p["partition"]) for p in o["partitions"]] for o in objs] == [[("a", 0), ("a", 1)], [("b", 0), ("b", 5)]]
    assert [p for o in objs for p in o["partitions"]] == r.reassignment()["partitions"]
    assert [len(o["partitions"]) for o in r.reassignment_batches(kinds=("replicas",))] == [1, 1]
    r.n_batches = 3                                                          # more batches than records: the room was too small
    with pytest.raises(ValueError):
        r.reassignment_batches()
    bare = VariantResult(label="x", status=0, fail_topic=None, fail_partition=-1, moved_replicas=0, moved_partitions=0, digest=0, _plan=plan)
    with pytest.raises(ValueError):
        bare.batches()
    assert bare.n_batches is None


def test_plain_calls_plan_the_bytes_they_planned():
    """the batches inputs default to "no batches pass": a plain call and a topic call, planned before and after a batches call,
    give the bytes they gave, nothing of theirs lies behind KAS_HB_EVERY, and the topic driver's plain call (which knows nothing of
    the new inputs) is this driver's plain call.  (tests/test_host_call.py, test_moves_cpu.py, test_choose_cpu.py and
    test_topics_cpu.py pin the figures themselves.)"""
    import test_topics_cpu as tt
    fb, ho, _ = solved("mixed7")
    every, final = const("HB_EVERY"), const("HB_FINAL")
    rc, err, _, before = _plan(fb, [], None, None)
    assert rc == 0, err
    scen = np.zeros(8, abi.SCENARIO_BATCHES_DTYPE)
    assert _plan(fb, [0, 1, -1], abi.batch_spec({"inbound": 1}), abi.Batches(scen.ctypes.data, None, 0))[0] == 0
    rc, err, _, after = _plan(fb, [], None, None)
    assert rc == 0 and before == after and after[every:] == [0] * (final - every)
    TL = tt._emu_lib()
    assert TL.kas_emu_topic_buffers(0) == every
    lens = (C.c_int64 * 4)(int(fb.cur.size), int(fb.out_len), int(fb.aux.size), int(fb.ctx.size))
    by = (C.c_int64 * every)()
    region = C.c_int64()
    e = C.create_string_buffer(512)
    bd = batch_desc(fb)
    assert TL.kas_emu_topic_host_call(C.byref(bd), lens, 0, 0, 0, 0, 0, 0, by, C.byref(region), e, 512) == 0, e.value
    assert list(by) == before[:every]
    assert TL.kas_emu_topic_host_call(C.byref(bd), lens, 0, 0, 1, 1, 0, 0, by, C.byref(region), e, 512) == 0, e.value
    topic_call = list(by)
    assert TL.kas_emu_topic_host_call(C.byref(bd), lens, 0, 0, 1, 1, 0, 0, by, C.byref(region), e, 512) == 0, e.value
    assert list(by) == topic_call and topic_call != before[:every]

"""Packed rounds (include/kas_abi.h: kas_round_spec / kas_move_round / kas_scenario_rounds / kas_rounds) without a GPU.

- The kernel body (kafka-assigner_amd/csrc/kas_rounds_body.h) compiled with g++ against tests/emu/kas_wave.h and stepped on CPU
  fibers (tests/emu/rounds_driver.cpp) against the checker (tests/rounds_ref.py: the header's loop in plain Python): over
  oracle-solved batches of tests/impact_batches.py, and over crafted out tables whose lists exceed the kernel's queue (several
  tiles) and its window of round counters (several walks).
- The crafted cases of tests/crafted_cases.py, which tests/test_rounds_crafted_gpu.py runs on the GPU.
- The refusals in their order, the node limit, the host call planner's bytes, the ABI, WhatIf's argument handling.
- The quality guards over the what-if batch, from the checker alone: rounds against consecutive batches and the lower bound.
"""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import crafted_cases as CC
import rounds_ref as R
import test_batches_cpu as tb
from batches_ref import cut, scenario_moves
from impact_batches import T, scenario, solved
from kafka_assigner_amd import abi, native
from kafka_assigner_amd.flatten import Scenario, Topic, batch_desc, flatten, to_cells16
from rounds_ref import assert_same_rounds, check_invariants, first_fit, lower_bound, monotone, rounds_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "kafka-assigner_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "kas_abi.h")
E_INVALID, E_UNSUPPORTED = abi.KAS_E_INVALID_ARG, abi.KAS_E_UNSUPPORTED
FILL = 0x5A5A5A5A                                   # what the output arrays hold before a call
CAPS = ({"inbound": 1}, {"inbound": 3, "outbound": 2}, {"outbound": 1}, {"inbound": 10 ** 6})
NAMES = ["mixed42", "degenerate", "widths_4_5", "widths_6_8", "sparse", "many_brokers"]
CONSTS = ("HB_BUFFERS", "HB_FINAL", "WINDOW", "ITEM_ROWS", "NODE_LIMIT", "QUEUE", "RD_SCEN", "RD_ROUNDS", "RD_OF", "BT_SDESC", "BT_NODE_ID",
          "BT_SELECT", "MV_SCEN", "MV_SEGS")
_LIB = None


# ---- the emulator ---------------------------------------------------------------------------------------------------------
def _emu_lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    so = os.path.join(EMU, "libkas_emu_rounds.so")
    srcs = [os.path.join(EMU, f) for f in ("rounds_driver.cpp", "emu_driver.cpp")]
    deps = srcs + [os.path.join(EMU, "kas_wave.h"), HEADER] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        tmp = so + ".tmp%d" % os.getpid()
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unused-parameter", "-Wno-unknown-pragmas",
                               "-I" + os.path.join(ROOT, "tests"), "-I" + CSRC, "-I" + os.path.join(ROOT, "include"),
                               "-o", tmp] + srcs)
        os.replace(tmp, so)
    L = C.CDLL(so)
    L.kas_emu_rounds.restype = C.c_int
    L.kas_emu_rounds.argtypes = [C.POINTER(abi.BatchDesc), C.POINTER(abi.Tables), C.c_int, C.c_void_p, C.c_int32, C.POINTER(abi.RoundSpec),
                                 C.POINTER(abi.Rounds), C.c_uint32, C.POINTER(C.c_int32), C.c_char_p, C.c_int]
    L.kas_emu_rounds_host_call.restype = C.c_int
    L.kas_emu_rounds_host_call.argtypes = [C.POINTER(abi.BatchDesc), C.POINTER(C.c_int64), C.c_int, C.c_int, C.c_void_p, C.c_int32, C.c_void_p,
                                           C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_char_p, C.c_int]
    L.kas_emu_rounds_const.restype = C.c_int
    L.kas_emu_rounds_const.argtypes = [C.c_int]
    L.kas_emu_rounds_lds.restype = None
    L.kas_emu_rounds_lds.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]
    _LIB = L
    return L


def const(name):
    return _emu_lib().kas_emu_rounds_const(CONSTS.index(name))


def emu_rc(fb, ho, select, caps, round_stride, move_stride, cells16=False, cur16=None, lds_fill=0xCDCDCDCD, spec=None, null_arrays=False,
           raw_out=None):
    """kas_emu_rounds over the tables a solve left in `ho`: (rc, text, scenario records, round records, round_of, info)"""
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
    rs, ms = max(round_stride, 0), max(move_stride, 0)
    scen = np.full(max(n, 1) * 8, FILL, np.int32).view(abi.SCENARIO_ROUNDS_DTYPE)[:n]
    recs = np.full(max(n * rs, 1) * 4, FILL, np.int32).view(abi.MOVE_ROUND_DTYPE)[:n * rs]
    rof = np.full(max(n * ms, 1), FILL, np.int32)[:n * ms]
    o = raw_out if raw_out is not None else abi.Rounds(scen.ctypes.data if n else None, None if null_arrays or not recs.size else recs.ctypes.data,
                                                       round_stride, None if null_arrays or not rof.size else rof.ctypes.data, move_stride)
    sp = spec if spec is not None else abi.round_spec(caps)
    info = (C.c_int32 * 4)()
    err = C.create_string_buffer(512)
    rc = L.kas_emu_rounds(C.byref(bd), C.byref(t), int(cells16), None if sel is None else sel.ctypes.data, -1 if sel is None else n,
                          C.byref(sp), C.byref(o), lds_fill, info, err, 512)
    return rc, err.value.decode(), scen, recs, rof, dict(lds=int(info[0]), n_cap=int(info[1]), W=int(info[2]), collectives=int(info[3]))


def emu(fb, ho, select, caps, round_stride, move_stride, **kw):
    rc, err, scen, recs, rof, info = emu_rc(fb, ho, select, caps, round_stride, move_stride, **kw)
    assert rc == 0, (rc, err)
    return scen, recs, rof, info


def check(fb, ho, select, caps, what, round_stride=None, move_stride=None, solve_records=True, want=None, **kw):
    """One call on the emulator against the checker, with the invariants; returns the checker's list (want: that list, where the
    caller has it already)"""
    select = list(range(fb.n_scenarios)) if select is None else list(select)
    want = want or rounds_ref(fb, ho, select, caps, cells16=kw.get("cells16", False), cur16=kw.get("cur16"))
    if round_stride is None:
        round_stride = max([w.record["n_rounds"] for w in want if w is not None] + [1]) + 2
    if move_stride is None:
        move_stride = max([w.record["n_moves"] for w in want if w is not None] + [1]) + 3
    scen, recs, rof, _ = emu(fb, ho, select, caps, round_stride, move_stride, **kw)
    assert_same_rounds(want, scen, recs, round_stride, rof, move_stride, fill=FILL, what=what)
    for j, s in enumerate(select):
        if want[j] is not None:
            sr = ho.scenario_results
            check_invariants(want[j], caps, sr["moved_partitions"][s] if solve_records else None, sr["moved_replicas"][s] if solve_records else None,
                             what=(what, j))
    return want


# ---- the checker itself -------------------------------------------------------------------------------------------------------
def test_the_loop_by_hand():
    """five moves on nodes 0..3 under inbound 1 / outbound 1, worked by hand from the header's loop"""
    mv = [(0, 0, (0,), (1,)), (0, 1, (0,), (2,)), (0, 2, (3,), (1,)), (0, 3, (0, 3), ()), (0, 4, (), (2,))]
    ro, by_in, by_out = monotone(mv, {"inbound": 1, "outbound": 1})
    # move 1: node 0 is full in round 0 -> 1.  move 2: Out node 1 is full in round 0 -> 1 (only Out raised it).  move 3: node 0 holds
    # round 1 (full) -> 2, node 3 holds round 1 (full) -> 2.  move 4: Out node 2 holds round 1, full -> 2.
    assert ro == [0, 1, 1, 2, 2] and (by_in, by_out) == (2, 2)
    rec, rd = R.records(mv, ro, by_in, by_out)
    assert rec == dict(n_rounds=3, n_moves=5, replicas=5, max_round_moves=2, max_round_replicas=2, raised_by_inbound=2, raised_by_outbound=2, reserved=0)
    assert [r["first_move"] for r in rd] == [0, 1, 3] and [r["replicas"] for r in rd] == [1, 2, 2]
    assert first_fit(mv, {"inbound": 1, "outbound": 1}) == [0, 1, 1, 2, 0]          # a true first fit returns to round 0
    assert lower_bound(mv, {"inbound": 1, "outbound": 1}) == 3 and lower_bound([], {"inbound": 1}) == 0
    # a node never returns to a round it left: the monotone rule wastes round 0's room on node 0 here
    mv = [(0, 0, (0,), ()), (0, 1, (0, 1), ()), (0, 2, (1,), ())]
    assert monotone(mv, {"inbound": 1})[0] == [0, 1, 2] and first_fit(mv, {"inbound": 1}) == [0, 1, 0]


# ---- oracle-solved batches: rows and cells, widths, cell types, lookups -------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_solved_batches(name):
    """the six named batches on int32 and 16-bit cells under the four caps against the checker, the sums against the solve's
    scenario records; a cap nobody reaches puts every move in round 0"""
    fb, ho, _ = solved(name)
    ho16, cur16 = tb.solved16(fb)
    same16 = np.array_equal(np.where(ho16.out == abi.KAS_CELL16_NONE, -1, ho16.out.astype(np.int64)), tb.index_form_out(fb, ho))
    moved = 0
    for caps in CAPS:
        want = check(fb, ho, None, caps, (name, caps))
        moved += sum(w.record["n_moves"] for w in want)
        want16 = check(fb, ho16, None, caps, (name, caps, "16-bit"), cells16=True, cur16=cur16, solve_records=False)
        if same16:
            assert [w.record for w in want16] == [w.record for w in want]
        if caps == CAPS[3]:
            assert all(w.record["n_rounds"] == (1 if w.record["n_moves"] else 0) for w in want)
            assert all(w.record["raised_by_inbound"] == 0 and w.record["max_round_moves"] == w.record["n_moves"] for w in want)
    assert moved > 0


# ---- lists beyond the queue and beyond the window ---------------------------------------------------------------------------------
def test_a_list_beyond_the_queue():
    """1,500 moves over three tiles of one topic and a second topic: the sequential wavefront crosses tile boundaries with its
    nodes' words as the tile before left them"""
    assert R.ITEM_ROWS == const("ITEM_ROWS") == const("QUEUE") and R.WINDOW == const("WINDOW")
    fb, ho = tb.crafted([(2600, tb.random_moves(2600, 1500, 12, 12, 11)), (300, tb.random_moves(300, 120, 12, 12, 12))])
    mv = scenario_moves(fb, ho, 0)
    assert len(mv) == 1620 > 1280
    for caps in ({"inbound": 1}, {"inbound": 3, "outbound": 2}, {"outbound": 1}, {"inbound": 10 ** 6}):
        want = check(fb, ho, None, caps, ("beyond the queue", caps), solve_records=False)
    # some node's word is carried over a tile boundary: a move of the second tile lands beyond round 0 because of the first tile
    ro = rounds_ref(fb, ho, [0], {"inbound": 1})[0].round_of
    assert min(ro[1100:]) > 0


def test_more_rounds_than_the_window():
    """1,100 moves that all bring a replica to node 11 under cap_inbound 1: 1,100 rounds, more than the window of round counters,
    so the scenario is walked twice; records, maxima and first moves of both windows, and strides that cut inside either"""
    rows = list(range(0, 2400, 2))[:1100]
    moved = {p: [p % 11, (p + 1) % 11, 11] for p in rows}
    fb, ho = tb.crafted([(2400, moved)], N=12, n_cur=11)
    mv = scenario_moves(fb, ho, 0)
    assert len(mv) == 1100 and all(m[2] == (11,) for m in mv)
    caps = {"inbound": 1}
    want = check(fb, ho, [0, 0], caps, "two windows", solve_records=False)
    assert want[0].record["n_rounds"] == 1100 > const("WINDOW") and want[0].round_of == list(range(1100))
    for rs in (1100, 1099, 1025, 1024, 1023, 0):
        check(fb, ho, [0], caps, ("two windows, round stride", rs), round_stride=rs, move_stride=1100 if rs else 0, solve_records=False)
    # two moves a round: 550 rounds, one walk; the maxima are the window's
    want = check(fb, ho, [0], {"inbound": 2}, "one window", solve_records=False)
    assert want[0].record["n_rounds"] == 550 and want[0].record["max_round_moves"] == 2


@pytest.mark.parametrize("run", CC.runs(CC.ROUND_CASES), ids=CC.run_id)
def test_crafted_case(run):
    """every case of tests/crafted_cases.py (the MI355X runs them too: tests/test_rounds_crafted_gpu.py) under each of its caps and
    strides, on int32 and 16-bit cells; the case's own claims about what the checker shows are held first (Case.wants)"""
    name, cells16 = run
    case = CC.rounds_case(name)
    fb, ho, cur16 = case.tables(cells16)
    kw = dict(cells16=True, cur16=cur16) if cells16 else {}
    for caps, w in zip(case.caps, case.wants(cells16)):
        for rs, ms in case.strides_for(w):
            check(fb, ho, case.select, caps, (name, caps, cells16, rs, ms), round_stride=rs, move_stride=ms, solve_records=False,
                  want=case.listed(w), **kw)


@pytest.mark.parametrize("n", [R.WINDOW, R.WINDOW + 1, 2 * R.WINDOW, 2 * R.WINDOW + 1])
def test_one_walk_per_window_of_rounds(n):
    """a scenario is walked once per window of rounds its schedule has and no more often: exactly KAS_ROUND_WINDOW rounds are one
    walk, one more round a second.  A walk runs through the same wave collectives whatever the caps, so the walks of a call are
    its collectives over those of a call whose cap nobody reaches (one round, one walk).  (An extra walk finds no round of its
    window and writes nothing: only its time shows.)"""
    case = CC.rounds_case("window_%d" % n)
    assert case.wants(False)[0].record["n_rounds"] == n
    one = emu(case.fb, case.ho, [0], {"inbound": 10 ** 6}, 0, 0)[3]["collectives"]
    got = emu(case.fb, case.ho, [0], {"inbound": 1}, 0, 0)[3]["collectives"]
    assert one > 0 and got == -(-n // R.WINDOW) * one, (n, got, one)


def test_any_lds_fill():
    fb, ho, _ = solved("beyond_the_table")
    for fill in (0xCDCDCDCD, tb.STALE_ID, 0, 0xFFFFFFFF, 0x00010001):
        check(fb, ho, None, {"inbound": 1, "outbound": 1}, ("LDS fill", fill), lds_fill=fill)


def test_listing_and_strides():
    fb, ho, _ = solved("degenerate")                                         # scenario 1 has no topics: no moves
    caps = {"inbound": 1}
    want = check(fb, ho, [0, -1, 1, 0, 2, -1], caps, "listing")
    assert want[1] is None and want[2].record["n_rounds"] == 0 and want[0].record == want[3].record
    nr, nm = want[0].record["n_rounds"], want[0].record["n_moves"]
    assert nr >= 3 and nm > nr
    check(fb, ho, [0, 0], caps, "strides exactly the counts", round_stride=nr, move_stride=nm)
    check(fb, ho, [0, 0], caps, "strides one less: the guard stays", round_stride=nr - 1, move_stride=nm - 1)
    check(fb, ho, [0, 0], caps, "records only", round_stride=nr, move_stride=0)
    check(fb, ho, [0, 0], caps, "round_of only", round_stride=0, move_stride=nm)
    # counts only: both strides 0 with NULL arrays
    rc, err, scen, _, _, _ = emu_rc(fb, ho, [0, -1], caps, 0, 0, null_arrays=True)
    assert rc == 0, err
    assert_same_rounds(rounds_ref(fb, ho, [0, -1], caps), scen, np.zeros(0, abi.MOVE_ROUND_DTYPE), 0, np.zeros(0, np.int32), 0)
    # the same inputs give the same bytes
    a = emu(fb, ho, [0, 2], caps, nr + 1, nm + 1)
    b = emu(fb, ho, [0, 2], caps, nr + 1, nm + 1)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:3], b[:3]))


def test_chaos_schedule():
    """the wavefronts released at random (KAS_EMU_CHAOS): the barriers still meet, the records are the same"""
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_rounds_cpu as t\n"
            "fb, ho = t.tb.crafted([(1100, t.tb.random_moves(1100, 600, 12, 12, 4)), (200, t.tb.random_moves(200, 90, 12, 12, 8))])\n"
            "for caps in ({'inbound': 1}, {'inbound': 3, 'outbound': 2}):\n"
            "    t.check(fb, ho, [0, -1, 0], caps, ('chaos', caps), solve_records=False)\n"
            "fb, ho, _ = t.solved('widths_4_5')\n"
            "t.check(fb, ho, None, {'outbound': 1}, 'chaos, lists 5 wide')\n" % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, KAS_EMU_CHAOS="7"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr


# ---- refusals, the node limit, the planner ----------------------------------------------------------------------------------
def test_refusals_in_order():
    fb, ho, _ = solved("degenerate")
    S = fb.n_scenarios
    ok = {"inbound": 1}
    scen = np.zeros(4, abi.SCENARIO_ROUNDS_DTYPE)
    recs = np.zeros(64, abi.MOVE_ROUND_DTYPE)
    rof = np.zeros(64, np.int32)

    def call(spec=None, out=None, select=(0,)):
        rc, err, *_ = emu_rc(fb, ho, list(select), ok, 4, 4, spec=spec, raw_out=out)
        return rc, err

    good = abi.Rounds(scen.ctypes.data, recs.ctypes.data, 4, rof.ctypes.data, 4)
    wrong = abi.Rounds(None, None, -1, None, -1)                                 # everything behind the spec is wrong too
    for bad, text in ((abi.RoundSpec(-1, 0, 0, 0), "negative cap"), (abi.RoundSpec(0, -1, 0, 0), "negative cap"), (abi.RoundSpec(0, 0, 0, 0), "no cap"),
                      (abi.RoundSpec(1, 0, 1, 0), "policy"), (abi.RoundSpec(1, 0, 0, 7), "reserved")):
        rc, err = call(spec=bad, out=wrong, select=(S,))
        assert rc == E_INVALID and "kas_round_spec" in err and text in err, (rc, err)
    for o in (wrong, abi.Rounds(None, None, 4, None, -1)):
        rc, err = call(out=o, select=(S,))
        assert rc == E_INVALID and "negative stride" in err
    for o in (abi.Rounds(None, recs.ctypes.data + 1, 4, rof.ctypes.data, 4), abi.Rounds(scen.ctypes.data + 2, None, 4, rof.ctypes.data, 4),
              abi.Rounds(scen.ctypes.data + 2, recs.ctypes.data, 4, None, 4)):
        rc, err = call(out=o, select=(S,))
        assert rc == E_INVALID and "NULL" in err
    for o in (abi.Rounds(scen.ctypes.data + 2, recs.ctypes.data, 4, rof.ctypes.data, 4), abi.Rounds(scen.ctypes.data, recs.ctypes.data + 1, 4, rof.ctypes.data, 4),
              abi.Rounds(scen.ctypes.data, recs.ctypes.data, 4, rof.ctypes.data + 2, 4)):
        rc, err = call(out=o, select=(S,))
        assert rc == E_INVALID and "aligned" in err
    for sel in ((S,), (-2,), (0, S + 5)):
        rc, err = call(out=good, select=sel)
        assert rc == E_INVALID and "out of range" in err
    # the room, each stride on its own
    rc, err = call(out=abi.Rounds(scen.ctypes.data, recs.ctypes.data, (1 << 31) // 16 + 1, rof.ctypes.data, 4), select=(0,))
    assert rc == E_UNSUPPORTED and "round_stride x 16" in err
    rc, err = call(out=abi.Rounds(scen.ctypes.data, recs.ctypes.data, 4, rof.ctypes.data, (1 << 31) // 4 // 2 + 1), select=(0, 1))
    assert rc == E_UNSUPPORTED and "move_stride x 4" in err
    rc, err = call(out=abi.Rounds(scen.ctypes.data, recs.ctypes.data, (1 << 31) // 16 + 1, rof.ctypes.data, (1 << 31) // 4 + 1), select=(0,))
    assert rc == E_UNSUPPORTED and "round_stride x 16" in err
    assert call(out=good)[0] == 0


def test_node_limit():
    """KAS_ROUND_NODE_LIMIT is what the widest kernel's LDS layout leaves; a listed scenario above it is refused before the room is
    looked at, an unlisted one is not"""
    L = _emu_lib()
    limit = const("NODE_LIMIT")
    assert limit == abi.KAS_ROUND_NODE_LIMIT == int(re.search(r"#define KAS_ROUND_NODE_LIMIT (\d+)", open(HEADER).read()).group(1))
    lay = (C.c_int32 * 6)()
    for W in (3, 5, 8):
        for c16 in (0, 1):
            L.kas_emu_rounds_lds(limit, W, c16, lay)
            assert lay[5] <= 160 * 1024 and lay[0] >= 8 * limit and lay[1] >= lay[0] + (0 if c16 else 4 * limit)
            assert lay[2] == lay[1] + 256 and lay[3] - lay[2] >= 4 * W * const("QUEUE") and lay[4] == lay[3] + 8 * const("QUEUE")
            assert lay[5] == lay[4] + 12 * const("WINDOW")
    # 12 bytes a node (two 32-bit words, 4 bytes of lookup) beside the queue of lists 8 wide, the window, the misc words and the slack
    assert limit == (160 * 1024 - const("QUEUE") * (4 * 8 + 8) - 12 * const("WINDOW") - 256 - 32) // 12
    big = Scenario(list(range(limit + 1)), {}, [Topic("t", {0: [0, 1, 2]}, 3)])
    small = scenario(5, 30, 5, [T(100)], remove=[4])
    fb = flatten([small, big])
    from kafka_assigner_amd.flatten import host_tables
    _, ho = host_tables(fb)
    ho.out[:fb.cur.size] = fb.cur[:ho.out.size] if ho.out.size <= fb.cur.size else np.resize(fb.cur, ho.out.size)
    rc, err, *_ = emu_rc(fb, ho, [0, 1], {"inbound": 1}, (1 << 31) // 16, 2)
    assert rc == E_UNSUPPORTED and "KAS_ROUND_NODE_LIMIT" in err
    rc, err, *_ = emu_rc(fb, ho, None, {"inbound": 1}, 2, 2)
    assert rc == E_UNSUPPORTED and "KAS_ROUND_NODE_LIMIT" in err
    rc, err, *_ = emu_rc(fb, ho, [0, -1], {"inbound": 1}, 2, 2)
    assert rc == 0, err


def test_caps_against_the_round_words():
    """a node's word gives the round the bits that hold the scenario's rows and `used` the rest: 70,000 rows take 17 bits, so a cap
    from 2^15 up to the row count is refused, behind the node limit and in front of the room; a cap above the rows never binds and
    is served, and the same cap on a scenario of fewer rows is too"""
    P = 70000
    big = Scenario(list(range(12)), {}, [Topic("t", {p: [p % 12, (p + 1) % 12, (p + 2) % 12] for p in range(P)}, 3)])
    small = scenario(5, 30, 5, [T(100)], remove=[4])
    fb = flatten([big, small])
    scen = np.zeros(4, abi.SCENARIO_ROUNDS_DTYPE)
    out = abi.Rounds(scen.ctypes.data, None, 0, None, 0)
    for cap, ok in ((1, True), (2 ** 15 - 1, True), (2 ** 15, False), (P, False), (P + 1, True), (10 ** 6, True)):
        for caps in ({"inbound": cap}, {"inbound": 1, "outbound": cap}):
            rc, err, *_ = _plan(fb, 2, [0, 1], abi.round_spec(caps), out)
            assert (rc == 0) == ok and (ok or (rc == E_UNSUPPORTED and "round words" in err)), (caps, rc, err)
    assert _plan(fb, 2, [1, -1], abi.round_spec({"inbound": 2 ** 15}), out)[0] == 0          # the big scenario is not listed
    rc, err, *_ = _plan(fb, 2, [0], abi.round_spec({"inbound": 2 ** 15}), abi.Rounds(scen.ctypes.data, scen.ctypes.data, (1 << 31) // 16 + 1, None, 0))
    assert rc == E_UNSUPPORTED and "round words" in err                                       # in front of the room


def _plan(fb, kind, select, spec, out, cells16=False, ranges=0):
    L = _emu_lib()
    bd = batch_desc(fb)
    if cells16:
        bd.node_id = None
    lens = (C.c_int64 * 4)(int(fb.cur.size), int(fb.out_len), int(fb.aux.size), int(fb.ctx.size))
    head = (C.c_int64 * 4)()
    by = (C.c_int64 * const("HB_BUFFERS"))()
    err = C.create_string_buffer(512)
    sel = None if select is None else np.ascontiguousarray(select, dtype=np.int32)
    rc = L.kas_emu_rounds_host_call(C.byref(bd), lens, int(cells16), kind, None if sel is None else sel.ctypes.data, -1 if sel is None else int(sel.size),
                                    C.addressof(spec) if spec is not None else None, C.addressof(out) if out is not None else None, ranges, head, by,
                                    err, 512)
    return rc, err.value.decode(), list(head), list(by)


def test_planner_bytes():
    """the output buffers of a rounds call lie behind KAS_HB_FINAL, its inputs where a batches call puts them; a plain solve and a
    batches call plan what they planned before the rounds inputs existed (the batches driver, which knows nothing of them, agrees)"""
    fb, ho, _ = solved("mixed7")
    S, T_ = fb.n_scenarios, fb.n_topics
    scen = np.zeros(8, abi.SCENARIO_ROUNDS_DTYPE)
    recs = np.zeros(64, abi.MOVE_ROUND_DTYPE)
    rof = np.zeros(64, np.int32)
    spec = abi.round_spec({"inbound": 5})
    out = abi.Rounds(scen.ctypes.data, recs.ctypes.data, 7, rof.ctypes.data, 9)
    final, total = const("HB_FINAL"), const("HB_BUFFERS")
    assert total == final + 3 and final == tb.const("HB_FINAL")
    rc, err, head, by = _plan(fb, 2, [0, -1, 2], spec, out)
    assert rc == 0, err
    assert head[:2] == [3, max(int(fb.scen["n_nodes"][0]), int(fb.scen["n_nodes"][2]))]
    assert by[const("BT_SDESC")] == 32 * (S + 1) and by[const("BT_NODE_ID")] == 4 * (fb.node_id.size + 1) and by[const("BT_SELECT")] == 4 * 4
    assert by[const("RD_SCEN")] == 32 * 4 and by[const("RD_ROUNDS")] == 16 * (3 * 7 + 1) and by[const("RD_OF")] == 4 * (3 * 9 + 1)
    assert by[const("MV_SCEN")] == 32 * (S + 1) and by[const("MV_SEGS")] == 56 * (T_ + 1)
    assert by[tb.const("BT_SCEN")] == 0 and by[tb.const("BT_BATCHES")] == 0
    rc, err, head, by_all = _plan(fb, 2, None, spec, abi.Rounds(scen.ctypes.data, None, 0, None, 0))
    assert rc == 0 and head[0] == S and by_all[const("RD_ROUNDS")] == 16 and by_all[const("RD_OF")] == 4
    # a plain solve: nothing behind KAS_HB_EVERY; everything else as in the rounds call
    rc, err, _, plain = _plan(fb, 0, [], None, None)
    assert rc == 0, err
    every = tb.const("HB_EVERY")
    assert plain[every:] == [0] * (total - every)
    same = [i for i in range(every) if i not in (const("MV_SCEN"), const("MV_SEGS"))]
    assert [plain[i] for i in same] == [by[i] for i in same]
    # ... and it and a batches call are what the batches driver plans
    assert tb._plan(fb, [], None, None)[3] == plain[:final]
    bspec, bscen = abi.batch_spec({"inbound": 5}), np.zeros(8, abi.SCENARIO_BATCHES_DTYPE)
    bout = abi.Batches(bscen.ctypes.data, None, 0)
    rc, err, _, bt = _plan(fb, 1, [0, -1, 2], bspec, bout)
    assert rc == 0 and bt[final:] == [0, 0, 0] and bt[:final] == tb._plan(fb, [0, -1, 2], bspec, bout)[3]
    # a 16-bit call solved on its own cells uploads no node ids
    fb3 = flatten([scenario(5, 30, 5, [T(100)], remove=[4])])
    rc, err, head, by16 = _plan(fb3, 2, None, spec, out, cells16=True)
    assert rc == 0, err
    assert by16[const("BT_NODE_ID")] == (0 if head[3] else 4 * (fb3.node_id.size + 1))
    # refusals of the planner come in the documented order, behind the solve's own
    rc, err, *_ = _plan(fb, 2, [S], abi.RoundSpec(0, 0, 0, 0), out)
    assert rc == E_INVALID and "kas_round_spec" in err
    rc, err, *_ = _plan(fb, 2, [S], spec, out)
    assert rc == E_INVALID and "out of range" in err


def test_moves_and_choose_calls_plan_the_bytes_they_planned():
    """the moves driver and the choose driver know nothing of the rounds inputs: what they plan is unchanged by a rounds call
    planned in between (tests/test_moves_cpu.py and test_choose_cpu.py pin the figures themselves)"""
    fb, ho, _ = solved("mixed7")
    before = tb._plan(fb, [], None, None)
    scen = np.zeros(8, abi.SCENARIO_ROUNDS_DTYPE)
    assert _plan(fb, 2, [0, 1, -1], abi.round_spec({"outbound": 1}), abi.Rounds(scen.ctypes.data, None, 0, None, 0))[0] == 0
    assert tb._plan(fb, [], None, None) == before


def test_header_and_library():
    """the header declares the four entries and the records; the library exports them (where it is built)"""
    text = open(HEADER).read()
    for name in abi.ROUNDS_ENTRIES:
        assert re.search(r"\bint %s\(" % name, text), name
        assert name in native.SYMBOLS
    for name in ("kas_round_spec", "kas_move_round", "kas_scenario_rounds", "kas_rounds", "KAS_ROUNDS_MONOTONE", "KAS_ROUND_NODE_LIMIT"):
        assert name in text
    assert "#define KAS_ABI_VERSION 6" in text
    for f in abi.MOVE_ROUND_FIELDS + abi.SCENARIO_ROUNDS_FIELDS + ("round_stride", "move_stride", "round_of", "cap_inbound", "cap_outbound", "policy"):
        assert re.search(r"\b%s\b" % f, text), f
    lib = os.path.join(CSRC, "libkas_hip.so")
    if os.path.exists(lib):
        syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
        for name in abi.ROUNDS_ENTRIES:
            assert re.search(r"\bT %s\b" % name, syms), name


def test_round_spec_mirror():
    sp = abi.round_spec({"inbound": 5})
    assert (sp.cap_inbound, sp.cap_outbound, sp.policy, sp.reserved) == (5, 0, abi.KAS_ROUNDS_MONOTONE, 0)
    assert abi.round_spec(sp) is sp
    with pytest.raises(ValueError):
        abi.round_spec({"inbound": 1, "max_moves": 2})


# ---- WhatIf, without a GPU ----------------------------------------------------------------------------------------------------
def test_whatif_argument_handling():
    """rounds= / round_room= are checked before anything is solved; rounds() and reassignment_rounds() over hand-made records"""
    from kafka_assigner_amd.whatif import Variant, VariantResult, WhatIf
    plan = WhatIf({b: "r%d" % (b % 3) for b in range(6)}, {"a": {0: [0, 1, 2], 1: [1, 2, 3]}, "b": {0: [2, 3, 4], 5: [3, 4, 5]}})
    vs = [Variant(remove=[5])]
    for call in (plan.solve, plan.best, plan.front):
        for bad in ({"inbound": -1}, {}, {"inbound": 0, "outbound": 0}, {"inbund": 3}, {"inbound": 1, "policy": 1}):
            with pytest.raises(ValueError):
                call(vs, rounds=bad)
        with pytest.raises(ValueError):
            call(vs, rounds={"inbound": 1}, round_room=-1)
    with pytest.raises(ValueError):
        plan.solve(vs, rounds={"inbound": 1}, solve_fn=lambda fb: None)
    R_, L_, O_ = abi.KAS_MOVE_REPLICAS, abi.KAS_MOVE_LEADER, abi.KAS_MOVE_ORDER
    recs = np.array([(0, 0, R_ | L_, 3, 1, 1, 0), (0, 1, L_, 3, 0, 0, 3), (1, 0, R_, 3, 1, 1, 6), (1, 5, R_ | O_, 3, 1, 1, 9)], abi.MOVE_DTYPE)
    cells = np.array([4, 1, 2, 2, 1, 3, 0, 3, 4, 4, 3, 5], np.int32)
    rd = np.array([(2, 2, 0, 0), (1, 1, 1, 0)], abi.MOVE_ROUND_DTYPE)
    r = VariantResult(label="x", status=0, fail_topic=None, fail_partition=-1, moved_replicas=3, moved_partitions=3, digest=0, _plan=plan,
                      _moves=(recs, cells), _moves_mask=7, n_rounds=2, round_moves=3, _rounds=rd, _round_of=np.array([0, 1, 0], np.int32))
    assert r.rounds() == [dict(n_moves=2, replicas=2, first_move=0, moves=[0, 2]), dict(n_moves=1, replicas=1, first_move=1, moves=[1])]
    objs = r.reassignment_rounds()
    assert [[(p["topic"], p["partition"]) for p in o["partitions"]] for o in objs] == [[("a", 0), ("a", 1), ("b", 5)], [("b", 0)]]   # the leader-only row: round 0
    key = lambda p: (p["topic"], p["partition"])
    assert sorted((p for o in objs for p in o["partitions"]), key=key) == sorted(r.reassignment()["partitions"], key=key)
    assert [len(o["partitions"]) for o in r.reassignment_rounds(kinds=("replicas",))] == [2, 1]
    assert [len(o["partitions"]) for o in r.reassignment_rounds(max_moves=2)] == [2, 1, 1]
    assert [len(o["partitions"]) for o in r.reassignment_rounds(max_moves=1)] == [1, 1, 1, 1]
    with pytest.raises(ValueError):
        r.reassignment_rounds(max_moves=-1)
    r._moves_mask = L_                                                           # a list without the replica moves cannot be cut into rounds
    with pytest.raises(ValueError):
        r.reassignment_rounds()
    r._moves_mask = 7
    r.n_rounds = 3                                                               # more rounds than records: the room was too small
    for f in (r.rounds, r.reassignment_rounds):
        with pytest.raises(ValueError):
            f()
    bare = VariantResult(label="x", status=0, fail_topic=None, fail_partition=-1, moved_replicas=0, moved_partitions=0, digest=0, _plan=plan)
    for f in (bare.rounds, bare.reassignment_rounds):
        with pytest.raises(ValueError):
            f()
    assert bare.n_rounds is None


# ---- the quality guards over the what-if batch (the checker alone) ------------------------------------------------------------------
@pytest.fixture(scope="module")
def whatif_lists():
    """the move lists of the what-if batch's variants that solve"""
    from test_choose_cpu import whatif_solved
    _, _, fb, ho, _ = whatif_solved()
    ok = np.nonzero(ho.scenario_results["status"][:fb.n_scenarios] == abi.KAS_OK)[0]
    return fb.n_scenarios, [scenario_moves(fb, ho, int(s)) for s in ok]


def test_guard_inbound_5(whatif_lists):
    """{"inbound": 5}: every variant that solves takes fewer rounds than consecutive batches, and at least 90 of the 184 meet the
    lower bound; the schedule respects the caps, and so does a true first fit"""
    S, lists = whatif_lists
    assert (S, len(lists)) == (302, 184)
    caps = {"inbound": 5}
    at_bound = 0
    for mv in lists:
        ro, _, _ = monotone(mv, caps)
        n_rounds, n_batches, lb = 1 + max(ro), cut(mv, caps)[0]["n_batches"], lower_bound(mv, caps)
        assert lb <= n_rounds < n_batches, (n_rounds, n_batches, lb)
        R.check_caps(mv, ro, caps)
        at_bound += n_rounds == lb
    assert at_bound >= 90, at_bound
    for mv in lists[:8]:
        ff = first_fit(mv, caps)
        R.check_caps(mv, ff, caps)
        assert lower_bound(mv, caps) <= 1 + max(ff)


def test_guard_outbound_1(whatif_lists):
    """{"outbound": 1}: all 184 meet the lower bound"""
    _, lists = whatif_lists
    caps = {"outbound": 1}
    for mv in lists:
        ro, by_in, _ = monotone(mv, caps)
        assert 1 + max(ro) == lower_bound(mv, caps) and by_in == 0

"""The topic pass (include/kas_abi.h: kas_topic_impact / kas_scenario_topic_impact) without a GPU.

- The kernel bodies (kafka-assigner_amd/csrc/kas_topics_body.h) compiled with g++ against tests/emu/kas_wave.h and stepped on CPU
  fibers (tests/emu/topic_driver.cpp) over oracle-produced out tables, against the checker (tests/topic_ref.py): the row loop's
  step boundary, every width class, both id lookups and the search's bound, degenerate scenarios, two scenarios on one node
  range, a cut topic (FLUSH) beside uncut ones (DIRECT), OK / failed / skipped topics in one scenario, a scenario beyond the LDS
  (GLOBAL), 16-bit cells, and the FLUSH and GLOBAL paths forced onto a small batch.
- Identities against the impact records, the refusals in their order, the host call planner's bytes, the ABI.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from impact_batches import T, scenario, solved
from impact_ref import impact_ref
from kafka_assigner_amd import abi, native
from kafka_assigner_amd import generator as G
from kafka_assigner_amd.flatten import Scenario, Topic, batch_desc, flatten, index_form, to_cells16
from oracle_lib import oracle_solve
from topic_ref import assert_same_topics, check_topic_identities, topic_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "kafka-assigner_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "kas_abi.h")
E_INVALID, E_UNSUPPORTED = abi.KAS_E_INVALID_ARG, abi.KAS_E_UNSUPPORTED
DIRECT, FLUSH, GLOBAL = 0, 1, 2                      # KAS_TOPIC_DIRECT / _FLUSH / _GLOBAL (kas_topics.h)
_LIB = None


# ---- the emulator ---------------------------------------------------------------------------------------------------------
def _emu_lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    so = os.path.join(EMU, "libkas_emu_topics.so")
    srcs = [os.path.join(EMU, f) for f in ("topic_driver.cpp", "emu_driver.cpp")]
    deps = srcs + [os.path.join(EMU, "kas_wave.h"), HEADER] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        tmp = so + ".tmp%d" % os.getpid()
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unused-parameter", "-Wno-unknown-pragmas",
                               "-I" + os.path.join(ROOT, "tests"), "-I" + CSRC, "-I" + os.path.join(ROOT, "include"),
                               "-o", tmp] + srcs)
        os.replace(tmp, so)
    L = C.CDLL(so)
    L.kas_emu_topics.restype = C.c_int
    L.kas_emu_topics.argtypes = [C.POINTER(abi.BatchDesc), C.POINTER(abi.Tables), C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.c_char_p, C.c_int]
    L.kas_emu_topic_host_call.restype = C.c_int
    L.kas_emu_topic_host_call.argtypes = [C.POINTER(abi.BatchDesc), C.POINTER(C.c_int64), C.c_int32, C.c_int, C.c_int, C.c_int, C.c_int,
                                          C.c_uint, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_char_p, C.c_int]
    L.kas_emu_topics_lds_fill.restype = None
    L.kas_emu_topics_lds_fill.argtypes = [C.c_uint32]
    L.kas_emu_topic_buffers.restype = C.c_int
    L.kas_emu_topic_buffers.argtypes = [C.c_int]
    _LIB = L
    return L


def emu_topics_rc(fb, ho, cells16=False, cur16=None, rows_per_item=0, node_cap=-1):
    """kas_emu_topics over the tables a solve left in `ho`: (rc, error text, (topics, scenarios), info, work list)."""
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
    topics = np.full(max(fb.n_topics, 1), -7, dtype=abi.TOPIC_IMPACT_DTYPE)                 # (every record must be written)
    scen = np.full(max(fb.n_scenarios, 1), -7, dtype=abi.SCENARIO_TOPIC_IMPACT_DTYPE)
    cap = 4096
    items = np.zeros((cap, 6), dtype=np.int32)
    info = (C.c_int32 * 8)()
    err = C.create_string_buffer(512)
    rc = L.kas_emu_topics(C.byref(bd), C.byref(t), int(cells16), int(node_cap), int(rows_per_item), topics.ctypes.data, scen.ctypes.data,
                          items.ctypes.data, cap, info, err, 512)
    names = ("items", "merge", "flush", "global", "node_cap")
    d = dict(zip(names, list(info)[:5]))
    d["region_ints"] = (int(info[5]) & 0xffffffff) | (int(info[6]) << 32)
    work = [dict(zip(("scen", "topic", "row_lo", "row_hi", "mode"), [int(v) for v in row[:5]])) for row in items[:min(d["items"], cap)]]
    return rc, err.value.decode(), (topics[:fb.n_topics], scen[:fb.n_scenarios]), d, work


def emu_topics(fb, ho, **kw):
    rc, err, got, info, work = emu_topics_rc(fb, ho, **kw)
    assert rc == 0, (rc, err)
    return got, info, work


def solved16(fb):
    """The oracle's solve of the batch's 16-bit form: (HostOutputs with uint16 out, cur16)."""
    ho = oracle_solve(index_form(fb))
    ho.out = np.where(ho.out < 0, abi.KAS_CELL16_NONE, ho.out).astype(np.uint16)
    return ho, to_cells16(fb)


def modes_by_topic(work):
    out = {}
    for it in work:
        out.setdefault(it["topic"], []).append(it["mode"])
    return out


# ---- the guard --------------------------------------------------------------------------------------------------------------
def assert_exercises_topics(fb, ho, want, not_ok_share=0.25):
    """A condition on the batch, from the oracle's solve and the checker's records alone: the test that calls this compares
    counted rows, not zeros.  Over the batch, leaders_moved, departed_replicas, max_inbound and a non-zero replica spread occur in
    some topic record; at most `not_ok_share` of the topics are not KAS_OK."""
    topics, _ = want
    status = ho.topic_results["status"][:fb.n_topics]
    assert fb.n_topics > 0 and (status != abi.KAS_OK).sum() <= not_ok_share * fb.n_topics, ("too few topics solve", status.tolist())
    for f in ("leaders_moved", "departed_replicas", "max_inbound"):
        assert int(topics[f].max()) > 0, f
    assert int((topics["max_replicas_after"] - topics["min_replicas_after"]).max()) > 0, "no topic with a replica spread"


# ---- batches of this file (beside impact_batches.BATCHES, whose oracle solves are shared) ------------------------------------
def _batch_a():
    """a cut topic beside uncut ones"""
    return flatten([scenario(2, 66, 6, [T(4097, exact=True, balanced=True, noise=2), T(300), T(513, ragged=0.1)], remove=[1, 13, 40])])


def _batch_b():
    """OK, then failed, then skipped, in one scenario"""
    return flatten([scenario(3, 60, 6, [T(300), T(10000, exact=True, balanced=True, noise=2), T(200, parts=True)], remove=[1, 13, 40])])


def _batch_c():
    """11,000 brokers: beyond the LDS for every lookup"""
    N = 11000
    brokers = list(range(N))
    topics = []
    for k, P in enumerate((600, 250, 100)):
        cur = G.random_assignment(11 + k, P, N + 50, 20, 3)
        topics.append(Topic("big%d" % k, {p: cur[p].tolist() for p in range(P)}, 3))
    return flatten([Scenario(brokers, {b: "r%d" % (b % 20) for b in brokers}, topics)])


OWN = {"A": _batch_a, "B": _batch_b, "C": _batch_c}
_OWN = {}


def own(name):
    """(fb, ho, impact_ref's records, topic_ref's records) of a batch of this file, built and solved by the oracle once"""
    if name not in _OWN:
        fb = OWN[name]()
        ho = oracle_solve(fb)
        want = topic_ref(fb, ho)
        assert_exercises_topics(fb, ho, want, not_ok_share=0.67 if name == "B" else 0.25)   # (B: the declared exception)
        _OWN[name] = (fb, ho, impact_ref(fb, ho), want)
    return _OWN[name]


_SHARED = {}


def shared(name):
    """the same for a named batch of impact_batches (its guard, assert_exercises, has passed there)"""
    if name not in _SHARED:
        fb, ho, imp = solved(name)
        want = topic_ref(fb, ho)
        assert_exercises_topics(fb, ho, want)
        _SHARED[name] = (fb, ho, imp, want)
    return _SHARED[name]


def _check(fb, ho, imp, want, what, cells=(False,), rows=(0,), caps=(-1,)):
    """every combination on the emulator against the checker; the identities that tie the records to the impact records"""
    infos = []
    ho16 = cur16 = None
    for c16 in cells:
        if c16 and ho16 is None:
            ho16, cur16 = solved16(fb)
            assert_same_topics(want, topic_ref(fb, ho16, cells16=True, cur16=cur16), f"{what}: checker, 16-bit cells")
        for r in rows:
            for cap in caps:
                got, info, work = emu_topics(fb, ho16 if c16 else ho, cells16=c16, cur16=cur16 if c16 else None, rows_per_item=r, node_cap=cap)
                assert_same_topics(want, got, f"{what}: cells16={c16}, rows per item {r}, node cap {cap}")
                infos.append((info, work))
    check_topic_identities(fb, ho, imp, want)
    return infos


# ---- the cases ------------------------------------------------------------------------------------------------------------
def test_row_step_boundary():
    """P = 1, 511, 512, 513, 1025 around the row loop's step of 2 x 256 rows; items of 512, 513 and 514 rows"""
    fb, ho, imp, want = shared("row_counts")
    _check(fb, ho, imp, want, "row_counts", cells=(False, True), rows=(0, 97, 512, 513, 514), caps=(-1, 0))
    # five single-topic scenarios: every topic record is its scenario's impact record
    for f in abi.TOPIC_IMPACT_FIELDS:
        assert want[0][f].tolist() == imp[1][f].tolist(), f


@pytest.mark.parametrize("name", ["mixed7", "mixed42"])
def test_merging_widths_2_and_3(name):
    fb, ho, imp, want = shared(name)
    _check(fb, ho, imp, want, name, cells=(False, True) if name == "mixed7" else (False,), rows=(0, 97), caps=(-1, 0))
    assert int(fb.scen["topic_count"].max()) >= 2 and int(want[1]["topics_ok"].max()) >= 2


@pytest.mark.parametrize("name", ["widths_4_5", "widths_6_8"])
def test_wider_instances(name):
    fb, ho, imp, want = shared(name)
    _check(fb, ho, imp, want, name, rows=(0, 97), caps=(-1, 0))


@pytest.mark.parametrize("name", ["sparse", "dense_and_sparse", "id_range_edge", "beyond_the_table"])
def test_both_lookups_and_the_search_bound(name):
    fb, ho, imp, want = shared(name)
    _check(fb, ho, imp, want, name, rows=(0, 97), caps=(-1, 0))


def test_a_stale_id_behind_the_sorted_ids_stays_departed():
    """beyond_the_table: the removed broker lies above every id of the set, so the search for its replicas ends one past the
    sorted ids; with that very id all over the LDS (what a workgroup before may have left) only the search's bound keeps such a
    replica departed"""
    from impact_batches import STALE_ID
    fb, ho, imp, want = shared("beyond_the_table")
    assert int(want[0]["departed_replicas"].sum()) > 0
    L = _emu_lib()
    L.kas_emu_topics_lds_fill(STALE_ID)
    try:
        for r in (0, 97):
            got, _, _ = emu_topics(fb, ho, rows_per_item=r)
            assert_same_topics(want, got, f"stale id in the LDS, rows per item {r}")
    finally:
        L.kas_emu_topics_lds_fill(0xCDCDCDCD)


def test_degenerate_scenarios():
    """a normal scenario, a scenario without topics (a zero summary) and one without brokers (its topic fails: a zero record)"""
    fb, ho, imp, want = shared("degenerate")
    assert fb.scen["topic_count"].tolist() == [3, 0, 1] and fb.scen["n_nodes"].tolist() == [29, 12, 0]
    _check(fb, ho, imp, want, "degenerate", cells=(False, True), rows=(0, 97), caps=(-1, 0))
    assert want[1]["topics_ok"].tolist() == [3, 0, 0]
    assert not any(int(want[0][f][3]) for f in abi.TOPIC_IMPACT_FIELDS)
    assert not any(int(want[1][f][s]) for f in abi.SCENARIO_TOPIC_FIELDS for s in (1, 2))


def test_two_scenarios_on_one_node_range():
    fb, ho, imp, want = shared("shared_node_range")
    assert int(fb.scen["node_off"][0]) == int(fb.scen["node_off"][1])
    _check(fb, ho, imp, want, "shared_node_range", cells=(False, True), rows=(0, 97), caps=(-1, 0))


@pytest.mark.parametrize("name,items", [("rows_4096", 1), ("rows_4097", 2), ("rows_10000", 3)])
def test_a_cut_topic(name, items):
    """one topic of one scenario, cut by the impact pass's rule into row ranges of 4096: FLUSH from two items on"""
    fb, ho, imp, want = shared(name)
    infos = _check(fb, ho, imp, want, name, cells=(False, True) if name == "rows_4097" else (False,))
    for info, work in infos:
        assert info["items"] == items and info["merge"] == (1 if items > 1 else 0)
        assert [w["mode"] for w in work] == [FLUSH if items > 1 else DIRECT] * items
        assert [w["row_hi"] - w["row_lo"] for w in work][:-1] == [4096] * (items - 1)


def test_batch_a_a_cut_topic_beside_uncut_ones():
    fb, ho, imp, want = own("A")
    assert ho.topic_results["status"][:3].tolist() == [abi.KAS_OK] * 3
    assert ho.topic_results["moved_replicas"][:3].tolist() == [648, 106, 191]
    infos = _check(fb, ho, imp, want, "batch A", cells=(False, True))
    for info, work in infos:
        assert modes_by_topic(work) == {0: [FLUSH, FLUSH], 1: [DIRECT], 2: [DIRECT]}
        assert info["merge"] == 1 and info["region_ints"] == 4 * 63 + 2
    assert want[1]["topics_ok"].tolist() == [3] and want[1]["max_topic_moved_replicas"].tolist() == [648]
    # forced: every topic cut, and every topic in global scratch
    _check(fb, ho, imp, want, "batch A, forced", rows=(97,), caps=(-1, 0))


def test_batch_b_ok_failed_and_skipped_topics_in_one_scenario():
    fb, ho, imp, want = own("B")
    assert ho.topic_results["status"][:3].tolist() == [abi.KAS_OK, abi.KAS_FAIL_UNASSIGNABLE, abi.KAS_SKIPPED]
    assert int(ho.topic_results["moved_replicas"][0]) == 94
    _check(fb, ho, imp, want, "batch B", cells=(False,), rows=(0, 97), caps=(-1, 0))
    for t in (1, 2):
        assert not any(int(want[0][f][t]) for f in abi.TOPIC_IMPACT_FIELDS), t
    assert int(want[1]["topics_ok"][0]) == 1 and int(want[1]["max_topic_moved_replicas"][0]) == 94
    # the failed topic is cut all the same (the work list does not know statuses): its merge workgroup writes the zeros
    _, info, work = emu_topics(fb, ho)
    assert modes_by_topic(work) == {0: [DIRECT], 1: [FLUSH, FLUSH, FLUSH], 2: [DIRECT]}


def test_batch_c_beyond_the_lds_for_every_lookup():
    fb, ho, imp, want = own("C")
    assert int(fb.scen["n_nodes"][0]) == 11000 and fb.topics["n_partitions"].tolist() == [600, 250, 100]
    assert ho.topic_results["status"][:3].tolist() == [abi.KAS_OK] * 3
    assert ho.topic_results["moved_replicas"][:3].tolist() == [166, 25, 9]
    infos = _check(fb, ho, imp, want, "batch C", cells=(False, True))
    for info, work in infos:                                     # (int32 cells: the direct table; 16-bit cells: no lookup at all)
        assert info["node_cap"] < 11000 and modes_by_topic(work) == {0: [GLOBAL], 1: [GLOBAL], 2: [GLOBAL]}
        assert info["global"] == 3 and info["merge"] == 3 and info["region_ints"] == 3 * (4 * 11000 + 2)
    assert int(want[1]["max_topic_replicas_after"][0]) >= 1 and int(want[0]["min_replicas_after"].max()) == 0


def test_forced_global_and_flush_equal_the_unforced_records():
    fb, ho, imp, want = shared("mixed7")
    plain, info0, work0 = emu_topics(fb, ho)
    assert {w["mode"] for w in work0} == {DIRECT} and info0["merge"] == 0
    glob, info1, work1 = emu_topics(fb, ho, node_cap=0)
    assert {w["mode"] for w in work1} == {GLOBAL} and info1["merge"] == fb.n_topics
    cut, info2, work2 = emu_topics(fb, ho, rows_per_item=97)
    assert FLUSH in {w["mode"] for w in work2} and info2["items"] > fb.n_topics
    both, _, work3 = emu_topics(fb, ho, rows_per_item=97, node_cap=0)
    assert {w["mode"] for w in work3} == {GLOBAL} and len(work3) == len(work2)
    for got, what in ((glob, "GLOBAL"), (cut, "FLUSH"), (both, "GLOBAL, cut")):
        assert_same_topics(plain, got, what)
    assert_same_topics(want, plain, "mixed7")


# ---- the planner: refusals and bytes ----------------------------------------------------------------------------------------
from test_racks_cpu import HOST_BUFS as RACK_HOST_BUFS, PARENT   # noqa: E402  (the names and the pinned bytes of the calls before)

HOST_BUFS = RACK_HOST_BUFS + ("tp_topics", "tp_scen")
MISSING = {"host_topics": 1, "topics": 2, "scenarios": 4}


def topic_host_call(fb, topics=True, impact=True, nodes=True, n_select=0, cells16=False, missing=()):
    """kas_plan_host_call for kas_solve_host_topic_impact (topics) or kas_solve_host_impact: (rc, {bytes by name, region_ints}, text)"""
    L = _emu_lib()
    assert L.kas_emu_topic_buffers(0) == len(HOST_BUFS) and L.kas_emu_topic_buffers(1) == len(RACK_HOST_BUFS)
    bd = batch_desc(fb)
    lens = (C.c_int64 * 4)(int(fb.cur.shape[0]), int(fb.out_len), int(fb.aux.shape[0]), int(fb.ctx.shape[0]))
    nbytes = (C.c_int64 * len(HOST_BUFS))()
    region = C.c_int64(0)
    err = C.create_string_buffer(512)
    rc = L.kas_emu_topic_host_call(C.byref(bd), lens, n_select, int(cells16), int(topics), int(impact), int(nodes),
                                   sum(MISSING[m] for m in missing), nbytes, C.byref(region), err, 512)
    if rc != 0:
        return rc, None, err.value.decode()
    return rc, dict(bytes=dict(zip(HOST_BUFS, [int(v) for v in nbytes])), region_ints=int(region.value)), ""


def _many_global_topics(n_topics):
    """batch C's scenario with its first topic descriptor repeated n_topics times: that many topics of an 11,000-broker
    scenario, every one of them counting in global scratch (descriptors only: nothing is solved)"""
    fb = own("C")[0]
    import copy
    big = copy.copy(fb)
    big.topics = np.repeat(fb.topics[:1], n_topics)
    big.scen = fb.scen.copy()
    big.scen["topic_count"][0] = n_topics
    return big


def test_refusals_in_their_order():
    fb = shared("mixed7")[0]
    assert topic_host_call(fb)[0] == 0
    for m in ("host_topics", "topics", "scenarios"):
        rc, _, err = topic_host_call(fb, missing=(m,))
        assert rc == E_INVALID and "kas_topic_impact_tables" in err, (m, rc, err)
    # the scratch limit: (4 N + 2) int32 per topic of an 11,000-broker scenario
    per_topic = 4 * (4 * 11000 + 2)
    fits = abi.KAS_TOPIC_SCRATCH_LIMIT // per_topic
    rc, plan, err = topic_host_call(_many_global_topics(fits), impact=False)
    assert rc == 0 and plan["region_ints"] * 4 == fits * per_topic <= abi.KAS_TOPIC_SCRATCH_LIMIT, (rc, err)
    over = _many_global_topics(fits + 1)
    rc, _, err = topic_host_call(over, impact=False)
    assert rc == E_UNSUPPORTED and "KAS_TOPIC_SCRATCH_LIMIT" in err, (rc, err)
    # ... behind the NULL arrays, and behind the impact call's own refusals
    rc, _, err = topic_host_call(over, impact=False, missing=("topics",))
    assert rc == E_INVALID and "kas_topic_impact_tables" in err, (rc, err)
    rc, _, err = topic_host_call(over, impact=True, nodes=True, missing=("host_topics",))
    assert rc == E_INVALID
    # the same batch without the topic pass is taken
    assert topic_host_call(over, topics=False)[0] == 0
    # batch C itself, three such topics, is far below the limit
    rc, plan, _ = topic_host_call(own("C")[0], impact=False)
    assert rc == 0 and plan["region_ints"] == 3 * (4 * 11000 + 2)


@pytest.mark.parametrize("cells16", [False, True], ids=["int32", "cells16"])
def test_planner_bytes(cells16):
    """the bytes of every existing call are what they were; the topic call adds its two buffers, and without host_impact the
    impact buffers are not this call's"""
    import emu_lib
    fb = shared("mixed42")[0]
    S, Tn = fb.n_scenarios, fb.n_topics
    for n_select in (-1, 0):
        rc, mine, err = topic_host_call(fb, topics=False, n_select=n_select, cells16=cells16)
        assert rc == 0, err
        assert [mine["bytes"][n] for n in emu_lib.HOST_BUFS] == PARENT[(cells16, n_select)]
        assert not any(mine["bytes"][n] for n in HOST_BUFS[len(emu_lib.HOST_BUFS):])           # nothing behind them, the new ids included
        rc, tp, err = topic_host_call(fb, n_select=n_select, cells16=cells16)
        assert rc == 0, err
        assert [tp["bytes"][n] for n in HOST_BUFS[:-2]] == [mine["bytes"][n] for n in HOST_BUFS[:-2]]
        assert tp["bytes"]["tp_topics"] == 32 * (Tn + 1) and tp["bytes"]["tp_scen"] == 64 * (S + 1)
        rc, no_nodes, err = topic_host_call(fb, nodes=False, n_select=n_select, cells16=cells16)
        assert rc == 0 and no_nodes["bytes"] == tp["bytes"], err                              # (the node records stay on the device)
        rc, bare, err = topic_host_call(fb, impact=False, n_select=n_select, cells16=cells16)
        assert rc == 0, err
        assert bare["bytes"]["imp_nodes"] == 0 and bare["bytes"]["imp_scen"] == 0
        assert {n: v for n, v in bare["bytes"].items() if not n.startswith("imp_")} == {n: v for n, v in tp["bytes"].items() if not n.startswith("imp_")}
        assert tp["region_ints"] == 0                                                          # (small scenarios, no topic cut)
    # the impact call still wants its node array
    assert topic_host_call(fb, topics=False, nodes=False)[0] == E_INVALID


# ---- ABI ------------------------------------------------------------------------------------------------------------------
def test_abi_declares_the_topic_entries_and_records(tmp_path):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(kas_[a-z_0-9]+)\s*\(", src))
    for name in abi.TOPIC_ENTRIES:
        assert name in declared and name in native.SYMBOLS, name
    assert re.search(r"#define KAS_ABI_VERSION (\d+)", src).group(1) == str(abi.KAS_ABI_VERSION) == "6"
    assert re.search(r"#define KAS_TOPIC_SCRATCH_LIMIT \((\d+)ll << (\d+)\)", src).groups() == ("256", "20")
    assert abi.KAS_TOPIC_SCRATCH_LIMIT == 256 << 20
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kas_abi.h"\n'
                     'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(kas_topic_impact), sizeof(kas_scenario_topic_impact), '
                     'sizeof(kas_topic_impact_tables), offsetof(kas_topic_impact, max_leaders_after), '
                     'offsetof(kas_scenario_topic_impact, max_topic_inbound), offsetof(kas_scenario_topic_impact, sum_topic_leader_spread), '
                     'offsetof(kas_scenario_topic_impact, reserved)); return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c11", "-I" + os.path.join(ROOT, "include"), str(probe), "-o", str(exe)])
    assert subprocess.check_output([str(exe)], text=True).split() == ["32", "64", "16", "28", "28", "56", "60"]
    # the topic record has kas_scenario_impact's eight fields, in its order
    assert abi.TOPIC_IMPACT_FIELDS == abi.SCENARIO_IMPACT_FIELDS
    assert [abi.TOPIC_IMPACT_DTYPE.fields[f][1] for f in abi.TOPIC_IMPACT_FIELDS] == [abi.SCENARIO_IMPACT_DTYPE.fields[f][1] for f in abi.TOPIC_IMPACT_FIELDS]
    assert [abi.SCENARIO_TOPIC_IMPACT_DTYPE.fields[f][1] for f in abi.SCENARIO_TOPIC_FIELDS] == [4 * i for i in range(15)]


def test_library_exports_the_topic_entries():
    from kafka_assigner_amd import build
    assert "kas_topics.hip" in build.SOURCES
    build.build()
    L = native.load()
    for name in abi.TOPIC_ENTRIES:
        assert hasattr(L, name), name
    assert L.kas_abi_version() == 6
    blob = open(build.LIB, "rb").read()
    for kernel in (b"kas_topic_item_kernel", b"kas_topic_merge_kernel", b"kas_topic_summary_kernel"):
        assert kernel in blob, kernel


def test_whatif_takes_topics_only_with_the_library_host_call():
    from kafka_assigner_amd.whatif import Variant, VariantResult, WhatIf
    w = WhatIf({0: "a", 1: "b", 2: "a", 3: "b"}, {"t": {0: [0, 1], 1: [2, 3]}})
    with pytest.raises(ValueError):
        w.solve([Variant()], topics=True, moves=("replicas",))
    with pytest.raises(ValueError):
        w.solve([Variant()], topics=True, solve_fn=lambda fb: None)
    r = VariantResult(label="", status=0, fail_topic=None, fail_partition=-1, moved_replicas=0, moved_partitions=0, digest=0)
    assert all(getattr(r, f) is None for f in abi.SCENARIO_TOPIC_FIELDS)
    with pytest.raises(ValueError):
        r.topic_impact()

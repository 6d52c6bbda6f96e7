"""The rack pass (include/kas_abi.h: kas_rack_impact / kas_scenario_rack_impact) without a GPU.

- The kernel bodies (kafka-assigner_amd/csrc/kas_racks_body.h) compiled with g++ against tests/emu/kas_wave.h and stepped on CPU
  fibers (tests/emu/rack_driver.cpp) over oracle-produced out tables, against the NumPy checker (tests/rack_ref.py): the row loop's
  step boundary, every width class, ragged rows, a duplicate broker in a row, departed cells, failing topics, scenarios without
  topics or brokers, a topic split into items, sparse ids, 16-bit cells, one rack and one rack per node, a report table that is
  not the solver's, two scenarios on one node range with different rack counts, a change of table on one plan, and the racks
  read from global memory.
- Identities, the refusals in their order, the host call planner's bytes (unchanged for the calls that were there), the ABI.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from impact_batches import T, assert_exercises, big_scenario, scenario, solved
from impact_ref import impact_ref
from kafka_assigner_amd import abi, native
from kafka_assigner_amd.flatten import batch_desc, flatten, index_form, to_cells16
from oracle_lib import oracle_solve
from rack_ref import assert_same_racks, check_identities, rack_counts, rack_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "kafka-assigner_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "kas_abi.h")
E_INVALID, E_UNSUPPORTED = abi.KAS_E_INVALID_ARG, abi.KAS_E_UNSUPPORTED
_LIB = None


# ---- the emulator ---------------------------------------------------------------------------------------------------------
def _emu_lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    so = os.path.join(EMU, "libkas_emu_racks.so")
    srcs = [os.path.join(EMU, f) for f in ("rack_driver.cpp", "impact_driver.cpp", "emu_driver.cpp")]
    deps = srcs + [os.path.join(EMU, "kas_wave.h"), HEADER] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        tmp = so + ".tmp%d" % os.getpid()
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unused-parameter", "-Wno-unknown-pragmas",
                               "-I" + os.path.join(ROOT, "tests"), "-I" + CSRC, "-I" + os.path.join(ROOT, "include"),
                               "-o", tmp] + srcs)
        os.replace(tmp, so)
    L = C.CDLL(so)
    L.kas_emu_racks.restype = C.c_int
    L.kas_emu_racks.argtypes = [C.POINTER(abi.BatchDesc), C.POINTER(abi.Tables), C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_char_p, C.c_int]
    L.kas_emu_racks_reset.restype = None
    L.kas_emu_rack_host_call.restype = C.c_int
    L.kas_emu_rack_host_call.argtypes = [C.POINTER(abi.BatchDesc), C.POINTER(C.c_int64), C.c_int32, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                         C.c_int64, C.c_uint, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_char_p, C.c_int]
    L.kas_emu_rack_buffers.restype = C.c_int
    L.kas_emu_rack_buffers.argtypes = [C.c_int]
    _LIB = L
    return L


def emu_racks_rc(fb, ho, report_rack=None, cells16=False, cur16=None, rows_per_item=0, rack_cap=-1, racks_cap=None, keep=False):
    """kas_emu_racks over the tables a solve left in `ho`: (rc, error text, (racks, scenarios, rack_off), node records, info)."""
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
    nodes, scen = native.impact_arrays(fb)
    rep = None if report_rack is None else np.ascontiguousarray(report_rack, dtype=np.int32)
    S = fb.n_scenarios
    try:
        need = int(rack_counts(fb, rep).sum())
    except ValueError:
        need = 0
    cap = max(need, 0) if racks_cap is None else racks_cap
    racks = np.full(max(min(max(cap, need), 1 << 20), 1), -7, dtype=abi.RACK_IMPACT_DTYPE)      # (every record must be written)
    rscen = np.full(max(S, 1), -7, dtype=abi.SCENARIO_RACK_IMPACT_DTYPE)
    rack_off = np.full(S + 1, -7, dtype=np.int64)
    info = (C.c_int32 * 4)()
    err = C.create_string_buffer(512)
    if not keep:
        L.kas_emu_racks_reset()
    rc = L.kas_emu_racks(C.byref(bd), C.byref(t), int(cells16), int(rows_per_item), int(rack_cap), None if rep is None else rep.ctypes.data,
                         nodes.ctypes.data, scen.ctypes.data, racks.ctypes.data, int(cap), rscen.ctypes.data, rack_off.ctypes.data,
                         info, err, 512)
    got = (racks[:max(int(rack_off[S]), 0)], rscen[:S], rack_off) if rc == 0 else None
    return rc, err.value.decode(), got, nodes, dict(zip(("rebuilt", "racks_in_lds", "items", "r_max"), list(info)))


def emu_racks(fb, ho, **kw):
    rc, err, got, nodes, info = emu_racks_rc(fb, ho, **kw)
    assert rc == 0, (rc, err)
    return got, nodes, info


def solved16(fb):
    """The oracle's solve of the batch's 16-bit form: (HostOutputs with uint16 out, cur16)."""
    ho = oracle_solve(index_form(fb))
    ho.out = np.where(ho.out < 0, abi.KAS_CELL16_NONE, ho.out).astype(np.uint16)
    return ho, to_cells16(fb)


# ---- report tables --------------------------------------------------------------------------------------------------------
def one_rack(fb):
    return np.zeros(fb.node_rack.shape[0], dtype=np.int32)


def rack_per_node(fb):
    """node i of every scenario on rack i: R_s = N (beyond KAS_RACK_LIMIT nodes the racks wrap: R_s = KAS_RACK_LIMIT)"""
    rr = np.zeros(fb.node_rack.shape[0], dtype=np.int32)
    for s in range(fb.n_scenarios):
        off, n = int(fb.scen["node_off"][s]), int(fb.scen["n_nodes"][s])
        rr[off:off + n] = np.arange(n) % abi.KAS_RACK_LIMIT
    return rr


def real_racks(fb, R):
    """broker b on rack b mod R whatever the solver's table says (impact_batches.scenario's layout, ids as they are)"""
    return (fb.node_id % R).astype(np.int32)


# ---- batches (beside impact_batches.BATCHES, whose oracle solves are shared) ------------------------------------------------
_OWN = {}


def own(name):
    """(fb, ho) of a batch of this file, built and solved by the oracle once"""
    if name not in _OWN:
        fb = {
            "width_1": lambda: flatten([scenario(301, 30, 5, [T(200, 1, 1), T(150, 1, 1, ragged=0.2)], remove=[4])]),
            "split_9000": lambda: big_scenario(9000, N=69, seed=2, noise=2),   # (69 - 3 brokers leave 60 free slots under the cap)
            "rack_unaware": lambda: flatten([scenario(311, 40, 8, [T(900, balanced=True, exact=True)], remove=[3, 17], rack_aware=False),
                                             scenario(311, 40, 8, [T(900, balanced=True, exact=True)], remove=[3, 17])]),
            "duplicates": _duplicates_batch,
            "shared_prefix": _shared_prefix_batch,
        }[name]()
        _OWN[name] = (fb, oracle_solve(fb))
    return _OWN[name]


def _duplicates_batch():
    """rows whose second replica repeats the first (a broker twice in one row of cur)"""
    fb = flatten([scenario(321, 30, 5, [T(300)], remove=[7])])
    rows = fb.cur[:300 * 3].reshape(300, 3)
    rows[::11, 1] = rows[::11, 0]
    return fb


def _shared_prefix_batch():
    """two scenarios on ONE node range: scenario 1 reads the first 24 of scenario 0's 30 nodes.  Reported on racks laid out in
    blocks of six (node i on rack i // 6), scenario 0 has five racks and scenario 1 four."""
    a = scenario(331, 30, 5, [T(400)])
    b = scenario(332, 30, 5, [T(300, ragged=0.1)], remove=[24, 25, 26, 27, 28, 29])
    fb = flatten([a, b])
    assert fb.scen["n_nodes"].tolist() == [30, 24] and fb.node_id[30:54].tolist() == list(range(24))
    fb.scen["node_off"][1] = fb.scen["node_off"][0]
    return fb


def blocks_of_six(fb):
    rr = np.zeros(fb.node_rack.shape[0], dtype=np.int32)
    rr[:30] = np.arange(30) // 6
    return rr


def _check(fb, ho, what, report_rack=None, cells=(False,), rows=(0,), caps=(-1,), ho16=None, cur16=None):
    """every combination on the emulator against the checker; the node records the reduce kernel folded against impact_ref's"""
    want_nodes = impact_ref(fb, ho)[0]
    want = rack_ref(fb, ho, report_rack, nodes=want_nodes)
    infos = []
    for c16 in cells:
        if c16 and ho16 is None:
            ho16, cur16 = solved16(fb)
            assert_same_racks(want, rack_ref(fb, ho16, report_rack, cells16=True, cur16=cur16), f"{what}: checker, 16-bit cells")
        for r in rows:
            for cap in caps:
                got, nodes, info = emu_racks(fb, ho16 if c16 else ho, report_rack=report_rack, cells16=c16, cur16=cur16 if c16 else None,
                                             rows_per_item=r, rack_cap=cap)
                assert_same_racks(want, got, f"{what}: cells16={c16}, rows per item {r}, rack cap {cap}")
                assert info["racks_in_lds"] == (0 if 0 <= cap < int(fb.scen["n_nodes"].max()) else 1) and info["rebuilt"] == 1
                for f in abi.NODE_IMPACT_FIELDS:
                    assert (nodes[f] == want_nodes[f]).all(), (what, f)
                infos.append(info)
    check_identities(fb, ho, want_nodes, want)
    return want, infos


def _counts_something(want, fields):
    for f in fields:
        assert int(want[1][f].sum()) > 0, f


# ---- the cases ------------------------------------------------------------------------------------------------------------
def test_row_step_boundary():
    """P = 1, 511, 512, 513, 1025 around the row loop's step of 2 x 256 rows; items of 512, 513 and 514 rows"""
    fb, ho, _ = solved("row_counts")
    want, _ = _check(fb, ho, "row_counts", cells=(False, True), rows=(0, 97, 512, 513, 514), caps=(-1, 0))
    # rack-aware solves on five racks at RF 3 of a rack-diverse snapshot: nothing shares a rack, before or after
    assert not want[1]["colocated_after"].any() and not want[1]["colocated_before"].any()
    assert not want[1]["single_rack_rows_after"].any()
    # ... and the same rows reported on ONE rack: every row with two known replicas is a single-rack row
    one = rack_ref(fb, ho, one_rack(fb))
    got, _, _ = emu_racks(fb, ho, report_rack=one_rack(fb))
    assert_same_racks(one, got, "row_counts on one rack")
    for s, P in enumerate(fb.topics["n_partitions"]):
        assert int(got[1]["single_rack_rows_after"][s]) == int(got[1]["rows_colocated_after"][s]) == int(P)
        assert int(got[1]["colocated_after"][s]) == 2 * int(P) and int(got[1]["new_rack_replicas"][s]) == 0


@pytest.mark.parametrize("name,wc", [("width_1", 2), ("mixed7", 3), ("widths_4_5", 5), ("widths_6_8", 8)])
def test_list_widths(name, wc):
    """lists 1, 2 and 3 wide (the <3> instance), 4 and 5 (<5>), 6 to 8 (<8>), RF raised and lowered among them"""
    fb, ho = own(name) if name == "width_1" else solved(name)[:2]
    w = int(fb.topics["out_width"].max())
    assert (2 if w <= 2 else (w if w <= 5 else 8)) == wc
    if name == "width_1":
        assert (ho.topic_results["status"] == abi.KAS_OK).all() and int(fb.topics["cur_width"].max()) == 1
    _check(fb, ho, name, cells=(False, True) if wc <= 3 else (False,), rows=(0, 97), caps=(-1, 0))
    # ... reported on one rack per node and on a single rack
    for table in (rack_per_node(fb), one_rack(fb)):
        want, _ = _check(fb, ho, name + ", extreme table", report_rack=table)
    _counts_something(want, ("colocated_before", "colocated_after", "single_rack_rows_after") if w > 1 else ("n_racks",))


def test_ragged_rows_departed_cells_and_a_duplicate_broker():
    """cur_len arrays with clen = 0 among them, replicas on removed brokers, and a broker twice in one row of cur"""
    fb, ho, _ = solved("mixed8")
    lens = np.concatenate([fb.aux[int(o):int(o) + int(p)] for o, p in zip(fb.topics["cur_len_off"], fb.topics["n_partitions"]) if o >= 0])
    assert (lens == 0).any() and (lens > 0).any()
    assert int(impact_ref(fb, ho)[1]["departed_replicas"].sum()) > 0
    _check(fb, ho, "mixed8", cells=(False, True), rows=(0, 97), caps=(-1, 0))
    fb, ho = own("duplicates")
    assert int(ho.topic_results["status"][0]) == abi.KAS_OK
    rows = fb.cur[:300 * 3].reshape(300, 3)
    assert int((rows[:, 0] == rows[:, 1]).sum()) >= 27
    want, _ = _check(fb, ho, "duplicates", rows=(0, 97), caps=(-1, 0))
    # a broker twice is two known cells on one rack: the rows with the duplicate are exactly the colocated ones (or, with the
    # duplicated broker removed, rows of one known cell)
    known_dup = int(((rows[:, 0] == rows[:, 1]) & (rows[:, 0] != 7)).sum())
    assert int(want[1]["rows_colocated_before"][0]) == int(want[1]["colocated_before"][0]) == known_dup > 0


def test_statuses_and_degenerate_scenarios():
    """a failing topic and a skipped one beside OK ones; a scenario without topics; a scenario without brokers"""
    from test_impact_cpu import _failing_then_skipped_batch
    fb = _failing_then_skipped_batch()
    ho = oracle_solve(fb)
    assert ho.topic_results["status"].tolist() == [abi.KAS_FAIL_RF_NOT_POSITIVE, abi.KAS_SKIPPED, abi.KAS_OK, abi.KAS_OK]
    want, _ = _check(fb, ho, "failing then skipped", rows=(0, 64), caps=(-1, 0))
    assert not any(int(want[1][f][0]) for f in abi.SCENARIO_RACK_ROW_FIELDS) and int(want[1]["n_racks"][0]) == 5
    assert not want[0][:5]["replicas_after"].any() and want[0][:5]["nodes"].tolist() == [4] * 5
    fb, ho, _ = solved("degenerate")
    assert fb.scen["topic_count"].tolist() == [3, 0, 1] and fb.scen["n_nodes"].tolist() == [29, 12, 0]
    want, _ = _check(fb, ho, "degenerate", cells=(False, True), rows=(0, 97), caps=(-1, 0))
    assert want[2].tolist() == [0, 5, 9, 9]
    assert int(want[1]["n_racks"][1]) == 4 and not any(int(want[1][f][2]) for f in abi.SCENARIO_RACK_FIELDS)
    assert want[0][5:9]["nodes"].tolist() == [3] * 4 and not want[0][5:9]["replicas_before"].any()


def test_a_topic_split_into_three_items():
    """one topic of 9,000 rows in a batch of one topic: three items of the impact pass's work list add into one scenario's sums"""
    fb, ho = own("split_9000")
    assert int(fb.topics["n_partitions"][0]) == 9000 and int(ho.topic_results["status"][0]) == abi.KAS_OK
    want, infos = _check(fb, ho, "split_9000", cells=(False, True), caps=(-1, 0))
    assert all(i["items"] == 3 for i in infos)
    assert int(want[0]["replicas_after"].sum()) == 27000 and int(want[1]["new_rack_replicas"][0]) >= 0


@pytest.mark.parametrize("name", ["sparse", "dense_and_sparse", "beyond_the_table"])
def test_sparse_ids(name):
    """ids that force the binary search, alone and beside a scenario on the direct table"""
    fb, ho, _ = solved(name)
    _check(fb, ho, name, rows=(0, 97), caps=(-1, 0))


def test_custom_table_for_a_rack_unaware_solve():
    """a variant solved without rack awareness (the solver's table is id-as-rack) reported on the real racks, beside its
    rack-aware sibling: the first puts replicas of a row on one rack, the second never does"""
    fb, ho = own("rack_unaware")
    assert (ho.topic_results["status"] == abi.KAS_OK).all()
    assert len(set(fb.node_rack[:38].tolist())) == 38 and len(set(fb.node_rack[38:].tolist())) == 8
    table = real_racks(fb, 8)
    assert (table[38:] == fb.node_rack[38:]).all() or len(set(zip(table[38:].tolist(), fb.node_rack[38:].tolist()))) == 8
    want, _ = _check(fb, ho, "rack_unaware on real racks", report_rack=table, cells=(False, True), rows=(0, 97), caps=(-1, 0))
    assert want[1]["n_racks"].tolist() == [8, 8]
    assert int(want[1]["colocated_after"][0]) > 0 and int(want[1]["colocated_after"][1]) == 0
    assert int(want[1]["rows_losing_racks"][0]) > 0
    own_table, _ = _check(fb, ho, "rack_unaware on the solver's own table")
    assert int(own_table[1]["n_racks"][0]) == 38 and int(own_table[1]["colocated_after"][0]) == 0


def test_two_scenarios_on_one_node_range_with_different_rack_counts():
    fb, ho = own("shared_prefix")
    assert int(fb.scen["node_off"][0]) == int(fb.scen["node_off"][1]) and (ho.topic_results["status"] == abi.KAS_OK).all()
    table = blocks_of_six(fb)
    want, _ = _check(fb, ho, "shared_prefix", report_rack=table, cells=(False, True), rows=(0, 97), caps=(-1, 0))
    assert want[2].tolist() == [0, 5, 9] and want[1]["n_racks"].tolist() == [5, 4]
    assert want[0]["nodes"].tolist() == [6] * 9
    P = fb.topics["n_partitions"]
    assert int(want[0]["replicas_after"][:5].sum()) == 3 * int(P[0]) and int(want[0]["replicas_after"][5:].sum()) == 3 * int(P[1])


def test_change_of_table_on_one_plan():
    """two calls with different tables on one plan: the second gets its own table's records (the contents are compared); a third
    call with a copy of the second's table at another address rebuilds nothing"""
    fb, ho, _ = solved("mixed7")
    a, b = fb.node_rack.copy(), rack_per_node(fb)
    _emu_lib().kas_emu_racks_reset()
    got_a, _, info_a = emu_racks(fb, ho, report_rack=a, keep=True)
    got_b, _, info_b = emu_racks(fb, ho, report_rack=b, keep=True)
    got_b2, _, info_b2 = emu_racks(fb, ho, report_rack=b.copy(), keep=True)
    got_n, _, info_n = emu_racks(fb, ho, report_rack=None, keep=True)                # NULL: the batch's node_rack, = a
    same_address = a.copy()
    got_c, _, info_c = emu_racks(fb, ho, report_rack=same_address, keep=True)
    same_address[:] = b                                                              # another table at the SAME address
    got_d, _, info_d = emu_racks(fb, ho, report_rack=same_address, keep=True)
    assert [i["rebuilt"] for i in (info_a, info_b, info_b2, info_n, info_c, info_d)] == [1, 1, 0, 1, 0, 1]
    assert_same_racks(rack_ref(fb, ho, a), got_a, "first table")
    for got in (got_b, got_b2, got_d):
        assert_same_racks(rack_ref(fb, ho, b), got, "second table")
    for got in (got_n, got_c):
        assert_same_racks(rack_ref(fb, ho, None), got, "the batch's own table")
    assert int(got_a[2][-1]) != int(got_b[2][-1])


def test_racks_from_global_memory_beyond_the_lds():
    """7,000 brokers fit the LDS (table and racks); the path for more is forced on them and on a small batch through the cap"""
    fb, ho, _ = solved("many_brokers")
    want, infos = _check(fb, ho, "many_brokers", cells=(False, True), caps=(-1, 0))
    assert int(want[1]["n_racks"][0]) == 20 and want[0]["nodes"].tolist() == [350] * 20
    fb, ho, _ = solved("mixed21")
    _check(fb, ho, "mixed21", cells=(False, True), rows=(0, 97), caps=(-1, 0, 30, 1000))
    assert int(fb.scen["n_nodes"].max()) == 39                 # (a cap of 30 is below it, one of 1000 above)


def test_identities_on_every_shared_batch():
    """sum over racks of each field == sum over nodes, sum of inbound == moved_replicas, every scenario field non-negative"""
    for name in ("mixed7", "mixed42", "shared_node_range", "widths_6_8", "id_range_edge", "rows_4097"):
        fb, ho, (nodes, _) = solved(name)
        for table in (None, one_rack(fb), rack_per_node(fb)):
            rk = rack_ref(fb, ho, table)
            check_identities(fb, ho, nodes, rk)
            got, _, _ = emu_racks(fb, ho, report_rack=table)
            assert_same_racks(rk, got, name)
            ok = ho.scenario_results["status"] == abi.KAS_OK
            if table is None:                                # rack-aware solves on >= RF racks of a rack-diverse snapshot
                assert not rk[1]["colocated_after"][ok].any(), name


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_in_their_order():
    fb, ho, _ = solved("mixed7")
    good = fb.node_rack.copy()
    need = int(rack_counts(fb).sum())
    neg = good.copy(); neg[3] = -1
    big = good.copy(); big[5] = abi.KAS_RACK_LIMIT                              # R_s = 4097
    both = big.copy(); both[int(fb.scen["node_off"][1]) + 2] = -1               # a negative entry BEHIND the oversized scenario
    edge = good.copy(); edge[5] = abi.KAS_RACK_LIMIT - 1                        # R_s = 4096: taken
    cases = [(neg, None, E_INVALID, "negative"), (big, None, E_UNSUPPORTED, "KAS_RACK_LIMIT"), (both, None, E_INVALID, "negative"),
             (both, 0, E_INVALID, "negative"), (big, 0, E_UNSUPPORTED, "KAS_RACK_LIMIT"), (good, need - 1, E_INVALID, "racks_cap")]
    for table, cap, code, text in cases:
        rc, err, _, _, _ = emu_racks_rc(fb, ho, report_rack=table, racks_cap=cap)
        assert rc == code and text in err, (rc, err, text)
    rc, err, got, _, _ = emu_racks_rc(fb, ho, report_rack=edge, racks_cap=None)
    assert rc == 0 and int(got[1]["n_racks"][0]) == abi.KAS_RACK_LIMIT, err
    assert_same_racks(rack_ref(fb, ho, edge), got, "R_s = KAS_RACK_LIMIT")
    # the host call planner, the same order behind its own checks
    for table, cap, code, text in cases:
        rc, _, err = rack_host_call(fb, report_rack=table, racks_cap=need if cap is None else cap)
        assert rc == code and text in err, (rc, err, text)
    assert rack_host_call(fb, racks_cap=need, missing=("rack_off",))[0] == E_INVALID
    assert rack_host_call(fb, racks_cap=need, missing=("scenarios",))[0] == E_INVALID
    assert rack_host_call(fb, racks_cap=need)[0] == 0
    # a table for a batch without nodes
    empty = flatten([])
    rc, _, err = rack_host_call(empty, report_rack=np.zeros(1, np.int32), racks_cap=0)
    assert rc == E_INVALID and "without nodes" in err
    assert rack_host_call(empty, racks_cap=0)[0] == 0


# ---- the planner ------------------------------------------------------------------------------------------------------------
HOST_BUFS = ("cur", "out", "aux", "ctx", "cur16", "out16", "tr", "sr", "tr_pin", "sr_pin", "imp_nodes", "imp_scen",
             "ch_sizes", "ch_segs", "ch_head", "ch_rows", "ch_nodes", "ch_head_pin", "ch_rows_pin", "ch_nodes_pin",
             "mv_scen", "mv_segs", "mv_select", "mv_scratch", "mv_head", "mv_moves", "mv_cells", "mv_sizes0", "mv_head_pin",
             "fr_cls", "fr_counts", "fr_counts_pin", "rk_racks", "rk_scen")
MISSING = {"racks": 1, "scenarios": 2, "rack_off": 4}


def rack_host_call(fb, racks=True, report_rack=None, racks_cap=0, n_select=0, cells16=False, nodes=False, missing=()):
    """kas_plan_host_call for kas_solve_host_rack_impact (racks) or kas_solve_host_impact: (rc, {bytes by name, rack_off}, text)"""
    L = _emu_lib()
    assert L.kas_emu_rack_buffers(0) == len(HOST_BUFS) and L.kas_emu_rack_buffers(1) == len(HOST_BUFS) - 2
    bd = batch_desc(fb)
    lens = (C.c_int64 * 4)(int(fb.cur.shape[0]), int(fb.out_len), int(fb.aux.shape[0]), int(fb.ctx.shape[0]))
    rep = None if report_rack is None else np.ascontiguousarray(report_rack, dtype=np.int32)
    nbytes = (C.c_int64 * len(HOST_BUFS))()
    rack_off = (C.c_int64 * (fb.n_scenarios + 1))()
    err = C.create_string_buffer(512)
    rc = L.kas_emu_rack_host_call(C.byref(bd), lens, n_select, int(cells16), int(racks), int(nodes), None if rep is None else rep.ctypes.data,
                                  int(racks_cap), sum(MISSING[m] for m in missing), nbytes, rack_off, err, 512)
    if rc != 0:
        return rc, None, err.value.decode()
    return rc, dict(bytes=dict(zip(HOST_BUFS, [int(v) for v in nbytes])), rack_off=[int(v) for v in rack_off]), ""


# what the parent of this change planned for mixed42 (kas_solve_host_impact, n_select = 0 and every row): bytes of the buffers
# every host call may use, in KasHostBuf's order, for int32 and 16-bit cells
PARENT = {(False, -1): [39028, 48644, 23936, 32, 0, 0, 208, 224, 208, 224, 6400, 224],
          (False, 0): [39028, 48644, 23936, 32, 0, 0, 208, 224, 208, 224, 6400, 224],
          (True, -1): [0, 0, 23936, 32, 19514, 24322, 208, 224, 208, 224, 6400, 224],
          (True, 0): [0, 0, 23936, 32, 19514, 24322, 208, 224, 208, 224, 6400, 224]}


@pytest.mark.parametrize("cells16", [False, True], ids=["int32", "cells16"])
def test_planner_bytes_of_existing_calls_are_unchanged(cells16):
    import emu_lib
    fb, _, _ = solved("mixed42")
    S, need = fb.n_scenarios, int(rack_counts(fb).sum())
    for sel, n_select in ((None, -1), ([], 0)):
        rc, plan, err = emu_lib.host_call(fb, select=sel, cells16=cells16, impact=True)
        assert rc == 0, err
        assert [plan["bytes"][n] for n in emu_lib.HOST_BUFS] == PARENT[(cells16, n_select)]
        rc, mine, err = rack_host_call(fb, racks=False, n_select=n_select, cells16=cells16, nodes=True)
        assert rc == 0, err
        assert [mine["bytes"][n] for n in emu_lib.HOST_BUFS] == PARENT[(cells16, n_select)]
        assert not any(mine["bytes"][n] for n in HOST_BUFS[len(emu_lib.HOST_BUFS):])          # nothing behind them, the new ids included
        # the rack call: the same bytes of every buffer that was there, and its two records buffers behind them
        rc, rk, err = rack_host_call(fb, racks_cap=need, n_select=n_select, cells16=cells16)
        assert rc == 0, err
        assert [rk["bytes"][n] for n in HOST_BUFS[:-2]] == [mine["bytes"][n] for n in HOST_BUFS[:-2]]
        assert rk["bytes"]["rk_racks"] == 32 * (need + 1) and rk["bytes"]["rk_scen"] == 64 * (S + 1)
        assert rk["rack_off"] == np.concatenate([[0], np.cumsum(rack_counts(fb))]).tolist()


# ---- ABI ------------------------------------------------------------------------------------------------------------------
def test_abi_declares_the_rack_entries_and_records(tmp_path):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(kas_[a-z_0-9]+)\s*\(", src))
    for name in abi.RACK_ENTRIES:
        assert name in declared and name in native.SYMBOLS, name
    assert re.search(r"#define KAS_ABI_VERSION (\d+)", src).group(1) == str(abi.KAS_ABI_VERSION) == "6"
    assert re.search(r"#define KAS_RACK_LIMIT (\d+)", src).group(1) == str(abi.KAS_RACK_LIMIT) == "4096"
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kas_abi.h"\n'
                     'int main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(kas_rack_impact), sizeof(kas_scenario_rack_impact), '
                     'sizeof(kas_rack_tables), offsetof(kas_rack_impact, outbound), offsetof(kas_scenario_rack_impact, n_racks), '
                     'offsetof(kas_scenario_rack_impact, max_rack_leaders_after)); return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c11", "-I" + os.path.join(ROOT, "include"), str(probe), "-o", str(exe)])
    assert subprocess.check_output([str(exe)], text=True).split() == ["32", "64", "32", "24", "32", "56"]
    assert abi.RACK_IMPACT_DTYPE.fields["outbound"][1] == 24 and abi.SCENARIO_RACK_IMPACT_DTYPE.fields["n_racks"][1] == 32
    assert abi.SCENARIO_RACK_IMPACT_DTYPE.fields["max_rack_leaders_after"][1] == 56


def test_library_exports_the_rack_entries():
    from kafka_assigner_amd import build
    build.build()
    L = native.load()
    for name in abi.RACK_ENTRIES:
        assert hasattr(L, name), name
    assert L.kas_abi_version() == 6
    blob = open(build.LIB, "rb").read()
    assert b"kas_rack_rows_kernel" in blob and b"kas_rack_reduce_kernel" in blob


def test_whatif_report_table_is_built_from_the_real_racks():
    """WhatIf.report_racks: the real racks whatever rack_aware says, a None rack as the broker's id, names back through the index"""
    from kafka_assigner_amd.whatif import Variant, WhatIf
    brokers = {0: "a", 1: "b", 2: "a", 3: None, 4: "b"}
    w = WhatIf(brokers, {"t": {0: [0, 1], 1: [2, 3]}})
    variants = [Variant(), Variant(rack_aware=False), Variant(remove=[0, 2], add={7: "c", 8: None})]
    fb = w.flat_batch(variants)
    table, names = w.report_racks(variants)
    assert table.tolist() == [0, 1, 0, 2, 1, 0, 1, 0, 2, 1, 0, 1, 0, 2, 3]
    assert names == [["a", "b", "3"], ["a", "b", "3"], ["b", "3", "c", "8"]]
    assert fb.node_rack[:5].tolist() == [0, 1, 0, 2, 1] and fb.node_rack[5:10].tolist() == [0, 1, 2, 3, 4]

"""The impact pass (ABI v6, include/kas_abi.h: kas_node_impact / kas_scenario_impact) without a GPU.

- The NumPy checker (tests/impact_ref.py) on the oracle's outputs: its invariants on the Appendix B vectors and random batches.
- The kernel body (kafka-assigner_amd/csrc/kas_impact_body.h) compiled with g++ against tests/emu/kas_wave.h and stepped on
  CPU fibers (tests/emu/impact_driver.cpp) over oracle-produced out tables: equal to the checker for one- and multi-item
  scenarios (the merge kernel), ragged lists, in_partitions flags, a failing topic followed by a skipped one, multi-topic
  scenarios, two scenarios on one node range, both cell layouts and the counters beyond the LDS budget; lists 4-8 wide with
  the replication factor raised and lowered, the binary-search lookup, the row loop's and the items' edges, scenarios without
  topics or brokers.  The batches come from tests/impact_batches.py, whose assert_exercises() keeps them counting rows.
- The ABI: the new entry points are declared and exported, the records are 32 bytes.
"""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from impact_batches import (ROW_COUNTS, STALE_ID, assert_exercises, lookup_kind, many_brokers_batch, mixed_batch, shared_node_range_batch,
                            solved)
from impact_ref import assert_same_impact, check_invariants, impact_ref
from kafka_assigner_amd import abi, native
from kafka_assigner_amd import generator as G
from kafka_assigner_amd.flatten import Scenario, Topic, batch_desc, flatten, index_form, to_cells16
from oracle_lib import oracle_solve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "kafka-assigner_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "kas_abi.h")
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "survey_appendix_b.json")))
NEW_ENTRIES = ["kas_impact_device", "kas_impact_device16", "kas_solve_host_impact", "kas_solve_host16_impact"]
_LIB = None


# ---- the emulator ---------------------------------------------------------------------------------------------------------
def _emu_lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    so = os.path.join(EMU, "libkas_emu_impact.so")
    srcs = [os.path.join(EMU, "impact_driver.cpp"), os.path.join(EMU, "emu_driver.cpp")]
    deps = srcs + [os.path.join(EMU, "kas_wave.h"), HEADER] + [os.path.join(CSRC, f) for f in (
        "kas_impact.h", "kas_impact_body.h", "kas_plan_math.h", "kas_solver_body.h", "kas_order_relax.h", "kas_order_wide.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        tmp = so + ".tmp%d" % os.getpid()
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unused-parameter", "-Wno-unknown-pragmas",
                               "-I" + os.path.join(ROOT, "tests"), "-I" + CSRC, "-I" + os.path.join(ROOT, "include"),
                               "-o", tmp] + srcs)
        os.replace(tmp, so)
    L = C.CDLL(so)
    L.kas_emu_impact.restype = C.c_int
    L.kas_emu_impact.argtypes = [C.POINTER(abi.BatchDesc), C.POINTER(abi.Tables), C.c_int, C.c_int, C.c_int64,
                                 C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_char_p, C.c_int]
    L.kas_emu_impact_lds_fill.restype = None
    L.kas_emu_impact_lds_fill.argtypes = [C.c_uint32]
    _LIB = L
    return L


def emu_impact(fb, ho, cells16=False, cur16=None, node_cap=-1, rows_per_item=0, lds_fill=0xCDCDCDCD):
    """kas_emu_impact over the tables a solve left in `ho`: ((nodes, scenarios), {items, merges, global_items, node_cap}).
    lds_fill: the word every workgroup finds all over its LDS (what the workgroup before left there)."""
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
    nodes[...] = -7                                       # (every record must be written)
    scen[...] = -7
    info = (C.c_int32 * 4)()
    err = C.create_string_buffer(512)
    _emu_lib().kas_emu_impact_lds_fill(lds_fill)
    try:
        rc = _emu_lib().kas_emu_impact(C.byref(bd), C.byref(t), int(cells16), int(node_cap), int(rows_per_item),
                                       nodes.ctypes.data, scen.ctypes.data, info, err, 512)
    finally:
        _emu_lib().kas_emu_impact_lds_fill(0xCDCDCDCD)
    assert rc == 0, (rc, err.value.decode())
    return (nodes, scen), dict(zip(("items", "merges", "global_items", "node_cap"), list(info)))


def solved16(fb):
    """The oracle's solve of the batch's 16-bit form: (HostOutputs with uint16 out, cur16)."""
    ho = oracle_solve(index_form(fb))
    ho.out = np.where(ho.out < 0, abi.KAS_CELL16_NONE, ho.out).astype(np.uint16)
    return ho, to_cells16(fb)


# ---- batches --------------------------------------------------------------------------------------------------------------
def _appendix_b_batch():
    scs = []
    C1 = GOLD["config1"]
    for case in C1["cases"]:
        racks = {int(k): v for k, v in case["racks"].items()}
        topics = [Topic(name, {int(p): r for p, r in C1["current"][t].items()}, 3) for t, name in enumerate(C1["topics"])]
        scs.append(Scenario(brokers=case["brokers"], racks=racks, topics=topics))
    for case in GOLD["ktat"]:
        cur = {int(p): r for p, r in case["current"].items()}
        rf = case["desired_rf"] if case["desired_rf"] > 0 else max([len(r) for r in cur.values()] + [1])
        scs.append(Scenario(brokers=case["brokers"], racks={int(k): v for k, v in case["racks"].items()},
                            topics=[Topic(case["topic"], cur, rf)]))
    return flatten(scs)


def _random_batch(seed, n_scen=4):
    """remove / add / replace / as is, one to three topics per scenario, ragged lists, partition sets that are not the keys of
    the current assignment, replicas on brokers outside the set (impact_batches.mixed_batch: topics that solve)"""
    return mixed_batch(seed, n_scen=n_scen)


def _failing_then_skipped_batch():
    """scenario 0: topic 0 has no positive replication factor, so topic 1 is KAS_SKIPPED; scenario 1 is fine"""
    cur_a, cur_b = G.random_assignment(3, 200, 20, 5, 3), G.random_assignment(4, 150, 20, 5, 3)
    a = {p: cur_a[p].tolist() for p in range(200)}
    b = {p: cur_b[p].tolist() for p in range(150)}
    brokers = list(range(20))
    racks = {n: "r%d" % (n % 5) for n in brokers}
    return flatten([Scenario(brokers, racks, [Topic("a", a, 0), Topic("b", b, 3)]),
                    Scenario(brokers, racks, [Topic("a", a, 3), Topic("b", b, 3)])])


_shared_node_range_batch = shared_node_range_batch
_many_brokers_batch = many_brokers_batch


def guarded(fb, ho=None, **claims):
    """(ho, want): the oracle's solve of `fb` and the checker's records of it, after assert_exercises has found rows in them"""
    ho = oracle_solve(fb) if ho is None else ho
    want = impact_ref(fb, ho)
    assert_exercises(fb, ho, want, **claims)
    return ho, want


# ---- the checker on the oracle's outputs ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["appendix_b", "random0", "random1", "failing_then_skipped", "shared_node_range"])
def test_checker_invariants_on_oracle_outputs(name):
    fb = {"appendix_b": _appendix_b_batch, "random0": lambda: _random_batch(100), "random1": lambda: _random_batch(101),
          "failing_then_skipped": _failing_then_skipped_batch, "shared_node_range": _shared_node_range_batch}[name]()
    ho = oracle_solve(fb)
    imp = impact_ref(fb, ho)
    if name in ("random0", "random1", "shared_node_range"):
        assert_exercises(fb, ho, imp)
    check_invariants(fb, ho, imp)
    nodes, scen = imp
    base = native.node_blocks(fb)
    for s in range(fb.n_scenarios):
        blk = nodes[base[s]:base[s + 1]]
        if blk.size == 0:
            continue
        assert int(scen["max_inbound"][s]) == int(blk["inbound"].max())
        assert int(scen["min_replicas_after"][s]) == int(blk["replicas_after"].min())
        # every replica the scenario keeps or gives up is counted once: before == (after - inbound) + outbound, per node
        assert (blk["replicas_before"] == blk["replicas_after"] - blk["inbound"] + blk["outbound"]).all() or \
            (ho.topic_results["status"] != abi.KAS_OK).any()


def test_checker_sees_the_appendix_b_replacement():
    """'replace 5->6': broker 6 receives exactly what broker 5 gives up, and 5 keeps nothing"""
    fb = _appendix_b_batch()
    ho = oracle_solve(fb)
    nodes, scen = impact_ref(fb, ho)
    C1 = GOLD["config1"]
    s = [c["name"] for c in C1["cases"]].index("replace 5->6 (rack c)")
    ids = fb.node_id[int(fb.scen["node_off"][s]):int(fb.scen["node_off"][s]) + int(fb.scen["n_nodes"][s])].tolist()
    blk = nodes[native.node_blocks(fb)[s]:native.node_blocks(fb)[s + 1]]
    assert 5 not in ids
    i6 = ids.index(6)
    assert int(blk["replicas_before"][i6]) == 0 and int(blk["inbound"][i6]) == int(blk["replicas_after"][i6]) > 0
    assert int(scen["departed_replicas"][s]) == int(blk["inbound"].sum()) == int(ho.scenario_results["moved_replicas"][s])


# ---- the kernel body on CPU fibers ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [7, 8])
def test_emulated_kernel_equals_checker_random_batches(seed):
    fb = _random_batch(seed)
    ho, want = guarded(fb, merge=True, widths=[(2, 3), (3, 3)])
    got, info = emu_impact(fb, ho)
    assert info["merges"] > 0 and info["items"] > info["merges"]      # (multi-topic scenarios merge, single-topic ones do not)
    assert_same_impact(want, got, "emulated impact, one item per topic")
    got, info = emu_impact(fb, ho, rows_per_item=97)
    assert info["items"] > fb.n_topics
    assert_same_impact(want, got, "emulated impact, topics cut into items of 97 rows")


def test_emulated_kernel_one_item_scenarios_write_directly():
    fb = _shared_node_range_batch()
    ho, want = guarded(fb, must_solve=[0, 1])
    got, info = emu_impact(fb, ho)
    assert info == {"items": 2, "merges": 0, "global_items": 0, "node_cap": 29}
    assert_same_impact(want, got, "one item per scenario, two scenarios on one node range")
    assert native.node_blocks(fb)[-1] == 58
    nodes, scen = got
    for s in (0, 1):                                          # both blocks hold counts, and not the same ones
        assert int(nodes["replicas_after"][29 * s:29 * s + 29].sum()) > 0 and int(scen["leaders_moved"][s]) > 0
    assert any((nodes[f][:29] != nodes[f][29:]).any() for f in abi.NODE_IMPACT_FIELDS)
    assert any(int(scen[f][0]) != int(scen[f][1]) for f in abi.SCENARIO_IMPACT_FIELDS)


def test_emulated_kernel_failing_then_skipped_topic():
    fb = _failing_then_skipped_batch()
    ho = oracle_solve(fb)
    assert ho.topic_results["status"].tolist() == [abi.KAS_FAIL_RF_NOT_POSITIVE, abi.KAS_SKIPPED, abi.KAS_OK, abi.KAS_OK]
    want = impact_ref(fb, ho)
    assert int(want[0]["replicas_before"][:20].sum()) == 0                # failed and skipped topics count nothing
    for rows in (0, 64):
        got, _ = emu_impact(fb, ho, rows_per_item=rows)
        assert_same_impact(want, got, "failing then skipped, rows per item %d" % rows)


@pytest.mark.parametrize("seed", [21, 22])
def test_emulated_kernel_cells16_equals_int32(seed):
    fb = _random_batch(seed, n_scen=3)
    ho, want = guarded(fb, merge=True)
    ho16, cur16 = solved16(fb)
    assert_same_impact(want, impact_ref(fb, ho16, cells16=True, cur16=cur16), "checker, 16-bit cells")
    for rows in (0, 150):
        got16, _ = emu_impact(fb, ho16, cells16=True, cur16=cur16, rows_per_item=rows)
        assert_same_impact(want, got16, "emulated impact, 16-bit cells, rows per item %d" % rows)
        got32, _ = emu_impact(fb, ho, rows_per_item=rows)
        assert_same_impact(got32, got16, "int32 and 16-bit cells")


def test_emulated_kernel_global_counters():
    """the counters in global scratch: forced on a small batch, and for real beyond the LDS budget (7,000 brokers)"""
    fb = _random_batch(31, n_scen=3)
    ho, want = guarded(fb, merge=True)
    got, info = emu_impact(fb, ho, node_cap=0)
    assert info["global_items"] == info["items"] and info["merges"] == fb.n_scenarios
    assert_same_impact(want, got, "global counters (forced)")
    fb = _many_brokers_batch()
    ho, want = guarded(fb, must_solve=[0])
    assert int(ho.topic_results["status"][0]) == abi.KAS_OK
    assert int(want[1]["departed_replicas"][0]) > 0
    for cells16 in (False, True):
        h = solved16(fb)[0] if cells16 else ho
        got, info = emu_impact(fb, h, cells16=cells16)
        assert info["global_items"] == 1 and info["node_cap"] < 7000, info
        assert_same_impact(want, got, "beyond the LDS budget, cells16=%s" % cells16)


# ---- the paths no other test counts a row on ------------------------------------------------------------------------------
def _emulator_matrix(name, rows_per_item=(0, 97), cells16=True):
    """The named batch (impact_batches.BATCHES, guard passed) on the emulator: one item per topic and items of 97 rows, counters
    in the LDS and in global scratch, int32 and 16-bit cells -- every run equal to the checker on the oracle's rows."""
    fb, ho, want = solved(name)
    runs = [(False, ho, None)]
    if cells16:
        ho16, cur16 = solved16(fb)
        assert_same_impact(want, impact_ref(fb, ho16, cells16=True, cur16=cur16), f"{name}: checker, 16-bit cells")
        runs.append((True, ho16, cur16))
    infos = []
    for c16, h, cur16 in runs:
        for rows in rows_per_item:
            for cap in (-1, 0):
                got, info = emu_impact(fb, h, cells16=c16, cur16=cur16, node_cap=cap, rows_per_item=rows)
                assert_same_impact(want, got, f"{name}: cells16={c16}, rows per item {rows}, node_cap {cap}")
                assert (got[0]["reserved"] == 0).all()
                assert (info["global_items"] > 0) == (cap == 0)
                infos.append(info)
    return fb, ho, want, infos


def _width_class(fb):
    """kas_width_class (kas_plan_math.h) of the batch: the instance of kas_impact_kernel its launch takes"""
    w = int(fb.topics["out_width"].max())
    return 2 if w <= 2 else (w if w <= 5 else 8)


def test_emulated_kernel_lists_4_and_5_wide():
    """kas_impact_kernel<5>: (cur_width, rf) = (5,5), (4,4), (2,4) RF raised, (5,3) RF lowered (pads in out), (3,3)"""
    fb, ho, want, _ = _emulator_matrix("widths_4_5")
    assert _width_class(fb) == 5
    t = [i for i in range(fb.n_topics) if (int(fb.topics["cur_width"][i]), int(fb.topics["rf"][i])) == (5, 3)][0]
    td = fb.topics[t]
    rows = ho.out[int(td["out_off"]):][:int(td["n_partitions"]) * 5].reshape(-1, 5)
    assert (rows[:, 3] == -1).any() and (rows[:, 0] != -1).all()          # RF lowered: rows with pads behind the list


def test_emulated_kernel_lists_6_to_8_wide():
    """kas_impact_kernel<8>: (cur_width, rf) = (7,7), (8,8), (3,6) RF raised, (8,2) RF lowered"""
    fb, _, _, _ = _emulator_matrix("widths_6_8")
    assert _width_class(fb) == 8


@pytest.mark.parametrize("name", ["sparse", "dense_and_sparse", "id_range_edge", "beyond_the_table"])
def test_emulated_kernel_binary_search_lookup(name):
    """node_of's binary search over the sorted ids in the LDS: id ranges beyond KAS_IDMAP_CAP alone, next to a dense scenario
    whose direct table shares the LDS region, on either side of the cap (ranges of 16384 and 16385 ids), and for a departed
    broker whose id stands in the LDS right behind the table (the search's bound)"""
    fb, _, _, _ = _emulator_matrix(name)
    kinds = [lookup_kind(fb, s) for s in range(fb.n_scenarios)]
    assert kinds == {"sparse": ["bsearch"] * 2, "dense_and_sparse": ["direct", "bsearch", "direct"],
                     "id_range_edge": ["direct", "bsearch"], "beyond_the_table": ["bsearch"]}[name]
    if name == "beyond_the_table":
        fb, ho, want = solved(name)
        assert STALE_ID > int(fb.node_id.max()) and int((fb.cur == STALE_ID).sum()) > 0      # departed, above every id of the set
        for cap in (-1, 0):
            got, _ = emu_impact(fb, ho, node_cap=cap, lds_fill=STALE_ID)
            assert_same_impact(want, got, f"the departed broker's id all over the LDS, node_cap {cap}")


def test_emulated_kernel_row_loop_edges():
    """P = 1, 511, 512, 513, 1025 around the row loop's stride of ROWS_PER_LANE * KAS_IMPACT_BLOCK = 512 rows, and items of
    P - 1, P and P + 1 rows for P = 513"""
    fb, ho, want, _ = _emulator_matrix("row_counts", rows_per_item=(0, 97, 512, 513, 514), cells16=True)
    assert tuple(int(p) for p in fb.topics["n_partitions"]) == ROW_COUNTS
    items = {rows: emu_impact(fb, ho, rows_per_item=rows)[1]["items"] for rows in (512, 513, 514)}
    assert items == {512: 1 + 1 + 1 + 2 + 3, 513: 1 + 1 + 1 + 1 + 2, 514: 1 + 1 + 1 + 1 + 2}
    base = native.node_blocks(fb)
    for s, P in enumerate(ROW_COUNTS):                           # every row of every scenario is counted once
        assert int(want[0]["replicas_after"][base[s]:base[s + 1]].sum()) == 3 * P


def test_emulated_kernel_scenarios_without_topics_or_brokers():
    """a scenario without topics (work-list item with topic == -1) and a scenario without brokers beside a normal one: flatten
    and kas_shape_batch take both, and both records are written as zeros"""
    fb, ho, want, infos = _emulator_matrix("degenerate")
    assert fb.scen["topic_count"].tolist() == [3, 0, 1] and fb.scen["n_nodes"].tolist() == [29, 12, 0]
    assert int(ho.topic_results["status"][3]) == abi.KAS_FAIL_RF_GT_BROKERS
    assert infos[0]["items"] == 3 + 1 + 1
    nodes, scen = emu_impact(fb, ho)[0]
    assert nodes.shape[0] == 41 and not any(nodes[f][29:].any() for f in abi.NODE_IMPACT_FIELDS)
    for s in (1, 2):
        assert not any(int(scen[f][s]) for f in abi.SCENARIO_IMPACT_FIELDS)
    assert int(scen["min_replicas_after"][0]) > 0




@pytest.mark.parametrize("name,items,global_items", [("rows_4096", 1, 0), ("rows_4097", 2, 0), ("rows_10000", 3, 0),
                                                     ("many_brokers_10000", 3, 3)])
def test_emulated_kernel_items_cut_by_the_library_rule(name, items, global_items):
    """the GPU tests' shapes under kas_impact_rows_per_item (items of KAS_IMPACT_MIN_ITEM_ROWS = 4096 rows): 4096 rows are one
    DIRECT item, 4097 two FLUSH items and a merge, 10000 three -- and with 7,000 brokers three items adding into one region"""
    fb, ho, want = solved(name)
    ho16, cur16 = solved16(fb)
    assert_same_impact(want, impact_ref(fb, ho16, cells16=True, cur16=cur16), f"{name}: checker, 16-bit cells")
    for c16, h in ((False, ho), (True, ho16)):
        got, info = emu_impact(fb, h, cells16=c16, cur16=cur16 if c16 else None)
        assert (info["items"], info["merges"], info["global_items"]) == (items, int(items > 1), global_items), info
        assert_same_impact(want, got, f"{name}: cells16={c16}")


# ---- ABI ------------------------------------------------------------------------------------------------------------------
def test_abi_declares_the_impact_entries_and_32_byte_records(tmp_path):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(kas_[a-z_0-9]+)\s*\(", src))
    for name in NEW_ENTRIES:
        assert name in declared and name in native.SYMBOLS, name
    assert re.search(r"#define KAS_ABI_VERSION (\d+)", src).group(1) == str(abi.KAS_ABI_VERSION) == "6"
    assert abi.NODE_IMPACT_DTYPE.itemsize == 32 and abi.SCENARIO_IMPACT_DTYPE.itemsize == 32
    assert C.sizeof(abi.ImpactTables) == 16
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kas_abi.h"\n'
                     'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(kas_node_impact), sizeof(kas_scenario_impact), '
                     'sizeof(kas_impact_tables), offsetof(kas_node_impact, outbound), offsetof(kas_scenario_impact, max_leaders_after)); '
                     'return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c11", "-I" + os.path.join(ROOT, "include"), str(probe), "-o", str(exe)])
    assert subprocess.check_output([str(exe)], text=True).split() == ["32", "32", "16", "20", "28"]
    assert abi.NODE_IMPACT_DTYPE.fields["outbound"][1] == 20 and abi.SCENARIO_IMPACT_DTYPE.fields["max_leaders_after"][1] == 28


def test_library_exports_the_impact_entries():
    from kafka_assigner_amd import build
    build.build()
    L = native.load()
    for name in NEW_ENTRIES:
        assert hasattr(L, name), name
    assert L.kas_abi_version() == 6
    blob = open(build.LIB, "rb").read()
    assert b"kas_impact_kernel" in blob and b"kas_impact_merge_kernel" in blob

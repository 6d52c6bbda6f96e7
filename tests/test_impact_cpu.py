"""The impact pass (ABI v6, include/kas_abi.h: kas_node_impact / kas_scenario_impact) without a GPU.

- The NumPy checker (tests/impact_ref.py) on the oracle's outputs: its invariants on the Appendix B vectors and random batches.
- The kernel body (kafka-assigner_amd/csrc/kas_impact_body.h) compiled with g++ against tests/emu/kas_wave.h and stepped on
  CPU fibers (tests/emu/impact_driver.cpp) over oracle-produced out tables: equal to the checker for one- and multi-item
  scenarios (the merge kernel), ragged lists, in_partitions flags, a failing topic followed by a skipped one, multi-topic
  scenarios, two scenarios on one node range, both cell layouts and the counters beyond the LDS budget.
- The ABI: the new entry points are declared and exported, the records are 32 bytes.
"""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

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
    _LIB = L
    return L


def emu_impact(fb, ho, cells16=False, cur16=None, node_cap=-1, rows_per_item=0):
    """kas_emu_impact over the tables a solve left in `ho`: ((nodes, scenarios), {items, merges, global_items, node_cap})."""
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
    rc = _emu_lib().kas_emu_impact(C.byref(bd), C.byref(t), int(cells16), int(node_cap), int(rows_per_item),
                                   nodes.ctypes.data, scen.ctypes.data, info, err, 512)
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


def _random_batch(seed, n_scen=4, max_p=600, ragged=True, flags=True):
    """Sparse broker ids (some of the current replicas name brokers outside the set), ragged lists, partition sets that are not
    the keys of the current assignment, one to three topics per scenario."""
    rng = np.random.default_rng(seed)
    scs = []
    for _ in range(n_scen):
        N = int(rng.integers(6, 40))
        R = int(rng.integers(2, 6))
        brokers = sorted(int(b) for b in rng.choice(60, N, replace=False))
        racks = {b: "r%d" % (b % R) for b in brokers}
        topics = []
        for t in range(int(rng.integers(1, 4))):
            P = int(rng.integers(1, max_p))
            rf = int(rng.integers(2, 4))
            cur = {}
            for p in range(P):
                reps = [int(x) for x in rng.choice(70, rf, replace=False)]
                if ragged and rng.random() < 0.15:
                    reps = reps[:int(rng.integers(0, rf))]
                cur[p] = reps
            parts = None
            if flags and rng.random() < 0.5:
                parts = set(range(P)) - {int(x) for x in rng.choice(P, P // 5, replace=False)} | {P + 3, P + 7}
            topics.append(Topic("t%d" % t, cur, rf, partitions=parts))
        scs.append(Scenario(brokers=brokers, racks=racks, topics=topics))
    return flatten(scs)


def _failing_then_skipped_batch():
    """scenario 0: topic 0 has no positive replication factor, so topic 1 is KAS_SKIPPED; scenario 1 is fine"""
    cur_a, cur_b = G.random_assignment(3, 200, 20, 5, 3), G.random_assignment(4, 150, 20, 5, 3)
    a = {p: cur_a[p].tolist() for p in range(200)}
    b = {p: cur_b[p].tolist() for p in range(150)}
    brokers = list(range(20))
    racks = {n: "r%d" % (n % 5) for n in brokers}
    return flatten([Scenario(brokers, racks, [Topic("a", a, 0), Topic("b", b, 3)]),
                    Scenario(brokers, racks, [Topic("a", a, 3), Topic("b", b, 3)])])


def _shared_node_range_batch():
    """two scenarios that read one node range (node_off equal): each gets a block of records of its own"""
    cur = G.random_assignment(5, 400, 20, 5, 3)
    brokers = [b for b in range(22) if b != 4]
    racks = {b: "r%d" % (b % 5) for b in brokers}
    fb = flatten([Scenario(brokers, racks, [Topic("x", {p: cur[p].tolist() for p in range(400)}, 3)]),
                  Scenario(brokers, racks, [Topic("y", {p: cur[(p * 7) % 400].tolist() for p in range(400)}, 3)])])
    fb.scen["node_off"][1] = fb.scen["node_off"][0]
    return fb


def _many_brokers_batch():
    """7,000 brokers: N x 24 bytes of counters do not fit the LDS next to the id table (the global-scratch path)"""
    N, P = 7000, 300
    cur = G.random_assignment(11, P, N + 50, 20, 3)
    brokers = list(range(N))
    return flatten([Scenario(brokers, {b: "r%d" % (b % 20) for b in brokers}, [Topic("big", {p: cur[p].tolist() for p in range(P)}, 3)])])


# ---- the checker on the oracle's outputs ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["appendix_b", "random0", "random1", "failing_then_skipped", "shared_node_range"])
def test_checker_invariants_on_oracle_outputs(name):
    fb = {"appendix_b": _appendix_b_batch, "random0": lambda: _random_batch(100), "random1": lambda: _random_batch(101),
          "failing_then_skipped": _failing_then_skipped_batch, "shared_node_range": _shared_node_range_batch}[name]()
    ho = oracle_solve(fb)
    imp = impact_ref(fb, ho)
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
    ho = oracle_solve(fb)
    want = impact_ref(fb, ho)
    got, info = emu_impact(fb, ho)
    assert info["merges"] > 0 and info["items"] > info["merges"]      # (multi-topic scenarios merge, single-topic ones do not)
    assert_same_impact(want, got, "emulated impact, one item per topic")
    got, info = emu_impact(fb, ho, rows_per_item=97)
    assert info["items"] > fb.n_topics
    assert_same_impact(want, got, "emulated impact, topics cut into items of 97 rows")


def test_emulated_kernel_one_item_scenarios_write_directly():
    fb = _shared_node_range_batch()
    ho = oracle_solve(fb)
    got, info = emu_impact(fb, ho)
    assert info == {"items": 2, "merges": 0, "global_items": 0, "node_cap": 21}
    assert_same_impact(impact_ref(fb, ho), got, "one item per scenario, two scenarios on one node range")
    assert native.node_blocks(fb)[-1] == 42


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
    ho = oracle_solve(fb)
    want = impact_ref(fb, ho)
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
    ho = oracle_solve(fb)
    got, info = emu_impact(fb, ho, node_cap=0)
    assert info["global_items"] == info["items"] and info["merges"] == fb.n_scenarios
    assert_same_impact(impact_ref(fb, ho), got, "global counters (forced)")
    fb = _many_brokers_batch()
    ho = oracle_solve(fb)
    assert int(ho.topic_results["status"][0]) == abi.KAS_OK
    want = impact_ref(fb, ho)
    assert int(want[1]["departed_replicas"][0]) > 0
    for cells16 in (False, True):
        h = solved16(fb)[0] if cells16 else ho
        got, info = emu_impact(fb, h, cells16=cells16)
        assert info["global_items"] == 1 and info["node_cap"] < 7000, info
        assert_same_impact(want, got, "beyond the LDS budget, cells16=%s" % cells16)


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

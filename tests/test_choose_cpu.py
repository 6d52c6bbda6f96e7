"""Choosing the best scenarios (include/kas_abi.h: kas_choose_spec / kas_choice) without a GPU.

- The rank kernel's body (kafka-assigner_amd/csrc/kas_choose_body.h) compiled with g++ against tests/emu/kas_wave.h and stepped on
  CPU fibers (tests/emu/choose_driver.cpp) over synthetic records, against the NumPy checker (tests/choose_ref.py): the S values
  around the workgroup and the LDS tile, every criterion, specs of 2 to 4 criteria, ties everywhere, failed scenarios, every k.
- The gather kernel's body over oracle-solved batches of tests/impact_batches.py: both cell layouts and the narrowing form, k from
  1 to S, a guard behind both capacities.
- The what-if batch of 302 variants (118 of which fail) through both, with the guard that keeps it meaningful.
- The host call planner (csrc/kas_host_call.h) with the choose arguments: refusals, tables, capacities.
- The ABI: entries declared and exported, struct layouts against a compiled probe, version still 6.
"""
import ctypes as C
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from choose_ref import assert_same_choice, choose_ref, criterion, offsets_ref, packed_cells, rank_ref
from impact_batches import solved, whatif_inputs
from impact_ref import impact_ref
from kafka_assigner_amd import abi, native
from kafka_assigner_amd.flatten import batch_desc, index_form
from oracle_lib import oracle_solve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "kafka-assigner_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "kas_abi.h")
E_INVALID = abi.KAS_E_INVALID_ARG
TILE = 1024                                                   # KAS_CHOOSE_TILE
S_VALUES = [1, 2, 63, 64, 65, 255, 256, 257, 1000, 1025, 1500, 2 * TILE + 1]
MULTI_SPECS = [("max_inbound", "moved_replicas"), ("replica_spread", "leader_spread", "leaders_moved"),
               ("replica_spread", "leader_spread", "leaders_moved", "moved_partitions")]
WHATIF_SPECS = [("moved_replicas",), ("max_inbound", "moved_replicas"), ("replica_spread", "leader_spread", "leaders_moved", "moved_partitions")]
SENTINEL = -77
_LIB = None


# ---- the emulator ---------------------------------------------------------------------------------------------------------
def _emu_lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    so = os.path.join(EMU, "libkas_emu_choose.so")
    srcs = [os.path.join(EMU, "choose_driver.cpp"), os.path.join(EMU, "emu_driver.cpp")]
    deps = srcs + [os.path.join(EMU, "kas_wave.h"), HEADER] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        tmp = so + ".tmp%d" % os.getpid()
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unused-parameter", "-Wno-unknown-pragmas",
                               "-I" + os.path.join(ROOT, "tests"), "-I" + CSRC, "-I" + os.path.join(ROOT, "include"),
                               "-o", tmp] + srcs)
        os.replace(tmp, so)
    L = C.CDLL(so)
    L.kas_emu_rank.restype = C.c_int
    L.kas_emu_rank.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(abi.ChooseSpec), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_char_p, C.c_int]
    L.kas_emu_choose.restype = C.c_int
    L.kas_emu_choose.argtypes = [C.POINTER(abi.BatchDesc), C.POINTER(abi.Tables), C.POINTER(abi.ImpactTables), C.c_int,
                                 C.POINTER(abi.ChooseSpec), C.POINTER(abi.Choice), C.c_uint32, C.c_char_p, C.c_int]
    L.kas_emu_choose_host_call.restype = C.c_int
    L.kas_emu_choose_host_call.argtypes = [C.POINTER(abi.BatchDesc), C.POINTER(C.c_int64), C.c_uint, C.c_int, C.POINTER(abi.ChooseSpec),
                                           C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_void_p, C.c_void_p, C.c_int64, C.c_char_p, C.c_int]
    L.kas_emu_choose_buffers.restype = C.c_int
    _LIB = L
    return L


def _spec(keys, k, n_keys=None):
    """kas_choose_spec without abi.choose_spec's own checks (the refusals are the library's to make)"""
    spec = abi.ChooseSpec()
    ids = [abi.KEYS[x] if isinstance(x, str) else int(x) for x in keys]
    spec.n_keys = len(ids) if n_keys is None else n_keys
    for i, v in enumerate(ids[:4]):
        spec.key[i] = v
    spec.k = k
    return spec


def emu_rank(sr, si, keys, k, cells=None, n_nodes=None, lds_fill=0xCDCDCDCD):
    """kas_emu_rank: every output pre-filled with a sentinel.  cells / n_nodes: the size table's columns (offsets are written)"""
    S = int(sr.shape[0])
    got = SimpleNamespace(rank=np.full(S + 1, SENTINEL, np.int32), chosen=np.full(k + 1, SENTINEL, np.int32),
                          row_off=np.full(k + 2, SENTINEL, np.int64), node_off=np.full(k + 2, SENTINEL, np.int64),
                          n_ok=np.full(2, SENTINEL, np.int32))
    sized = cells is not None
    if sized:
        cells, n_nodes = np.ascontiguousarray(cells, np.int64), np.ascontiguousarray(n_nodes, np.int32)
    err = C.create_string_buffer(512)
    spec = _spec(keys, k)
    rc = _emu_lib().kas_emu_rank(sr.ctypes.data, si.ctypes.data, S, C.byref(spec), cells.ctypes.data if sized else None,
                                 n_nodes.ctypes.data if sized else None, got.rank.ctypes.data, got.chosen.ctypes.data,
                                 got.row_off.ctypes.data if sized else None, got.node_off.ctypes.data if sized else None,
                                 got.n_ok.ctypes.data, lds_fill, err, 512)
    assert rc == 0, (rc, err.value.decode())
    # one element behind every array is a guard
    assert got.rank[S] == SENTINEL and got.chosen[k] == SENTINEL and got.n_ok[1] == SENTINEL
    assert got.row_off[k + 1] == SENTINEL and got.node_off[k + 1] == SENTINEL
    got.rank, got.chosen, got.n_ok = got.rank[:S], got.chosen[:k], int(got.n_ok[0])
    got.row_off, got.node_off = got.row_off[:k + 1], got.node_off[:k + 1]
    return got


GUARD_CELLS, GUARD_NODES = 64, 3


def emu_choose(fb, out, sr, imp, keys, k, mode=0, lds_fill=0xCDCDCDCD):
    """kas_emu_choose over the tables of a solve (`out`: the out pool, every row in place; mode 0 int32 cells, 1 uint16 cells, 2
    int32 cells gathered into uint16 rows) and its impact records: the choice, capacities exactly the k largest scenarios', with
    guard cells / records behind them checked here."""
    S = fb.n_scenarios
    nodes, si = imp
    bd = batch_desc(fb)
    t = abi.Tables()
    t.out = out.ctypes.data
    t.scenario_results = sr.ctypes.data
    itab = abi.ImpactTables(nodes.ctypes.data if nodes.size else None, si.ctypes.data)
    rows_cap = int(np.sort(packed_cells(fb))[::-1][:k].sum())
    nodes_cap = int(np.sort(np.clip(fb.scen["n_nodes"], 0, None).astype(np.int64))[::-1][:k].sum())
    dt = np.int32 if mode == 0 else np.uint16
    got = SimpleNamespace(rank=np.full(S, SENTINEL, np.int32), chosen=np.full(max(k, 1), SENTINEL, np.int32),
                          row_off=np.full(k + 1, SENTINEL, np.int64), node_off=np.full(k + 1, SENTINEL, np.int64),
                          n_ok=np.full(1, SENTINEL, np.int32), rows=np.full(rows_cap + GUARD_CELLS, 0x7B7B, dt),
                          nodes=np.zeros(nodes_cap + GUARD_NODES, abi.NODE_IMPACT_DTYPE))
    raw_nodes = got.nodes.view(np.uint8)
    raw_nodes[...] = 0x7B
    ch = abi.Choice(got.rank.ctypes.data, got.chosen.ctypes.data, got.row_off.ctypes.data, got.node_off.ctypes.data, got.n_ok.ctypes.data,
                    got.rows.ctypes.data, rows_cap, got.nodes.ctypes.data, nodes_cap)
    err = C.create_string_buffer(512)
    spec = _spec(keys, k)
    rc = _emu_lib().kas_emu_choose(C.byref(bd), C.byref(t), C.byref(itab), mode, C.byref(spec), C.byref(ch), lds_fill, err, 512)
    assert rc == 0, (rc, err.value.decode())
    used, recs = int(got.row_off[k]), int(got.node_off[k])
    assert 0 <= used <= rows_cap and 0 <= recs <= nodes_cap
    assert (got.rows[used:] == 0x7B7B).all(), "cells behind row_off[k] (the guard behind rows_cap among them) were written"
    assert (raw_nodes[32 * recs:] == 0x7B).all(), "records behind node_off[k] (the guard behind nodes_cap among them) were written"
    got.chosen, got.n_ok = got.chosen[:k], int(got.n_ok[0])
    return got


# ---- synthetic records ----------------------------------------------------------------------------------------------------
def synthetic(S, seed, values=4, failed="alternate"):
    """S scenario records and impact records whose criteria are drawn from `values` (an int: 0..values-1; a list: those values):
    most scenarios tie on every criterion.  failed: 'none', 'alternate' (every second scenario), 'all', 'random'."""
    rng = np.random.default_rng([seed, S])
    pool = np.arange(values) if isinstance(values, int) else np.asarray(values, dtype=np.int64)
    draw = lambda: pool[rng.integers(0, pool.size, S)]
    sr = np.zeros(S, abi.SCENARIO_RESULT_DTYPE)
    si = np.zeros(S, abi.SCENARIO_IMPACT_DTYPE)
    status = {"none": np.zeros(S, np.int32), "alternate": (np.arange(S) % 2) * abi.KAS_FAIL_UNASSIGNABLE,
              "all": np.full(S, abi.KAS_FAIL_RF_GT_BROKERS), "random": rng.integers(0, 3, S) * (rng.integers(0, 2, S))}[failed]
    sr["status"] = status
    sr["fail_topic"] = np.where(status != 0, 0, -1)
    sr["moved_replicas"], sr["moved_partitions"] = draw(), draw()
    sr["digest"] = rng.integers(0, 2**63, S).astype(np.uint64)
    for f in ("departed_replicas", "leaders_moved", "max_inbound", "max_outbound", "max_replicas_after", "max_leaders_after"):
        si[f] = draw()
    # spreads: max - min, itself one of the pool's values
    si["min_replicas_after"] = si["max_replicas_after"] - np.minimum(draw(), si["max_replicas_after"])
    si["min_leaders_after"] = si["max_leaders_after"] - np.minimum(draw(), si["max_leaders_after"])
    return sr, si


def _check_rank(sr, si, keys, k, what, sized=True, lds_fill=0xCDCDCDCD):
    S = int(sr.shape[0])
    rng = np.random.default_rng(S + k)
    cells = rng.integers(0, 7, S) * 3 + (np.arange(S) % 5 == 0) if sized else None       # (odd sizes and zeros among them)
    n_nodes = rng.integers(0, 50, S) if sized else None
    want = rank_ref(sr, si, keys, k)
    got = emu_rank(sr, si, keys, k, cells, n_nodes, lds_fill=lds_fill)
    assert got.n_ok == want.n_ok, (what, got.n_ok, want.n_ok)
    assert np.array_equal(got.rank, want.rank), (what, "rank", np.nonzero(got.rank != want.rank)[0][:5])
    assert np.array_equal(got.chosen, want.chosen), (what, "chosen", got.chosen[:8], want.chosen[:8])
    if sized:
        assert np.array_equal(got.row_off, offsets_ref(want.order, cells, k)), (what, "row_off")
        assert np.array_equal(got.node_off, offsets_ref(want.order, n_nodes, k)), (what, "node_off")
    return want


def _ks(S, n_ok):
    return sorted({k for k in (0, 1, n_ok - 1, n_ok, n_ok + 1, S) if 0 <= k <= S})


@pytest.mark.parametrize("S", S_VALUES)
def test_emulated_rank_every_criterion_and_spec(S):
    """every single criterion and specs of 2, 3 and 4 criteria, criteria drawn from {0..3}: the index decides most comparisons"""
    sr, si = synthetic(S, 1, failed="random")
    n_ok = int((sr["status"] == 0).sum())
    for keys in [(name,) for name in abi.KEY_NAMES] + MULTI_SPECS:
        want = _check_rank(sr, si, keys, min(S, max(n_ok - 1, 0)), f"S={S} {keys}")
        if S >= 64 and n_ok >= 16:                                # (the batch does tie: the guard of this test)
            first = criterion(sr, si, keys[0])[want.order]
            assert np.unique(first).size <= 4 < first.size
    # rank only (kas_rank_device: no size table, no offsets)
    _check_rank(sr, si, MULTI_SPECS[0], min(S, 3), f"S={S} rank only", sized=False)


@pytest.mark.parametrize("S", S_VALUES)
@pytest.mark.parametrize("failed", ["none", "alternate", "all"])
def test_emulated_rank_failed_scenarios_and_every_k(S, failed):
    sr, si = synthetic(S, 2, failed=failed)
    n_ok = int((sr["status"] == 0).sum())
    assert n_ok == {"none": S, "alternate": (S + 1) // 2, "all": 0}[failed]
    for k in _ks(S, n_ok):
        want = _check_rank(sr, si, ("leaders_moved", "max_outbound"), k, f"S={S} failed={failed} k={k}")
        if failed == "all":
            assert want.n_ok == 0 and (want.chosen == -1).all() and (want.rank == -1).all()


@pytest.mark.parametrize("S", [1, 65, 257, 1025])
def test_emulated_rank_all_keys_equal(S):
    """all keys equal: the rank is the position among the OK scenarios"""
    for failed in ("none", "alternate"):
        sr, si = synthetic(S, 3, values=[5], failed=failed)
        ok = np.nonzero(sr["status"] == 0)[0]
        for keys in (("moved_replicas",), MULTI_SPECS[2]):
            got = emu_rank(sr, si, keys, S)
            assert np.array_equal(got.rank[ok], np.arange(ok.size)) and np.array_equal(got.chosen[:ok.size], ok)
            _check_rank(sr, si, keys, S, f"S={S} equal keys")


@pytest.mark.parametrize("S", [2, 257, 1025])
def test_emulated_rank_extreme_values(S):
    """criterion values at 0 and at 2^31 - 1"""
    sr, si = synthetic(S, 4, values=[0, 2**31 - 1], failed="alternate")
    for keys in [(name,) for name in abi.KEY_NAMES] + MULTI_SPECS:
        assert set(np.unique(criterion(sr, si, keys[0]))) <= {0, 2**31 - 1}
        _check_rank(sr, si, keys, S, f"S={S} extremes {keys}")
    sr, si = synthetic(S, 5, values=[2**31 - 1], failed="random")           # every key at the top, among failed scenarios
    _check_rank(sr, si, MULTI_SPECS[2], S, f"S={S} every criterion 2^31 - 1")


@pytest.mark.parametrize("fill", [0, 0xFFFFFFFF, 0x00000001, 0xCDCDCDCD])
def test_emulated_rank_whatever_the_lds_holds(fill):
    """LDS is uninitialised on hardware: zeros (the smallest key, OK flag clear), all ones, an OK flag set everywhere"""
    for S in (65, 1025, 1500):
        sr, si = synthetic(S, 6, failed="random")
        _check_rank(sr, si, MULTI_SPECS[1], S // 2, f"S={S} lds {fill:#x}", lds_fill=fill)


def test_emulated_rank_refuses_bad_specs():
    sr, si = synthetic(8, 7)
    L = _emu_lib()
    out = np.zeros(16, np.int32)
    for spec, text in ((_spec(("moved_replicas",), 1, n_keys=0), "n_keys outside 1..4"), (_spec(("moved_replicas",), 1, n_keys=5), "n_keys outside 1..4"),
                       (_spec((10,), 1), "unknown criterion"), (_spec((0, -1), 1), "unknown criterion"),
                       (_spec(("moved_replicas",), -1), "k outside"), (_spec(("moved_replicas",), 9), "k outside")):
        err = C.create_string_buffer(256)
        rc = L.kas_emu_rank(sr.ctypes.data, si.ctypes.data, 8, C.byref(spec), None, None, out.ctypes.data, out.ctypes.data, None, None,
                            out.ctypes.data, 0, err, 256)
        assert rc == E_INVALID and text in err.value.decode(), (rc, err.value.decode(), text)


# ---- the gather kernel over oracle-solved batches -------------------------------------------------------------------------
def _forms(fb, ho):
    """(mode, out pool, the out pool the checker slices) for int32 cells, 16-bit cells and the narrowing gather"""
    ho_idx = oracle_solve(index_form(fb))                                   # int32 node indices, -1 pads: a widened solve's out pool
    out16 = np.where(ho_idx.out < 0, abi.KAS_CELL16_NONE, ho_idx.out).astype(np.uint16)
    return [(0, ho.out, ho.out), (1, out16, out16), (2, ho_idx.out, out16)]


@pytest.mark.parametrize("name", ["mixed42", "row_counts", "shared_node_range", "degenerate", "widths_4_5"])
def test_emulated_gather_equals_checker(name):
    """multi-topic scenarios, scenarios of different (and odd) sizes, topics narrower than the batch, a scenario without topics and
    one that fails: packed rows and node blocks cell for cell, for every k from 1 to S"""
    fb, ho, imp = solved(name)
    S = fb.n_scenarios
    sizes = packed_cells(fb)
    if name in ("mixed42", "row_counts"):
        assert (sizes % 2 == 1).any() and np.unique(sizes).size > 2         # odd sizes: later scenarios land misaligned
    if name in ("mixed42", "degenerate", "widths_4_5"):
        assert (fb.scen["topic_count"] > 1).any()
    for mode, out, ref_out in _forms(fb, ho):
        for k in range(1, S + 1):
            for keys in (("moved_replicas",), ("leaders_moved", "max_inbound")) if k in (1, S) else (("max_inbound", "moved_replicas"),):
                want = choose_ref(fb, ho.scenario_results, ref_out, imp, keys, k)
                got = emu_choose(fb, out, ho.scenario_results[:S], imp, keys, k, mode=mode)
                assert_same_choice(want, got, f"{name} mode {mode} k {k} {keys}")
    # k = 0 ranks only
    got = emu_choose(fb, ho.out, ho.scenario_results[:S], imp, ("moved_replicas",), 0)
    assert_same_choice(choose_ref(fb, ho.scenario_results, ho.out, imp, ("moved_replicas",), 0), got, f"{name} k 0")


# ---- the what-if batch: variants that fail and tie ------------------------------------------------------------------------
def whatif_variants():
    from kafka_assigner_amd.whatif import Variant, WhatIf
    brokers, topics = whatif_inputs()
    w = WhatIf(brokers, topics)
    rng = np.random.default_rng(3)
    vs = [Variant(label="as is"), Variant(label="as is again")]
    for i in range(298):
        k = int(rng.integers(0, 5)); a = int(rng.integers(0, 4))
        rem = sorted(rng.choice(60, size=k, replace=False).tolist())
        add = {60 + j: "r%d" % int(rng.integers(0, 6)) for j in range(a)}
        vs.append(Variant(remove=rem, add=add, rack_aware=bool(rng.integers(0, 8) != 0)))
    vs += [Variant(remove=[b for b in range(60) if b % 6 != 0]), Variant(remove=[b for b in range(60) if b % 6 > 1])]
    return w, vs


_WHATIF = None


def whatif_solved():
    """(WhatIf, variants, fb, the oracle's solve, the checker's impact records) of the what-if batch, computed once, with its guard:
    at least 100 variants solve, at least 50 fail, and at least 20 solved ones tie on the first criterion of every spec used"""
    global _WHATIF
    if _WHATIF is None:
        w, vs = whatif_variants()
        fb = w.flat_batch(vs)
        ho = oracle_solve(fb)
        imp = impact_ref(fb, ho)
        sr = ho.scenario_results[:fb.n_scenarios]
        ok = sr["status"] == abi.KAS_OK
        assert len(vs) == 302 and ok.sum() >= 100 and (~ok).sum() >= 50, (int(ok.sum()), int((~ok).sum()))
        for keys in WHATIF_SPECS:
            v, n = np.unique(criterion(sr, imp[1], keys[0])[ok], return_counts=True)
            assert int(n[n > 1].sum()) >= 20, (keys, "too few solved variants tie on the first criterion")
        _WHATIF = (w, vs, fb, ho, imp)
    return _WHATIF


def own_cur_form(fb):
    """The same batch with a cur table per scenario.  16-bit cells are node indices of the scenario's own broker set, so the
    what-if layout (every scenario reads ONE cur table) has no 16-bit form (flatten.to_cells16 refuses it): a caller of the 16-bit
    entries lays the snapshot out once per variant.  Same scenarios, same rows out, same records."""
    import dataclasses
    S, n = fb.n_scenarios, int(fb.cur.shape[0])
    topics = fb.topics.copy()
    for s in range(S):
        b, c = int(fb.scen["topic_begin"][s]), int(fb.scen["topic_count"][s])
        topics["cur_off"][b:b + c] += s * n
    return dataclasses.replace(fb, topics=topics, cur=np.tile(fb.cur, S))


def test_emulated_choice_of_the_whatif_batch():
    _, _, fb, ho, imp = whatif_solved()
    S = fb.n_scenarios
    n_ok = int((ho.scenario_results["status"][:S] == 0).sum())
    for keys, ks in ((WHATIF_SPECS[0], (5,)), (WHATIF_SPECS[1], (1, 5, n_ok, n_ok + 1, S)), (WHATIF_SPECS[2], (5,))):
        for k in ks:
            want = choose_ref(fb, ho.scenario_results, ho.out, imp, keys, k)
            got = emu_choose(fb, ho.out, ho.scenario_results[:S], imp, keys, k)
            assert_same_choice(want, got, f"what-if {keys} k {k}")
    # "as is" appears twice and ties with itself: the earlier variant wins
    got = emu_choose(fb, ho.out, ho.scenario_results[:S], imp, ("moved_replicas", "leaders_moved"), 2)
    assert got.chosen.tolist() == [0, 1]


# ---- the planner ----------------------------------------------------------------------------------------------------------
HOST_BUFS = ("cur", "out", "aux", "ctx", "cur16", "out16", "tr", "sr", "tr_pin", "sr_pin", "imp_nodes", "imp_scen",
             "ch_sizes", "ch_segs", "ch_head", "ch_rows", "ch_nodes", "ch_head_pin", "ch_rows_pin", "ch_nodes_pin")
MISSING = {"cur": 1, "aux": 4, "ctx": 8, "topic_results": 16, "scenario_results": 32, "imp_scenarios": 128, "rank": 256, "chosen": 512,
           "row_off": 1024, "node_off": 2048, "n_ok": 4096, "rows": 8192, "nodes": 16384}


def k_largest(fb, k):
    return (int(np.sort(packed_cells(fb))[::-1][:max(k, 0)].sum()),
            int(np.sort(np.clip(fb.scen["n_nodes"], 0, None).astype(np.int64))[::-1][:max(k, 0)].sum()))


def choose_host_call(fb, spec, rows_cap=None, nodes_cap=None, missing=(), cells16=False):
    """kas_plan_host_call for a kas_solve_host_choose call: (return code, plan or None, error text)"""
    L = _emu_lib()
    assert L.kas_emu_choose_buffers() == len(HOST_BUFS)
    bd = batch_desc(fb)
    if cells16:
        bd.node_id = None
    need = k_largest(fb, spec.k)
    lens = (C.c_int64 * 5)(int(fb.cur.shape[0]), int(fb.aux.shape[0]), int(fb.ctx.shape[0]), need[0] if rows_cap is None else rows_cap,
                           need[1] if nodes_cap is None else nodes_cap)
    head, nbytes = (C.c_int64 * 8)(), (C.c_int64 * len(HOST_BUFS))()
    sizes = np.zeros((fb.n_scenarios + 1, 5), np.int64)
    segs = np.zeros((fb.n_topics + 1, 3), np.int64)
    err = C.create_string_buffer(512)
    rc = L.kas_emu_choose_host_call(C.byref(bd), lens, sum(MISSING[m] for m in missing), int(cells16), C.byref(spec), head, nbytes,
                                    sizes.ctypes.data, segs.ctypes.data, fb.n_topics, err, 512)
    if rc != 0:
        return rc, None, err.value.decode()
    names = ("rows_need", "nodes_need", "chunks", "head_bytes", "segments", "K", "native16", "S")
    plan = dict(zip(names, [int(v) for v in head]))
    plan.update(bytes=dict(zip(HOST_BUFS, [int(v) for v in nbytes])), sizes=sizes[:fb.n_scenarios], segs=segs[:plan["segments"]])
    return rc, plan, ""


def test_planner_refuses_in_order_each_with_its_text():
    fb, _, _ = solved("mixed42")
    S = fb.n_scenarios
    good = ("moved_replicas", "leaders_moved")
    rows, nodes = k_largest(fb, 2)
    cases = [
        (dict(spec=_spec(good, 2, n_keys=0)), "n_keys outside 1..4"),
        (dict(spec=_spec(good, 2, n_keys=5)), "n_keys outside 1..4"),
        (dict(spec=_spec((0, 10), 2)), "unknown criterion"),
        (dict(spec=_spec((-1,), 2)), "unknown criterion"),
        (dict(spec=_spec(good, -1)), "k outside"),
        (dict(spec=_spec(good, S + 1)), "k outside"),
        (dict(spec=_spec(good, 2), rows_cap=rows - 1), "rows_cap below"),
        (dict(spec=_spec(good, 2), nodes_cap=nodes - 1), "nodes_cap below"),
    ] + [(dict(spec=_spec(good, 2), missing=(m,)), "an array the call writes is NULL") for m in ("rank", "chosen", "row_off", "node_off", "n_ok", "rows", "nodes")]
    for kw, text in cases:
        rc, plan, err = choose_host_call(fb, **kw)
        assert rc == E_INVALID and text in err, (kw, rc, err)
    # the order of the refusals: the earlier one is reported when several apply
    order = [(dict(spec=_spec((10,), -1, n_keys=0), rows_cap=0, nodes_cap=0, missing=("rank",)), "n_keys outside"),
             (dict(spec=_spec((10,), -1), rows_cap=0, nodes_cap=0, missing=("rank",)), "unknown criterion"),
             (dict(spec=_spec(good, -1), rows_cap=0, nodes_cap=0, missing=("rank",)), "k outside"),
             (dict(spec=_spec(good, 2), rows_cap=0, nodes_cap=0, missing=("rank",)), "rows_cap below"),
             (dict(spec=_spec(good, 2), nodes_cap=0, missing=("rank",)), "nodes_cap below"),
             (dict(spec=_spec(good, 2), missing=("rank",)), "is NULL")]
    for kw, text in order:
        rc, _, err = choose_host_call(fb, **kw)
        assert rc == E_INVALID and text in err, (kw, err)
    # the impact scenarios and the records are still asked for; out and the node table are not
    rc, _, err = choose_host_call(fb, _spec(good, 2), missing=("imp_scenarios",))
    assert rc == E_INVALID and "kas_impact_tables" in err
    rc, _, err = choose_host_call(fb, _spec(good, 2), missing=("scenario_results",))
    assert rc == E_INVALID
    # k = 0 ranks only: no chosen, rows or nodes array is needed
    rc, plan, err = choose_host_call(fb, _spec(good, 0), missing=("chosen", "rows", "nodes"))
    assert rc == 0 and plan["rows_need"] == 0 and plan["nodes_need"] == 0, err


def test_planner_capacities_at_and_below_the_k_largest_bound():
    fb, _, _ = solved("mixed42")
    for k in (1, 3, fb.n_scenarios):
        rows, nodes = k_largest(fb, k)
        spec = _spec(("max_inbound",), k)
        rc, plan, err = choose_host_call(fb, spec, rows_cap=rows, nodes_cap=nodes)
        assert rc == 0 and (plan["rows_need"], plan["nodes_need"]) == (rows, nodes), err
        assert choose_host_call(fb, spec, rows_cap=rows - 1, nodes_cap=nodes)[0] == E_INVALID
        assert choose_host_call(fb, spec, rows_cap=rows, nodes_cap=nodes - 1)[0] == E_INVALID
        assert choose_host_call(fb, spec, rows_cap=rows + 5, nodes_cap=nodes + 5)[0] == 0


@pytest.mark.parametrize("cells16", [False, True], ids=["int32", "cells16"])
def test_planner_tables_of_a_multi_topic_batch(cells16):
    fb, _, _ = solved("mixed42")
    S, k = fb.n_scenarios, 3
    rc, plan, err = choose_host_call(fb, _spec(("moved_replicas",), k), cells16=cells16)
    assert rc == 0, err
    sizes, segs = plan["sizes"], plan["segs"]
    assert (fb.scen["topic_count"] > 1).any() and plan["segments"] == fb.n_topics
    assert np.array_equal(sizes[:, 0], packed_cells(fb))
    assert np.array_equal(sizes[:, 1], native.node_blocks(fb)[:-1]) and np.array_equal(sizes[:, 2], fb.scen["n_nodes"])
    assert np.array_equal(sizes[:, 3], fb.scen["topic_begin"]) and np.array_equal(sizes[:, 4], fb.scen["topic_count"])
    # segments: the descriptors' own out offsets (the device pools are rebased so that they apply), packed one behind the other
    assert np.array_equal(segs[:, 0], fb.topics["out_off"])
    assert np.array_equal(segs[:, 1], fb.topics["n_partitions"].astype(np.int64) * fb.topics["out_width"])
    for s in range(S):
        b, c = int(fb.scen["topic_begin"][s]), int(fb.scen["topic_count"][s])
        assert np.array_equal(segs[b:b + c, 2], np.concatenate([[0], np.cumsum(segs[b:b + c, 1])])[:c])
    cell = 2 if cells16 else 4
    by = plan["bytes"]
    assert by["ch_sizes"] == 32 * (S + 1) and by["ch_segs"] == 32 * (fb.n_topics + 1)
    assert by["ch_head"] == by["ch_head_pin"] == plan["head_bytes"] == 16 * (k + 1) + 4 * S + 4 * k + 4
    assert by["ch_rows"] == by["ch_rows_pin"] == cell * (plan["rows_need"] + 8)
    assert by["ch_nodes"] == by["ch_nodes_pin"] == 32 * (plan["nodes_need"] + 1)
    assert by["imp_nodes"] == 32 * (int(native.node_blocks(fb)[-1]) + 1) and by["imp_scen"] == 32 * (S + 1)      # they stay on the device
    assert plan["chunks"] == -(-int(packed_cells(fb).max()) * cell // 16384) + -(-int(fb.scen["n_nodes"].max()) * 32 // 16384)
    # the other host calls reserve none of the choice's buffers
    import emu_lib
    rc, other, _ = emu_lib.host_call(fb, select=[], impact=True, cells16=cells16)
    assert rc == 0 and set(other["bytes"]) == set(HOST_BUFS[:12])
    assert {n: by[n] for n in HOST_BUFS[:12]} == other["bytes"]


@pytest.mark.parametrize("S,K", [(40, 1), (44, 2)])
def test_planner_scenario_ranges_of_a_choice(S, K):
    """S x 100k x 3 cells with a `cur` per scenario: a choice uploads cur and downloads no out table, so 48.0 MB (S = 40) stay one
    range where kas_solve_host_impact's 96 MB are cut, and 52.8 MB (S = 44) are cut into two; the tables cover the whole call"""
    from kafka_assigner_amd import generator as G
    from kafka_assigner_amd.flatten import node_set_batch
    P, N, R = 100_000, 200, 10
    sets = [G.scenario_action(61, s, N, R, actions=G.BENCH_ACTIONS)[1] for s in range(S)]
    fb = node_set_batch([b.node_id for b in sets], [b.node_rack for b in sets], P, 3, 3, cur=np.zeros((S, P, 3), np.int32))
    rc, plan, err = choose_host_call(fb, _spec(("moved_replicas",), 3))
    assert rc == 0 and plan["K"] == K, (err, plan and plan["K"])
    assert plan["sizes"].shape[0] == S and (plan["sizes"][:, 0] == 3 * P).all() and plan["rows_need"] == 9 * P
    assert np.array_equal(plan["segs"][:, 0], fb.topics["out_off"])


# ---- ABI ------------------------------------------------------------------------------------------------------------------
def test_abi_declares_the_choose_entries_and_layouts(tmp_path):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(kas_[a-z_0-9]+)\s*\(", src))
    for name in abi.CHOOSE_ENTRIES:
        assert name in declared and name in native.SYMBOLS, name
    assert re.search(r"#define KAS_ABI_VERSION (\d+)", src).group(1) == str(abi.KAS_ABI_VERSION) == "6"
    probe = tmp_path / "probe.c"
    fields = ["rank", "chosen", "row_off", "node_off", "n_ok", "rows", "rows_cap", "nodes", "nodes_cap"]
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kas_abi.h"\nint main(void) {\n'
                     '  printf("%zu %zu %zu %zu %zu\\n", sizeof(kas_choose_spec), offsetof(kas_choose_spec, n_keys), offsetof(kas_choose_spec, key), '
                     'offsetof(kas_choose_spec, k), sizeof(kas_choice));\n'
                     + "".join('  printf("%%zu\\n", offsetof(kas_choice, %s));\n' % f for f in fields)
                     + "".join('  printf("%%d\\n", KAS_KEY_%s);\n' % n.upper() for n in abi.KEY_NAMES)
                     + '  printf("%d %d\\n", KAS_KEY_COUNT, KAS_CHOOSE_MAX_KEYS);\n  return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c11", "-I" + os.path.join(ROOT, "include"), str(probe), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)], text=True).splitlines()
    assert lines[0].split() == [str(C.sizeof(abi.ChooseSpec)), str(abi.ChooseSpec.n_keys.offset), str(abi.ChooseSpec.key.offset),
                                str(abi.ChooseSpec.k.offset), str(C.sizeof(abi.Choice))]
    assert [int(v) for v in lines[1:10]] == [getattr(abi.Choice, f).offset for f in fields]
    assert [int(v) for v in lines[10:20]] == [abi.KEYS[n] for n in abi.KEY_NAMES] == list(range(10))
    assert lines[20].split() == [str(abi.KAS_KEY_COUNT), str(abi.KAS_CHOOSE_MAX_KEYS)]
    with pytest.raises(ValueError):
        abi.choose_spec(("moved_replicas", "no_such_criterion"), 1)


def test_library_exports_the_choose_entries():
    from kafka_assigner_amd import build
    build.build()
    L = native.load()
    for name in abi.CHOOSE_ENTRIES:
        assert hasattr(L, name), name
    assert L.kas_abi_version() == 6
    blob = open(build.LIB, "rb").read()
    assert b"kas_rank_kernel" in blob and b"kas_gather_kernel" in blob
    assert "kas_choose.hip" in build.SOURCES

"""Ranking and fronting by rack criteria (include/kas_abi.h: KAS_KEY_RACK_BASE, the *_racks entries) without a GPU.

- The instances of the rank, mark and front rank kernels' bodies that read the scenario rack records (kas_choose_body.h /
  kas_front_body.h with kasc::RackRecords), compiled with g++ against tests/emu/kas_wave.h and stepped on CPU fibers
  (tests/emu/rack_choose_driver.cpp) over synthetic records, against the NumPy checker (tests/rack_choose_ref.py): the S values
  around the wavefront, the workgroup and the LDS tile, every rack key alone, specs mixing broker and rack keys, extremes, every
  k, failed scenarios, two LDS patterns, bounds on rack keys inside and outside the spec, and the parent code path's bytes for
  broker keys.
- The what-if batch of 302 variants with the report table of WhatIf.report_racks, each test with the guard that keeps it meaningful.
- Refusals in their order, the host call planner (the combined call's decisions, the existing calls' bytes), the ABI, the exports,
  and WhatIf.best / WhatIf.front over the emulator.
"""
import ctypes as C
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import rack_choose_ref as R
import test_choose_cpu as tc
import test_front_cpu as tf
import test_moves_cpu as tm
import test_racks_cpu as tr
from choose_ref import assert_same_choice, offsets_ref
from front_ref import DOMINATED, NOT_OK, OVER_LIMIT, assert_same_front, cut
from impact_batches import solved
from kafka_assigner_amd import abi, native
from kafka_assigner_amd.flatten import batch_desc
from rack_ref import rack_counts, rack_ref
from test_choose_cpu import SENTINEL, k_largest, own_cur_form, synthetic, whatif_solved

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "kafka-assigner_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "kas_abi.h")
E_INVALID, E_UNSUPPORTED = abi.KAS_E_INVALID_ARG, abi.KAS_E_UNSUPPORTED
TOP = 2**31 - 1
S_VALUES = [1, 2, 63, 64, 65, 255, 256, 257, 1025, 2049]
RACK_NAMES = abi.RACK_KEY_NAMES
MIXED = [("colocated_after", "replica_spread"), ("max_inbound", "rack_replica_spread", "new_rack_replicas"),
         ("rack_leader_spread", "leader_spread", "rows_losing_racks", "moved_partitions"), ("moved_replicas", "single_rack_rows_after")]
NO_RECORDS = "rack criterion without rack records"
_LIB = None


# ---- the emulator ---------------------------------------------------------------------------------------------------------
def _emu_lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    so = os.path.join(EMU, "libkas_emu_rack_choose.so")
    srcs = [os.path.join(EMU, "rack_choose_driver.cpp"), os.path.join(EMU, "emu_driver.cpp")]
    deps = srcs + [os.path.join(EMU, "kas_wave.h"), HEADER] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        tmp = so + ".tmp%d" % os.getpid()
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unused-parameter", "-Wno-unknown-pragmas",
                               "-I" + os.path.join(ROOT, "tests"), "-I" + CSRC, "-I" + os.path.join(ROOT, "include"),
                               "-o", tmp] + srcs)
        os.replace(tmp, so)
    L = C.CDLL(so)
    L.kas_emu_rack_rank.restype = C.c_int
    L.kas_emu_rack_rank.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(abi.FrontSpec), C.POINTER(abi.ChooseSpec), C.c_int] + \
        [C.c_void_p] * 8 + [C.c_uint32, C.c_char_p, C.c_int]
    L.kas_emu_rack_choose.restype = C.c_int
    L.kas_emu_rack_choose.argtypes = [C.POINTER(abi.BatchDesc), C.POINTER(abi.Tables), C.POINTER(abi.ImpactTables), C.c_void_p, C.c_int,
                                      C.POINTER(abi.FrontSpec), C.POINTER(abi.ChooseSpec), C.POINTER(abi.Choice), C.c_void_p, C.c_uint32,
                                      C.c_char_p, C.c_int]
    L.kas_emu_rack_choose_host_call.restype = C.c_int
    L.kas_emu_rack_choose_host_call.argtypes = [C.POINTER(abi.BatchDesc), C.POINTER(C.c_int64), C.c_uint, C.c_int, C.POINTER(abi.FrontSpec),
                                                C.POINTER(abi.ChooseSpec), C.POINTER(abi.Moves), C.c_int, C.c_int, C.c_void_p,
                                                C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_char_p, C.c_int]
    L.kas_emu_rack_choose_buffers.restype = C.c_int
    _LIB = L
    return L


def _id(x):
    return abi.rack_key_id(x) if isinstance(x, str) else int(x)


def _cspec(keys, k, n_keys=None):
    """kas_choose_spec without abi's own checks (the refusals are the library's to make)"""
    spec = abi.ChooseSpec()
    ids = [_id(x) for x in keys]
    spec.n_keys = len(ids) if n_keys is None else n_keys
    for i, v in enumerate(ids[:4]):
        spec.key[i] = v
    spec.k = k
    return spec


def _fspec(keys, k, within=(), n_keys=None, n_limits=None):
    spec = abi.FrontSpec()
    ids = [_id(x) for x in keys]
    spec.n_keys = len(ids) if n_keys is None else n_keys
    for i, v in enumerate(ids[:4]):
        spec.key[i] = v
    pairs = list(within.items()) if isinstance(within, dict) else list(within)
    spec.n_limits = len(pairs) if n_limits is None else n_limits
    for i, (name, limit) in enumerate(pairs[:4]):
        spec.limit_key[i] = _id(name)
        spec.limit[i] = limit
    spec.k = k
    return spec


def emu_rack_rank(sr, si, srk, keys, k, within=None, cells=None, n_nodes=None, lds_fill=0xCDCDCDCD, path=0):
    """kas_emu_rack_rank: a ranking (within is None) or a front; every output pre-filled with a sentinel, one element behind every
    array a guard"""
    S = int(sr.shape[0])
    front = within is not None
    got = SimpleNamespace(rank=np.full(S + 1, SENTINEL, np.int32), chosen=np.full(k + 1, SENTINEL, np.int32),
                          row_off=np.full(k + 2, SENTINEL, np.int64), node_off=np.full(k + 2, SENTINEL, np.int64),
                          n_ok=np.full(2, SENTINEL, np.int32), counts=np.full(5, SENTINEL, np.int32))
    sized = cells is not None
    if sized:
        cells, n_nodes = np.ascontiguousarray(cells, np.int64), np.ascontiguousarray(n_nodes, np.int32)
    err = C.create_string_buffer(512)
    fs, cs = (_fspec(keys, k, within), None) if front else (None, _cspec(keys, k))
    rc = _emu_lib().kas_emu_rack_rank(sr.ctypes.data, si.ctypes.data, None if srk is None else srk.ctypes.data, S,
                                      None if fs is None else C.byref(fs), None if cs is None else C.byref(cs), path,
                                      cells.ctypes.data if sized else None, n_nodes.ctypes.data if sized else None, got.rank.ctypes.data,
                                      got.chosen.ctypes.data, got.row_off.ctypes.data if sized else None,
                                      got.node_off.ctypes.data if sized else None, got.n_ok.ctypes.data,
                                      got.counts.ctypes.data if front else None, lds_fill, err, 512)
    assert rc == 0, (rc, err.value.decode())
    assert got.rank[S] == SENTINEL and got.chosen[k] == SENTINEL and got.n_ok[1] == SENTINEL and got.counts[4] == SENTINEL
    assert got.row_off[k + 1] == SENTINEL and got.node_off[k + 1] == SENTINEL
    if not front:
        assert (got.counts == SENTINEL).all()
    got.rank, got.chosen, got.n_ok, got.counts = got.rank[:S], got.chosen[:k], int(got.n_ok[0]), got.counts[:4]
    got.row_off, got.node_off = (got.row_off[:k + 1], got.node_off[:k + 1]) if sized else (None, None)
    return got


def emu_refusal(sr, si, srk, keys, k, within=None, **kw):
    """(rc, text) of kas_emu_rack_rank for a spec built without checks"""
    out = np.zeros(16, np.int32)
    err = C.create_string_buffer(256)
    fs, cs = (_fspec(keys, k, within, **kw), None) if within is not None else (None, _cspec(keys, k, **kw))
    rc = _emu_lib().kas_emu_rack_rank(sr.ctypes.data, si.ctypes.data, None if srk is None else srk.ctypes.data, int(sr.shape[0]),
                                      None if fs is None else C.byref(fs), None if cs is None else C.byref(cs), 0, None, None,
                                      out.ctypes.data, out.ctypes.data, None, None, out.ctypes.data, out.ctypes.data, 0, err, 256)
    return rc, err.value.decode()


# ---- synthetic records ----------------------------------------------------------------------------------------------------
def synthetic_racks(S, seed, values=4):
    """S scenario rack records drawn as test_choose_cpu.synthetic draws the others: every field from `values` (an int: 0..values-1;
    a list: those values), the two minima such that the spreads are values of the pool too"""
    rng = np.random.default_rng([seed, S, 16])
    pool = np.arange(values) if isinstance(values, int) else np.asarray(values, dtype=np.int64)
    draw = lambda: pool[rng.integers(0, pool.size, S)]
    srk = np.zeros(S, abi.SCENARIO_RACK_IMPACT_DTYPE)
    for f in abi.SCENARIO_RACK_FIELDS:
        srk[f] = draw()
    srk["min_rack_replicas_after"] = srk["max_rack_replicas_after"] - np.minimum(draw(), srk["max_rack_replicas_after"])
    srk["min_rack_leaders_after"] = srk["max_rack_leaders_after"] - np.minimum(draw(), srk["max_rack_leaders_after"])
    return srk


def records(S, seed, values=4, failed="random"):
    sr, si = synthetic(S, seed, values=values, failed=failed)
    return sr, si, synthetic_racks(S, seed, values=values)


def _sizes(S, k):
    rng = np.random.default_rng(S + k)
    return rng.integers(0, 7, S) * 3 + (np.arange(S) % 5 == 0), rng.integers(0, 50, S)     # (odd sizes and zeros among them)


def _check_rank(sr, si, srk, keys, k, what, sized=True, lds_fill=0xCDCDCDCD, path=0):
    S = int(sr.shape[0])
    cells, n_nodes = _sizes(S, k) if sized else (None, None)
    want = R.rank_ref(sr, si, srk, keys, k)
    got = emu_rack_rank(sr, si, srk, keys, k, None, cells, n_nodes, lds_fill=lds_fill, path=path)
    assert got.n_ok == want.n_ok, (what, got.n_ok, want.n_ok)
    assert np.array_equal(got.rank, want.rank), (what, "rank", np.nonzero(got.rank != want.rank)[0][:5])
    assert np.array_equal(got.chosen, want.chosen), (what, "chosen", got.chosen[:8], want.chosen[:8])
    if sized:
        assert np.array_equal(got.row_off, offsets_ref(want.order, cells, k)), (what, "row_off")
        assert np.array_equal(got.node_off, offsets_ref(want.order, n_nodes, k)), (what, "node_off")
    return want


def _check_front(sr, si, srk, keys, k, what, within=(), sized=True, lds_fill=0xCDCDCDCD, base=None, path=0):
    """base: the checker's front of the same records and spec at another k (the O(S^2) pass is then not repeated)"""
    S = int(sr.shape[0])
    cells, n_nodes = _sizes(S, k) if sized else (None, None)
    want = R.front_of(sr, si, srk, keys, k, within) if base is None else cut(base, k)
    if sized:
        want.row_off, want.node_off = offsets_ref(want.order, cells, k), offsets_ref(want.order, n_nodes, k)
    got = emu_rack_rank(sr, si, srk, keys, k, within, cells, n_nodes, lds_fill=lds_fill, path=path)
    assert got.n_ok == want.n_ok, (what, got.n_ok, want.n_ok)
    assert_same_front(want, got, what)
    return want


def _ks(S, n):
    return sorted({k for k in (0, 1, n - 1, n, n + 1, S) if 0 <= k <= S})


def _front_every_k(sr, si, srk, keys, what, within=()):
    want = R.front_of(sr, si, srk, keys, 0, within)
    for k in _ks(int(sr.shape[0]), int(want.order.size)):
        _check_front(sr, si, srk, keys, k, f"{what} k={k}", within, base=want)
    return want


@pytest.mark.parametrize("S", S_VALUES)
def test_emulated_every_rack_key_alone(S):
    """every rack criterion alone, ranked and fronted, criteria from {0..3}: the index decides most comparisons; the front of one
    criterion is the first of the smallest"""
    sr, si, srk = records(S, 1)
    n_ok = int((sr["status"] == 0).sum())
    for name in RACK_NAMES:
        want = _check_rank(sr, si, srk, (name,), min(S, max(n_ok - 1, 0)), f"S={S} {name}")
        if S >= 64 and n_ok >= 16:                              # (the records do tie: the guard of this test)
            first = R.criterion(sr, si, srk, name)[want.order]
            assert np.unique(first).size <= 4 < first.size
        front = _check_front(sr, si, srk, (name,), min(S, 2), f"S={S} front {name}")
        assert front.order.size == (1 if n_ok else 0)
    # the checker reads the record as the header lays it out: word i is key KAS_KEY_RACK_BASE + i
    words = srk.view(np.int32).reshape(S, 16)
    for i, name in enumerate(RACK_NAMES[:15]):
        assert np.array_equal(R.criterion(sr, si, srk, abi.KAS_KEY_RACK_BASE + i), words[:, i]) and abi.RACK_KEYS[name] == 16 + i
    assert np.array_equal(R.criterion(sr, si, srk, 31), words[:, 12].astype(np.int64) - words[:, 11])
    assert np.array_equal(R.criterion(sr, si, srk, 32), words[:, 14].astype(np.int64) - words[:, 13])


@pytest.mark.parametrize("S", S_VALUES)
def test_emulated_specs_mixing_broker_and_rack_keys(S):
    """specs of 2 to 4 criteria from both sets: rankings for every k, and fronts of values from {0..63} for every k"""
    sr, si, srk = records(S, 2)
    n_ok = int((sr["status"] == 0).sum())
    for keys in MIXED:
        for k in _ks(S, n_ok):
            _check_rank(sr, si, srk, keys, k, f"S={S} {keys} k={k}")
    _check_rank(sr, si, srk, MIXED[0], min(S, 3), f"S={S} rank only", sized=False)
    sr, si, srk = records(S, 2, values=64)
    for keys in MIXED:
        want = _front_every_k(sr, si, srk, keys, f"S={S} wide {keys}")
        if S >= 257 and len(keys) == 4:
            assert want.order.size >= 10, want.order.size
    _check_front(sr, si, srk, MIXED[1], min(S, 3), f"S={S} front, rank only", sized=False)


@pytest.mark.parametrize("S", [2, 257, 1025])
def test_emulated_extreme_values(S):
    """criterion values at 0 and at 2^31 - 1, among failed scenarios"""
    sr, si, srk = records(S, 4, values=[0, TOP], failed="alternate")
    for keys in [(name,) for name in RACK_NAMES] + MIXED:
        assert set(np.unique(R.criterion(sr, si, srk, keys[0]))) <= {0, TOP}
        _check_rank(sr, si, srk, keys, S, f"S={S} extremes {keys}")
    for keys in MIXED + [("rack_replica_spread", "rack_leader_spread")]:
        _check_front(sr, si, srk, keys, S, f"S={S} extremes front {keys}")
    sr, si, srk = records(S, 5, values=[TOP])                               # every field at the top: the spreads are 0 or 2^31 - 1
    _check_rank(sr, si, srk, MIXED[2], S, f"S={S} every criterion 2^31 - 1")
    _check_front(sr, si, srk, MIXED[2], S, f"S={S} every criterion 2^31 - 1", within={"max_rack_inbound": TOP})


@pytest.mark.parametrize("S", S_VALUES)
@pytest.mark.parametrize("failed", ["none", "alternate", "all"])
def test_emulated_failed_scenarios_and_every_k(S, failed):
    sr, si, srk = records(S, 2, failed=failed)
    n_ok = int((sr["status"] == 0).sum())
    assert n_ok == {"none": S, "alternate": (S + 1) // 2, "all": 0}[failed]
    for k in _ks(S, n_ok):
        want = _check_rank(sr, si, srk, ("colocated_after", "max_outbound"), k, f"S={S} failed={failed} k={k}")
        if failed == "all":
            assert want.n_ok == 0 and (want.chosen == -1).all() and (want.rank == -1).all()
    # an antichain over a rack criterion and a broker criterion: every OK scenario is a member, and k cuts the front
    perm = np.random.default_rng(S).permutation(S).astype(np.int32)
    srk["new_rack_replicas"], sr["moved_replicas"] = perm, S - perm
    want = _front_every_k(sr, si, srk, ("new_rack_replicas", "moved_replicas"), f"S={S} antichain {failed}")
    assert want.order.size == n_ok and (want.classes[sr["status"] == 0] == 0).all()
    if failed == "all":
        assert (want.chosen == -1).all() and (want.rank == NOT_OK).all() and want.counts.tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("fill", [0, 0xFFFFFFFF])
def test_emulated_whatever_the_lds_holds(fill):
    """LDS is uninitialised on hardware: zeros (the smallest key, flags clear) and all ones (flags set everywhere)"""
    for S in (65, 1025):
        sr, si, srk = records(S, 6, values=64)
        _check_rank(sr, si, srk, MIXED[1], S // 2, f"S={S} lds {fill:#x}", lds_fill=fill)
        _check_front(sr, si, srk, MIXED[2], S // 2, f"S={S} lds {fill:#x}", within={"max_rack_outbound": 40}, lds_fill=fill)


@pytest.mark.parametrize("S", [1, 65, 257, 1025, 2049])
def test_emulated_bounds_on_rack_keys(S):
    """bounds on rack criteria inside and outside the spec, beside a broker bound, limit 2^31 - 1, and a bound nobody meets"""
    sr, si, srk = records(S, 7, values=64)
    keys = ("max_rack_inbound", "moved_replicas")
    free = R.front_of(sr, si, srk, keys, 0)
    cases = [{}, {"max_rack_inbound": 30}, {"max_rack_outbound": 20}, {"rack_replica_spread": 20, "moved_replicas": 40},
             {"max_rack_outbound": 30, "leaders_moved": 30, "colocated_after": 30, "max_rack_inbound": 50},
             {"rack_leader_spread": TOP}, {"max_rack_outbound": TOP, "max_inbound": TOP}]
    for within in cases:
        want = _front_every_k(sr, si, srk, keys, f"S={S} within {within}", within)
        if S >= 257 and within == {"max_rack_inbound": 30}:                 # inside the spec: the bound only filters the front
            assert set(want.order) <= set(free.order) and (want.classes == OVER_LIMIT).any()
        if S >= 257 and within == {"max_rack_outbound": 20}:                # outside: it creates members
            assert not set(want.order) <= set(free.order)
        if TOP in within.values():
            assert np.array_equal(want.rank, free.rank)
    srk["single_rack_rows_after"] += 1                                      # a bound nobody meets: the front is empty
    want = _check_front(sr, si, srk, keys, min(S, 3), f"S={S} nobody", within={"single_rack_rows_after": 0})
    assert want.counts[1] == 0 and want.counts[2] == 0 and (want.chosen == -1).all() and (want.row_off == 0).all()
    assert set(np.unique(want.rank)) <= {NOT_OK, OVER_LIMIT}


@pytest.mark.parametrize("S", [1, 65, 256, 1025])
def test_broker_keys_give_the_parent_code_paths_bytes(S):
    """a spec without a rack criterion, with rack records or with NULL: the bytes of the parent code path (the drivers that were there),
    from the instance the library launches (the parent's) and from the instance that reads rack records"""
    sr, si, srk = records(S, 8)
    k = S // 2
    cells, n_nodes = _sizes(S, k)
    for keys in (tc.MULTI_SPECS[0], tc.MULTI_SPECS[2]):
        theirs = tc.emu_rank(sr, si, keys, k, cells, n_nodes)
        for records_given, path in ((None, 0), (srk, 0), (srk, 1)):
            mine = emu_rack_rank(sr, si, records_given, keys, k, None, cells, n_nodes, path=path)
            for f in ("rank", "chosen", "row_off", "node_off"):
                assert getattr(mine, f).tobytes() == getattr(theirs, f).tobytes(), (keys, f, path)
            assert mine.n_ok == theirs.n_ok
        within = {"max_outbound": 2}
        theirs = tf.emu_front_rank(sr, si, keys, k, within, cells, n_nodes)
        for records_given, path in ((None, 0), (srk, 0), (srk, 1)):
            mine = emu_rack_rank(sr, si, records_given, keys, k, within, cells, n_nodes, path=path)
            for f in ("rank", "chosen", "row_off", "node_off", "counts"):
                assert getattr(mine, f).tobytes() == getattr(theirs, f).tobytes(), (keys, f, path)


def test_refusals_in_their_order_each_with_its_text():
    """the spec refusals of the parents with the widened key set and the same texts, then the missing rack records"""
    sr, si, srk = records(8, 7)
    good = ("colocated_after",)
    cases = [(dict(keys=good, k=1, n_keys=0), "kas_choose_spec: n_keys outside 1..4"), (dict(keys=good, k=1, n_keys=5), "n_keys outside 1..4"),
             (dict(keys=(10,), k=-1), "kas_choose_spec: unknown criterion"), (dict(keys=(15,), k=1), "unknown criterion"),
             (dict(keys=(33,), k=1), "unknown criterion"), (dict(keys=(17, -1), k=1), "unknown criterion"),
             (dict(keys=good, k=-1), "kas_choose_spec: k outside"), (dict(keys=good, k=9), "k outside"),
             (dict(keys=(33,), k=-1, within=[(33, -1)], n_keys=0, n_limits=5), "kas_front_spec: n_keys outside 1..4"),
             (dict(keys=(33,), k=-1, within=[(33, -1)], n_limits=5), "kas_front_spec: unknown criterion"),
             (dict(keys=good, k=-1, within=[(33, -1)], n_limits=5), "n_limits outside 0..4"),
             (dict(keys=good, k=-1, within=[(17, -1), (12, -1)]), "unknown limit criterion"),
             (dict(keys=good, k=-1, within=[(17, 3), (32, -1)]), "negative limit"),
             (dict(keys=good, k=-1, within=[(32, 3)]), "kas_front_spec: k outside")]
    for kw, text in cases:
        for given in (srk, None):                                           # (the spec's refusals come before the missing records)
            rc, err = emu_refusal(sr, si, given, **kw)
            assert rc == E_INVALID and text in err, (kw, rc, err)
    for kw in (dict(keys=good, k=1), dict(keys=("moved_replicas", "rack_leader_spread"), k=8), dict(keys=good, k=1, within=[]),
               dict(keys=("moved_replicas",), k=1, within=[("n_racks", 3)])):
        rc, err = emu_refusal(sr, si, None, **kw)
        assert rc == E_INVALID and err == NO_RECORDS, (kw, rc, err)
        assert emu_refusal(sr, si, srk, **kw)[0] == 0
    assert emu_refusal(sr, si, None, keys=("moved_replicas",), k=1, within=[("max_inbound", 3)])[0] == 0
    # the entries that were there know no rack criterion
    out = np.zeros(16, np.int32)
    err = C.create_string_buffer(256)
    spec = _cspec(good, 1)
    rc = tc._emu_lib().kas_emu_rank(sr.ctypes.data, si.ctypes.data, 8, C.byref(spec), None, None, out.ctypes.data, out.ctypes.data, None, None,
                                    out.ctypes.data, 0, err, 256)
    assert rc == E_INVALID and "unknown criterion" in err.value.decode()


# ---- rank / mark / front rank and gather over solved batches ----------------------------------------------------------------
GUARD_CELLS, GUARD_NODES = 64, 3


def emu_rack_choose(fb, out, sr, imp, srk, keys, k, within=None, mode=0, lds_fill=0xCDCDCDCD):
    """kas_emu_rack_choose over the tables of a solve, its impact records and its scenario rack records: a choice (within is None)
    or a front; capacities exactly the k largest scenarios', guards behind them"""
    S = fb.n_scenarios
    nodes, si = imp
    bd = batch_desc(fb)
    t = abi.Tables()
    t.out = out.ctypes.data
    t.scenario_results = sr.ctypes.data
    itab = abi.ImpactTables(nodes.ctypes.data if nodes.size else None, si.ctypes.data)
    rows_cap, nodes_cap = k_largest(fb, k)
    dt = np.int32 if mode == 0 else np.uint16
    got = SimpleNamespace(rank=np.full(S + 1, SENTINEL, np.int32), chosen=np.full(k + 1, SENTINEL, np.int32),
                          row_off=np.full(k + 2, SENTINEL, np.int64), node_off=np.full(k + 2, SENTINEL, np.int64),
                          n_ok=np.full(2, SENTINEL, np.int32), counts=np.full(5, SENTINEL, np.int32),
                          rows=np.full(rows_cap + GUARD_CELLS, 0x7B7B, dt), nodes=np.zeros(nodes_cap + GUARD_NODES, abi.NODE_IMPACT_DTYPE))
    raw_nodes = got.nodes.view(np.uint8)
    raw_nodes[...] = 0x7B
    ch = abi.Choice(got.rank.ctypes.data, got.chosen.ctypes.data, got.row_off.ctypes.data, got.node_off.ctypes.data, got.n_ok.ctypes.data,
                    got.rows.ctypes.data, rows_cap, got.nodes.ctypes.data, nodes_cap)
    err = C.create_string_buffer(512)
    front = within is not None
    fs, cs = (_fspec(keys, k, within), None) if front else (None, _cspec(keys, k))
    rc = _emu_lib().kas_emu_rack_choose(C.byref(bd), C.byref(t), C.byref(itab), None if srk is None else srk.ctypes.data, mode,
                                        None if fs is None else C.byref(fs), None if cs is None else C.byref(cs), C.byref(ch),
                                        got.counts.ctypes.data if front else None, lds_fill, err, 512)
    assert rc == 0, (rc, err.value.decode())
    assert got.rank[S] == SENTINEL and got.chosen[k] == SENTINEL and got.n_ok[1] == SENTINEL and got.counts[4] == SENTINEL
    assert got.row_off[k + 1] == SENTINEL and got.node_off[k + 1] == SENTINEL
    got.rank, got.chosen, got.n_ok, got.counts = got.rank[:S], got.chosen[:k], int(got.n_ok[0]), got.counts[:4]
    got.row_off, got.node_off = got.row_off[:k + 1], got.node_off[:k + 1]
    used, recs = int(got.row_off[k]), int(got.node_off[k])
    assert 0 <= used <= rows_cap and 0 <= recs <= nodes_cap
    assert (got.rows[used:] == 0x7B7B).all(), "cells behind row_off[k] (the guard behind rows_cap among them) were written"
    assert (raw_nodes[32 * recs:] == 0x7B).all(), "records behind node_off[k] (the guard behind nodes_cap among them) were written"
    return got


_WHATIF_RACKS = None


def whatif_racks():
    """(WhatIf, variants, fb, the oracle's solve, the checker's impact records, the checker's scenario rack records against the
    report table of WhatIf.report_racks, the table, the rack names), computed once"""
    global _WHATIF_RACKS
    if _WHATIF_RACKS is None:
        w, vs, fb, ho, imp = whatif_solved()
        table, names = w.report_racks(vs)
        assert not np.array_equal(table, fb.node_rack)                      # (rack-unaware variants: the report table is not the solver's)
        _WHATIF_RACKS = (w, vs, fb, ho, imp, rack_ref(fb, ho, table)[1], table, names)
    return _WHATIF_RACKS


WHATIF_RANK = ("colocated_after", "replica_spread")
WHATIF_FRONT = ("new_rack_replicas", "replica_spread")
WHATIF_FOUR = ("max_rack_outbound", "rack_leader_spread", "rows_losing_racks", "replica_spread")
WHATIF_BOUND = {"max_outbound": 24}


def test_emulated_choice_of_the_whatif_batch_by_rack_criteria():
    _, _, fb, ho, imp, srk, _, _ = whatif_racks()
    S = fb.n_scenarios
    sr, si = ho.scenario_results[:S], imp[1][:S]
    ok = sr["status"] == 0
    n_ok = int(ok.sum())
    # the guards: co-located replicas exist among the variants that solve and change the ranking near the top
    coloc = srk["colocated_after"][ok]
    assert n_ok == 184 and int((coloc > 0).sum()) == 32 and np.unique(coloc).size == 28 and int(coloc.max()) == 373
    with_racks = R.rank_ref(sr, si, srk, WHATIF_RANK, 0).order
    without = R.rank_ref(sr, si, srk, WHATIF_RANK[1:], 0).order
    first = int(np.nonzero(with_racks != without)[0][0])
    assert first == 3 and int(without[3]) == 143 and int(srk["colocated_after"][143]) > 0 and 143 not in with_racks[:10].tolist()
    for keys, ks in ((WHATIF_RANK, (1, 5, n_ok, n_ok + 1, S)), (("single_rack_rows_after", "rack_replica_spread", "moved_replicas"), (5,)),
                     (("rack_leader_spread",), (5,))):
        for k in ks:
            want = R.choose_of(fb, sr, ho.out, imp, srk, keys, k)
            got = emu_rack_choose(fb, ho.out, sr, imp, srk, keys, k)
            assert_same_choice(want, got, f"what-if {keys} k {k}")
    # 16-bit cells and the narrowing gather, at one k
    fb16 = own_cur_form(fb)
    for mode, out, ref_out in tc._forms(fb16, ho)[1:]:
        want = R.choose_of(fb16, sr, ref_out, imp, srk, WHATIF_RANK, 5)
        assert_same_choice(want, emu_rack_choose(fb16, out, sr, imp, srk, WHATIF_RANK, 5, mode=mode), f"what-if mode {mode}")


def _same(want, got, what):
    assert_same_front(want, got, what)
    assert_same_choice(want, got, what)


def test_emulated_front_of_the_whatif_batch_by_rack_criteria():
    _, _, fb, ho, imp, srk, _, _ = whatif_racks()
    S = fb.n_scenarios
    sr, si = ho.scenario_results[:S], imp[1][:S]
    a = R.front_of(sr, si, srk, WHATIF_FRONT, 0)
    four = R.front_of(sr, si, srk, WHATIF_FOUR, 0)
    bounded = R.front_of(sr, si, srk, WHATIF_FOUR, 0, WHATIF_BOUND)
    clean = R.front_of(sr, si, srk, WHATIF_FOUR, 0, {"colocated_after": 0})
    broker = R.front_of(sr, si, srk, tf.WHATIF_A, 0)
    created = R.front_of(sr, si, srk, tf.WHATIF_A, 0, {"max_rack_inbound": 235})
    # the guards
    assert a.order.size >= 3 and sorted(a.order.tolist()) == [4, 143, 150]
    assert bounded.order.size >= 10 and bounded.counts.tolist() == [184, 128, 13, 0]
    assert four.order.size == 17 and clean.counts.tolist() == [184, 152, 13, 0]
    assert int((clean.classes != four.classes).sum()) == 32 and int((clean.classes == OVER_LIMIT).sum()) == 32     # the bound changes the classes
    assert sorted(broker.order.tolist()) == [0, 46, 47, 83, 175, 210]
    assert sorted(set(created.order.tolist()) - set(broker.order.tolist())) == [135, 184]      # a rack bound outside the spec creates members
    assert (broker.classes[[135, 184]] == DOMINATED).all()
    fb16 = own_cur_form(fb)
    forms = tc._forms(fb16, ho)
    cases = ((WHATIF_FRONT, {}, 3), (WHATIF_FOUR, WHATIF_BOUND, 13), (WHATIF_FOUR, {"colocated_after": 0}, 13),
             (tf.WHATIF_A, {"max_rack_inbound": 235}, 6))
    for keys, within, n_front in cases:
        for k in (1, n_front, n_front + 1, S) if keys == WHATIF_FRONT else (n_front,):
            for mode, out, ref_out in forms if (k == n_front and keys != tf.WHATIF_A) else forms[:1]:
                want = R.front_choice_of(fb16 if mode else fb, sr, ref_out, imp, srk, keys, k, within)
                got = emu_rack_choose(fb16 if mode else fb, out, sr, imp, srk, keys, k, within, mode=mode)
                _same(want, got, f"what-if {keys} {within} k {k} mode {mode}")
                assert want.counts[2] == n_front
        # the moves of the members, in member order (the moves pass takes the front's chosen[], -1 tail and all)
        want = R.front_of(sr, si, srk, keys, n_front + 1, within)
        assert want.chosen[-1] == -1
        tm.check(fb, fb.cur, ho, [int(s) for s in want.chosen], 7, 0, f"what-if moves {keys} {within}")


@pytest.mark.parametrize("name", ["mixed42", "degenerate"])
def test_emulated_choice_front_and_gather_for_every_k(name):
    """oracle-solved batches with a custom report table and with the batch's own racks: every k, both cell layouts and the
    narrowing gather"""
    fb, ho, imp = solved(name)
    S = fb.n_scenarios
    forms = tc._forms(fb, ho)
    for table in (None, tr.real_racks(fb, 3)):
        srk = rack_ref(fb, ho, table)[1]
        for k in range(0, S + 1):
            for mode, out, ref_out in forms if k in (1, S) else forms[:1]:
                keys = ("max_rack_inbound", "moved_replicas") if k % 2 else ("rack_replica_spread", "leaders_moved", "new_rack_replicas")
                want = R.choose_of(fb, ho.scenario_results, ref_out, imp, srk, keys, k)
                got = emu_rack_choose(fb, out, ho.scenario_results[:S], imp, srk, keys, k, mode=mode)
                assert_same_choice(want, got, f"{name} mode {mode} k {k} {keys}")
                want = R.front_choice_of(fb, ho.scenario_results, ref_out, imp, srk, keys, k, {"max_rack_outbound": 10**6})
                got = emu_rack_choose(fb, out, ho.scenario_results[:S], imp, srk, keys, k, {"max_rack_outbound": 10**6}, mode=mode)
                _same(want, got, f"{name} front mode {mode} k {k} {keys}")


# ---- the planner ----------------------------------------------------------------------------------------------------------
HOST_BUFS = tr.HOST_BUFS
MISSING = dict(tf.MISSING, rk_racks=65536, rk_scenarios=131072, rk_off=262144)
HEAD = ("rows_need", "nodes_need", "chunks", "head_bytes", "gather_rows", "K", "native16", "listed", "rack_records", "r_max")
_BUF = np.zeros(16, np.int64)


def rack_choose_host_call(fb, front=None, spec=None, mv=None, rows_cap=None, nodes_cap=None, racks_cap=None, racks=True, rack_keys=True,
                          report_rack=None, missing=(), cells16=False):
    """kas_plan_host_call for a kas_solve_host_front_racks call (front) or a kas_solve_host_choose_racks call (spec); rack_keys=False
    plans the parent call of the same arguments: (rc, plan or None, text)"""
    L = _emu_lib()
    assert L.kas_emu_rack_choose_buffers() == len(HOST_BUFS)
    bd = batch_desc(fb)
    if cells16:
        bd.node_id = None
    need = k_largest(fb, (front or spec).k)
    rep = None if report_rack is None else np.ascontiguousarray(report_rack, dtype=np.int32)
    try:
        rk_need = int(rack_counts(fb, rep).sum())
    except ValueError:
        rk_need = 0
    lens = (C.c_int64 * 6)(int(fb.cur.shape[0]), int(fb.aux.shape[0]), int(fb.ctx.shape[0]), need[0] if rows_cap is None else rows_cap,
                           need[1] if nodes_cap is None else nodes_cap, rk_need if racks_cap is None else racks_cap)
    head, nbytes = (C.c_int64 * len(HEAD))(), (C.c_int64 * len(HOST_BUFS))()
    err = C.create_string_buffer(512)
    rc = L.kas_emu_rack_choose_host_call(C.byref(bd), lens, sum(MISSING[m] for m in missing), int(cells16),
                                         None if front is None else C.byref(front), None if spec is None else C.byref(spec),
                                         None if mv is None else C.byref(mv), int(racks), int(rack_keys),
                                         None if rep is None else rep.ctypes.data, head, nbytes, err, 512)
    if rc != 0:
        return rc, None, err.value.decode()
    plan = dict(zip(HEAD, [int(v) for v in head]))
    plan["bytes"] = dict(zip(HOST_BUFS, [int(v) for v in nbytes]))
    return rc, plan, ""


def _mv(mask=7, moves_cap=10**6, cells_cap=10**7):
    b = _BUF.ctypes.data
    return abi.Moves(mask, 0, b, b, b, moves_cap, b, cells_cap)


def test_planner_refuses_in_order_each_with_its_text():
    """the spec (widened key set, the parents' texts), the missing rack records, everything the parent refuses in its order, then the
    rack refusals of kas_solve_host_rack_impact in their order: every case has every later refusal pending too"""
    fb, _, _ = solved("mixed42")
    S = fb.n_scenarios
    good = ("colocated_after", "leaders_moved")
    rows, nodes = k_largest(fb, 2)
    need = int(rack_counts(fb).sum())
    bad_mv = abi.Moves(9, 0, None, None, None, -1, None, -1)
    neg = fb.node_rack.copy(); neg[3] = -1
    big = fb.node_rack.copy(); big[5] = abi.KAS_RACK_LIMIT
    both = big.copy(); both[int(fb.scen["node_off"][1]) + 2] = -1
    late = dict(report_rack=both, racks_cap=0, missing=("rank", "counts", "rk_off"), mv=bad_mv)
    every = dict(rows_cap=0, nodes_cap=0, **late)
    order = [(dict(front=_fspec((33,), -1, [(33, -1)], n_keys=0, n_limits=5), **every), E_INVALID, "kas_front_spec: n_keys outside 1..4"),
             (dict(front=_fspec((33,), -1, [(33, -1)], n_limits=5), **every), E_INVALID, "kas_front_spec: unknown criterion"),
             (dict(front=_fspec(good, -1, [(33, -1)], n_limits=5), **every), E_INVALID, "n_limits outside 0..4"),
             (dict(front=_fspec(good, -1, [(12, -1)]), **every), E_INVALID, "unknown limit criterion"),
             (dict(front=_fspec(good, -1, [(17, -1)]), **every), E_INVALID, "negative limit"),
             (dict(front=_fspec(good, -1, [(17, 1)]), **every), E_INVALID, "kas_front_spec: k outside"),
             (dict(front=_fspec(good, S + 1, [(17, 1)]), **every), E_INVALID, "k outside"),
             (dict(spec=_cspec(good, 2, n_keys=5), **every), E_INVALID, "kas_choose_spec: n_keys outside 1..4"),
             (dict(spec=_cspec((10,), -1), **every), E_INVALID, "kas_choose_spec: unknown criterion"),
             (dict(spec=_cspec(good, -1), **every), E_INVALID, "kas_choose_spec: k outside"),
             (dict(front=_fspec(good, 2), racks=False, **every), E_INVALID, NO_RECORDS),
             (dict(front=_fspec(("moved_replicas",), 2, [(32, 5)]), racks=False, **every), E_INVALID, NO_RECORDS),
             (dict(spec=_cspec(good, 2), racks=False, **every), E_INVALID, NO_RECORDS),
             (dict(front=_fspec(good, 2), rows_cap=rows - 1, nodes_cap=0, **late), E_INVALID, "rows_cap below"),
             (dict(spec=_cspec(good, 2), rows_cap=rows - 1, nodes_cap=0, **late), E_INVALID, "rows_cap below"),
             (dict(front=_fspec(good, 2), nodes_cap=nodes - 1, **late), E_INVALID, "nodes_cap below"),
             (dict(front=_fspec(good, 2), **late), E_INVALID, "an array the call writes is NULL"),
             (dict(spec=_cspec(good, 2), report_rack=both, racks_cap=0, missing=("rk_off",), mv=bad_mv), E_INVALID, "mask outside 1..7"),
             (dict(spec=_cspec(good, 2), report_rack=both, racks_cap=0, missing=("rk_off",)), E_INVALID, "negative"),
             (dict(front=_fspec(good, 2), report_rack=both, racks_cap=0, missing=("rk_off",), mv=_mv()), E_INVALID, "negative"),
             (dict(spec=_cspec(good, 2), report_rack=neg, racks_cap=0, missing=("rk_off",)), E_INVALID, "negative"),
             (dict(spec=_cspec(good, 2), report_rack=big, racks_cap=0, missing=("rk_off",)), E_UNSUPPORTED, "KAS_RACK_LIMIT"),
             (dict(spec=_cspec(good, 2), racks_cap=need - 1, missing=("rk_off",)), E_INVALID, "racks_cap below"),
             (dict(front=_fspec(good, 2), missing=("rk_off",)), E_INVALID, "racks / scenarios / rack_off == NULL"),
             (dict(spec=_cspec(good, 2), missing=("rk_scenarios",)), E_INVALID, "racks / scenarios / rack_off == NULL"),
             (dict(spec=_cspec(good, 2), missing=("rk_racks",)), E_INVALID, "racks / scenarios / rack_off == NULL")]
    for kw, code, text in order:
        rc, _, err = rack_choose_host_call(fb, **kw)
        assert rc == code and text in err, (text, rc, err)
    # the parent calls refuse every rack criterion as unknown, with rack records or without
    for racks in (True, False):
        rc, _, err = rack_choose_host_call(fb, spec=_cspec(good, 2), rack_keys=False, racks=racks)
        assert rc == E_INVALID and "unknown criterion" in err
        rc, _, err = rack_choose_host_call(fb, front=_fspec(("moved_replicas",), 2, [(17, 0)]), rack_keys=False, racks=racks)
        assert rc == E_INVALID and "unknown limit criterion" in err
    # a table for a batch without nodes
    from kafka_assigner_amd.flatten import flatten
    rc, _, err = rack_choose_host_call(flatten([]), spec=_cspec(good, 0), report_rack=np.zeros(1, np.int32), racks_cap=0)
    assert rc == E_INVALID and "without nodes" in err


@pytest.mark.parametrize("cells16", [False, True], ids=["int32", "cells16"])
def test_planner_decisions_of_the_combined_call_and_bytes_of_the_calls_that_were_there(cells16):
    fb, _, _ = solved("mixed42")
    S, k = fb.n_scenarios, 3
    need = int(rack_counts(fb).sum())
    n_front, n_moves = len(tf.HOST_BUFS), len(tm.HOST_BUFS)
    broker = ("moved_replicas", "leaders_moved")
    keys = ("colocated_after", "leaders_moved")
    shapes = (("choose", {}), ("choose_moves", dict(mv=_mv())), ("choose_moves_norows", dict(mv=_mv(), rows_cap=0, missing=("rows",))))
    for what, kw in shapes:
        want = tf.PARENT[(what, cells16)]
        # the parent calls through this driver: byte for byte what the parent of the Pareto front planned, nothing behind
        rc, plan, err = rack_choose_host_call(fb, spec=_cspec(broker, k), racks=False, rack_keys=False, cells16=cells16, **kw)
        assert rc == 0, err
        got = [plan["bytes"][n] for n in HOST_BUFS]
        assert got[:len(want)] == want and not any(got[len(want):]), (what, got)
        # ... and through the driver that was there: the same
        rc, theirs, err = tf.front_host_call(fb, spec=_cspec(broker, k), cells16=cells16, **kw)
        assert rc == 0 and [theirs["bytes"][n] for n in tf.HOST_BUFS] == got[:n_front], err
        # the combined call, without a rack pass (host_racks == NULL): the parent's bytes whatever the switch says
        rc, plan, err = rack_choose_host_call(fb, spec=_cspec(broker, k), racks=False, cells16=cells16, **kw)
        assert rc == 0 and [plan["bytes"][n] for n in HOST_BUFS] == got, err
        # the combined call: the parent's bytes of every buffer that was there, and the two rack buffers of kas_solve_host_rack_impact
        for spec_kw in (dict(spec=_cspec(keys, k)), dict(front=_fspec(keys, k, {"max_rack_inbound": 100}))):
            rc, plan, err = rack_choose_host_call(fb, cells16=cells16, **spec_kw, **kw)
            assert rc == 0, err
            mine = [plan["bytes"][n] for n in HOST_BUFS]
            assert mine[:len(want)] == want and not any(mine[len(want):n_moves]), (what, mine)
            assert mine[n_moves:n_front] == ([4 * (S + 1), 16, 16] if "front" in spec_kw else [0, 0, 0])
            assert plan["bytes"]["rk_racks"] == 32 * (need + 1) and plan["bytes"]["rk_scen"] == 64 * (S + 1)
            assert plan["rack_records"] == need and plan["head_bytes"] == 16 * (k + 1) + 4 * S + 4 * k + 4
            assert plan["listed"] == (k if "mv" in kw else 0) and plan["gather_rows"] == (0 if "rows_cap" in kw else 1)
    # the rack call and the impact call through the driver that was there: unchanged (tests/test_racks_cpu.py pins the bytes)
    rc, rk, err = tr.rack_host_call(fb, racks_cap=need, cells16=cells16)
    assert rc == 0 and rk["bytes"]["rk_racks"] == 32 * (need + 1) and [rk["bytes"][n] for n in HOST_BUFS[:12]] == tr.PARENT[(cells16, 0)], err
    # a choice by rack criteria without moves and without rows: the size table without cells is the only moves buffer
    rc, plan, err = rack_choose_host_call(fb, spec=_cspec(keys, k), cells16=cells16, rows_cap=0, missing=("rows",))
    assert rc == 0 and plan["gather_rows"] == 0 and plan["bytes"]["mv_sizes0"] == 32 * (S + 1), err
    assert not any(plan["bytes"][n] for n in tm.HOST_BUFS[20:] if n != "mv_sizes0")
    # a custom report table sizes the rack buffers
    one = tr.one_rack(fb)
    rc, plan, err = rack_choose_host_call(fb, spec=_cspec(keys, k), cells16=cells16, report_rack=one)
    assert rc == 0 and plan["rack_records"] == int(rack_counts(fb, one).sum()) and plan["r_max"] == 1, err


# ---- ABI ------------------------------------------------------------------------------------------------------------------
def test_abi_declares_the_rack_criteria_and_entries(tmp_path):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(kas_[a-z_0-9]+)\s*\(", src))
    assert len(abi.RACK_CHOOSE_ENTRIES) == 10
    for name in abi.RACK_CHOOSE_ENTRIES:
        assert name in declared and name in native.SYMBOLS, name
    assert re.search(r"#define KAS_ABI_VERSION (\d+)", src).group(1) == str(abi.KAS_ABI_VERSION) == "6"
    probe = tmp_path / "probe.c"
    fields = abi.SCENARIO_RACK_FIELDS
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kas_abi.h"\nint main(void) {\n'
                     + "".join('  printf("%%d %%zu\\n", KAS_KEY_%s, offsetof(kas_scenario_rack_impact, %s));\n' % (f.upper(), f) for f in fields)
                     + '  printf("%d %d %d %d %d\\n", KAS_KEY_RACK_BASE, KAS_KEY_RACK_REPLICA_SPREAD, KAS_KEY_RACK_LEADER_SPREAD, KAS_KEY_RACK_END, KAS_KEY_COUNT);\n'
                     + '  printf("%zu %zu\\n", sizeof(kas_choose_spec), sizeof(kas_front_spec));\n  return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c11", "-I" + os.path.join(ROOT, "include"), str(probe), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)], text=True).splitlines()
    for i, f in enumerate(fields):
        key, off = (int(v) for v in lines[i].split())
        assert key == abi.RACK_KEYS[f] == 16 + i and off == 4 * (key - 16) == abi.SCENARIO_RACK_IMPACT_DTYPE.fields[f][1], f
    assert [int(v) for v in lines[15].split()] == [abi.KAS_KEY_RACK_BASE, abi.KAS_KEY_RACK_REPLICA_SPREAD, abi.KAS_KEY_RACK_LEADER_SPREAD,
                                                   abi.KAS_KEY_RACK_END, abi.KAS_KEY_COUNT] == [16, 31, 32, 33, 10]
    assert lines[16].split() == ["24", "60"]                                # (the specs are reused unchanged)
    assert abi.RACK_KEY_NAMES == abi.SCENARIO_RACK_FIELDS + ("rack_replica_spread", "rack_leader_spread")
    assert sorted(abi.RACK_KEYS.values()) == list(range(16, 33)) and abi.KEYS == {n: i for i, n in enumerate(abi.KEY_NAMES)} and len(abi.KEYS) == 10
    spec = abi.rack_choose_spec(("colocated_after", "replica_spread"), 3)
    assert (spec.n_keys, list(spec.key)[:2], spec.k) == (2, [17, 6], 3)
    fs = abi.rack_front_spec(("moved_replicas", "rack_leader_spread"), {"single_rack_rows_after": 0}, 4)
    assert (fs.n_keys, list(fs.key)[:2], fs.n_limits, fs.limit_key[0], fs.limit[0], fs.k) == (2, [0, 32], 1, 21, 0, 4)
    for bad in (lambda: abi.rack_choose_spec(("nope",), 1), lambda: abi.rack_front_spec(("moved_replicas",), {"nope": 1}),
                lambda: abi.choose_spec(("colocated_after",), 1), lambda: abi.front_spec(("moved_replicas",), {"n_racks": 1})):
        with pytest.raises(ValueError):
            bad()


def test_library_exports_the_rack_choose_entries():
    from kafka_assigner_amd import build
    build.build()
    L = native.load()
    for name in abi.RACK_CHOOSE_ENTRIES:
        assert hasattr(L, name), name
    assert L.kas_abi_version() == 6
    blob = open(build.LIB, "rb").read()
    for kernel in (b"kas_rank_racks_kernel", b"kas_front_mark_racks_kernel", b"kas_front_rank_racks_kernel",
                   b"kas_rank_kernel", b"kas_front_mark_kernel", b"kas_front_rank_kernel", b"kas_gather_kernel"):
        assert kernel in blob, kernel


# ---- WhatIf ---------------------------------------------------------------------------------------------------------------
def _fake_host_calls(monkeypatch):
    """native.solve_host_choose_racks / solve_host_front_racks over the emulator: the oracle's solve, the checker's impact and rack
    records, and the kernels' code for the ranking, the front and the gather"""
    from impact_ref import impact_ref
    from oracle_lib import oracle_solve
    calls = []

    def run(fb, keys, k, within, report_rack):
        ho = oracle_solve(fb)
        imp = impact_ref(fb, ho)
        racks, srk, rack_off = rack_ref(fb, ho, report_rack)
        S = fb.n_scenarios
        got = emu_rack_choose(fb, ho.out, ho.scenario_results[:S], imp, srk, keys, k, within)
        rr = native.RackReport(racks=racks, scenarios=srk, rack_off=rack_off, impact=imp[1])
        used, recs = int(got.row_off[k]), int(got.node_off[k])
        return ho, got, rr, dict(rank=got.rank, chosen=got.chosen, row_off=got.row_off, node_off=got.node_off, n_ok=got.n_ok,
                                 rows=got.rows[:used], nodes=got.nodes[:recs], scenarios=imp[1])

    def choose(fb, keys, k, report_rack=None, mask=None, rows=True, **kw):
        calls.append(("choose", tuple(abi.rack_key_id(x) for x in keys)))
        ho, got, rr, fields = run(fb, list(keys), k, None, report_rack)
        return ho, native.Choice(**fields), None, rr

    def front(fb, spec, report_rack=None, mask=None, rows=True, **kw):
        calls.append(("front", tuple(spec.key)[:spec.n_keys]))
        within = [(spec.limit_key[i], spec.limit[i]) for i in range(spec.n_limits)]
        ho, got, rr, fields = run(fb, list(spec.key)[:spec.n_keys], spec.k, within, report_rack)
        return ho, native.Front(n_eligible=int(got.counts[1]), n_front=int(got.counts[2]), **fields), None, rr

    def never(*a, **kw):
        raise AssertionError("a call with rack criteria took the entry without them")
    monkeypatch.setattr(native, "solve_host_choose_racks", choose)
    monkeypatch.setattr(native, "solve_host_front_racks", front)
    monkeypatch.setattr(native, "solve_host_choose", never)
    monkeypatch.setattr(native, "solve_host_front", never)
    return calls


def test_whatif_best_and_front_with_rack_criteria_without_a_gpu(monkeypatch):
    w, vs, fb, ho, imp, srk, table, names = whatif_racks()
    calls = _fake_host_calls(monkeypatch)
    S = fb.n_scenarios
    sr, si = ho.scenario_results[:S], imp[1][:S]
    best = w.best(vs, k=5, by=WHATIF_RANK)
    want = R.rank_ref(sr, si, srk, WHATIF_RANK, 5)
    assert [r._index for r in best] == want.chosen.tolist() and [r.rank for r in best] == list(range(5)) and 143 not in want.chosen
    for r in best:
        s = r._index
        assert r.colocated_after == int(srk["colocated_after"][s]) == 0 and r.n_racks == 6 and r.max_rack_inbound == int(srk["max_rack_inbound"][s])
        ri = r.rack_impact()
        assert list(ri) == names[s] and sum(v["inbound"] for v in ri.values()) == r.moved_replicas
        assert r.assignment(w.topic_names[0]) and r.broker_impact()
    # racks=True with broker criteria: the same order as without, and the rack figures beside it
    plain = w.best(vs, k=3, by=("replica_spread",), racks=True)
    assert [r._index for r in plain] == R.rank_ref(sr, si, srk, ("replica_spread",), 3).chosen.tolist() and plain[0].rack_impact()
    full = w.front(vs, by=WHATIF_FRONT, k=S)
    assert full.n_front == len(full) == 3 and sorted(r._index for r in full) == [4, 143, 150]
    assert full.classes.count("member") == 3 and "dominated" in full.classes and "failed" in full.classes
    bound = w.front(vs, by=tf.WHATIF_A, within={"max_rack_inbound": 235}, k=S)
    assert bound.n_eligible == 92 and {135, 184} <= {r._index for r in bound} and "over_limit" in bound.classes
    assert all(r.max_rack_inbound <= 235 and r.rack_impact() for r in bound)
    assert calls == [("choose", (17, 6)), ("choose", (6,)), ("front", (22, 6)), ("front", (0, 7, 6))]
    for call in (lambda: w.best(vs, by=("nope",)), lambda: w.front(vs, by=("nope",)), lambda: w.front(vs, within={"nope": 1}),
                 lambda: w.best(vs, by=("colocated_after",), rows=False)):
        with pytest.raises(ValueError) as e:
            call()
        assert "rows=False" in str(e.value) or ("rack_leader_spread" in str(e.value) and "moved_replicas" in str(e.value))

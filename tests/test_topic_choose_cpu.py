"""Ranking and fronting by topic criteria (include/kas_abi.h: KAS_KEY_TOPIC_BASE, the *_topics entries) without a GPU.

- The instances of the rank, mark and front rank kernels' bodies that read the scenario topic records (kas_choose_body.h /
  kas_front_body.h with kasc::TopicRecords), compiled with g++ against tests/emu/kas_wave.h and stepped on CPU fibers
  (tests/emu/topic_choose_driver.cpp) over synthetic records, against the NumPy checker (tests/topic_choose_ref.py): the S values
  around the wavefront, the workgroup and the LDS tile, every topic key alone, specs of four keys mixing the three sets, extremes,
  every k, failed scenarios, two LDS patterns, bounds on topic keys inside and outside the spec, garbage in the reserved word, and
  the parent code paths' bytes for specs without a topic key.
- The what-if batch of 302 variants, each test with the guard that keeps it meaningful.
- Refusals in their order, the host call planner (the combined call's decisions, the existing calls' bytes), the ABI, the exports,
  and WhatIf.best / WhatIf.front routed by criterion name.
"""
import ctypes as C
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import test_choose_cpu as tc
import test_front_cpu as tf
import test_moves_cpu as tm
import test_rack_choose_cpu as trc
import test_topics_cpu as ttp
import topic_choose_ref as R
from choose_ref import assert_same_choice, offsets_ref
from front_ref import NOT_OK, OVER_LIMIT, assert_same_front, cut
from impact_batches import solved
from kafka_assigner_amd import abi, native
from kafka_assigner_amd.flatten import batch_desc
from rack_ref import rack_counts, rack_ref
from test_choose_cpu import SENTINEL, k_largest, own_cur_form, synthetic
from topic_ref import topic_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "kafka-assigner_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "kas_abi.h")
E_INVALID, E_UNSUPPORTED = abi.KAS_E_INVALID_ARG, abi.KAS_E_UNSUPPORTED
TOP = 2**31 - 1
S_VALUES = [1, 2, 63, 64, 65, 255, 256, 257, 1025, 2049]
TOPIC_NAMES = abi.TOPIC_KEY_NAMES
# four keys each (position 4 of the packed entry), the three sets between them
MIXED = [("max_topic_inbound", "colocated_after", "replica_spread", "moved_replicas"),
         ("topics_moved", "rack_replica_spread", "sum_topic_leader_spread", "max_inbound")]
NO_RACKS = "rack criterion without rack records"
NO_TOPICS = "topic criterion without topic records"
_LIB = None


# ---- the emulator ---------------------------------------------------------------------------------------------------------
def _emu_lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    so = os.path.join(EMU, "libkas_emu_topic_choose.so")
    srcs = [os.path.join(EMU, "topic_choose_driver.cpp"), os.path.join(EMU, "emu_driver.cpp")]
    deps = srcs + [os.path.join(EMU, "kas_wave.h"), HEADER] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        tmp = so + ".tmp%d" % os.getpid()
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unused-parameter", "-Wno-unknown-pragmas",
                               "-I" + os.path.join(ROOT, "tests"), "-I" + CSRC, "-I" + os.path.join(ROOT, "include"),
                               "-o", tmp] + srcs)
        os.replace(tmp, so)
    L = C.CDLL(so)
    L.kas_emu_topic_rank.restype = C.c_int
    L.kas_emu_topic_rank.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(abi.FrontSpec),
                                     C.POINTER(abi.ChooseSpec), C.c_int] + [C.c_void_p] * 8 + [C.c_uint32, C.c_char_p, C.c_int]
    L.kas_emu_topic_choose.restype = C.c_int
    L.kas_emu_topic_choose.argtypes = [C.POINTER(abi.BatchDesc), C.POINTER(abi.Tables), C.POINTER(abi.ImpactTables), C.c_void_p, C.c_void_p,
                                       C.c_int, C.POINTER(abi.FrontSpec), C.POINTER(abi.ChooseSpec), C.POINTER(abi.Choice), C.c_void_p,
                                       C.c_uint32, C.c_char_p, C.c_int]
    L.kas_emu_topic_choose_host_call.restype = C.c_int
    L.kas_emu_topic_choose_host_call.argtypes = [C.POINTER(abi.BatchDesc), C.POINTER(C.c_int64), C.c_uint, C.c_int, C.POINTER(abi.FrontSpec),
                                                 C.POINTER(abi.ChooseSpec), C.POINTER(abi.Moves), C.c_int, C.c_int, C.c_int, C.c_int,
                                                 C.c_void_p, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_char_p, C.c_int]
    L.kas_emu_topic_choose_buffers.restype = C.c_int
    _LIB = L
    return L


def _id(x):
    return abi.topic_key_id(x) if isinstance(x, str) else int(x)


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


def _p(a):
    return None if a is None else a.ctypes.data


def emu_topic_rank(sr, si, srk, stp, keys, k, within=None, cells=None, n_nodes=None, lds_fill=0xCDCDCDCD, path=0):
    """kas_emu_topic_rank: a ranking (within is None) or a front; every output pre-filled with a sentinel, one element behind every
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
    rc = _emu_lib().kas_emu_topic_rank(sr.ctypes.data, si.ctypes.data, _p(srk), _p(stp), S,
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


def emu_refusal(sr, si, srk, stp, keys, k, within=None, **kw):
    """(rc, text) of kas_emu_topic_rank for a spec built without checks"""
    out = np.zeros(16, np.int32)
    err = C.create_string_buffer(256)
    fs, cs = (_fspec(keys, k, within, **kw), None) if within is not None else (None, _cspec(keys, k, **kw))
    rc = _emu_lib().kas_emu_topic_rank(sr.ctypes.data, si.ctypes.data, _p(srk), _p(stp), int(sr.shape[0]),
                                       None if fs is None else C.byref(fs), None if cs is None else C.byref(cs), 0, None, None,
                                       out.ctypes.data, out.ctypes.data, None, None, out.ctypes.data, out.ctypes.data, 0, err, 256)
    return rc, err.value.decode()


# ---- synthetic records ----------------------------------------------------------------------------------------------------
def synthetic_topics(S, seed, values=4, reserved=0):
    """S scenario topic records, every criterion word drawn from `values` (an int: 0..values-1; a list: those values); the
    sixteenth word is `reserved` (0, as the topic pass leaves it, or an array of anything)"""
    rng = np.random.default_rng([seed, S, 48])
    pool = np.arange(values) if isinstance(values, int) else np.asarray(values, dtype=np.int64)
    stp = np.zeros(S, abi.SCENARIO_TOPIC_IMPACT_DTYPE)
    for f in abi.SCENARIO_TOPIC_FIELDS:
        stp[f] = pool[rng.integers(0, pool.size, S)]
    stp["reserved"] = reserved
    return stp


def records(S, seed, values=4, failed="random"):
    sr, si = synthetic(S, seed, values=values, failed=failed)
    return sr, si, trc.synthetic_racks(S, seed, values=values), synthetic_topics(S, seed, values=values)


def _sizes(S, k):
    rng = np.random.default_rng(S + k)
    return rng.integers(0, 7, S) * 3 + (np.arange(S) % 5 == 0), rng.integers(0, 50, S)     # (odd sizes and zeros among them)


def _check_rank(sr, si, srk, stp, keys, k, what, sized=True, lds_fill=0xCDCDCDCD, path=0):
    S = int(sr.shape[0])
    cells, n_nodes = _sizes(S, k) if sized else (None, None)
    want = R.rank_ref(sr, si, srk, stp, keys, k)
    got = emu_topic_rank(sr, si, srk, stp, keys, k, None, cells, n_nodes, lds_fill=lds_fill, path=path)
    assert got.n_ok == want.n_ok, (what, got.n_ok, want.n_ok)
    assert np.array_equal(got.rank, want.rank), (what, "rank", np.nonzero(got.rank != want.rank)[0][:5])
    assert np.array_equal(got.chosen, want.chosen), (what, "chosen", got.chosen[:8], want.chosen[:8])
    if sized:
        assert np.array_equal(got.row_off, offsets_ref(want.order, cells, k)), (what, "row_off")
        assert np.array_equal(got.node_off, offsets_ref(want.order, n_nodes, k)), (what, "node_off")
    return want


def _check_front(sr, si, srk, stp, keys, k, what, within=(), sized=True, lds_fill=0xCDCDCDCD, base=None, path=0):
    """base: the checker's front of the same records and spec at another k (the O(S^2) pass is then not repeated)"""
    S = int(sr.shape[0])
    cells, n_nodes = _sizes(S, k) if sized else (None, None)
    want = R.front_of(sr, si, srk, stp, keys, k, within) if base is None else cut(base, k)
    if sized:
        want.row_off, want.node_off = offsets_ref(want.order, cells, k), offsets_ref(want.order, n_nodes, k)
    got = emu_topic_rank(sr, si, srk, stp, keys, k, within, cells, n_nodes, lds_fill=lds_fill, path=path)
    assert got.n_ok == want.n_ok, (what, got.n_ok, want.n_ok)
    assert_same_front(want, got, what)
    return want


_ks = trc._ks


def _front_every_k(sr, si, srk, stp, keys, what, within=()):
    want = R.front_of(sr, si, srk, stp, keys, 0, within)
    for k in _ks(int(sr.shape[0]), int(want.order.size)):
        _check_front(sr, si, srk, stp, keys, k, f"{what} k={k}", within, base=want)
    return want


@pytest.mark.parametrize("S", S_VALUES)
def test_emulated_every_topic_key_alone(S):
    """every topic criterion alone, ranked (every k of _ks) and fronted, criteria from {0..3}: the index decides most comparisons;
    the front of one criterion is the first of the smallest.  No rack records are given: srk is NULL."""
    sr, si, _, stp = records(S, 1)
    n_ok = int((sr["status"] == 0).sum())
    for name in TOPIC_NAMES:
        for k in _ks(S, n_ok):
            want = _check_rank(sr, si, None, stp, (name,), k, f"S={S} {name} k={k}")
        if S >= 64 and n_ok >= 16:                              # (the records do tie: the guard of this test)
            first = R.criterion(sr, si, None, stp, name)[want.order]
            assert np.unique(first).size <= 4 < first.size
        front = _front_every_k(sr, si, None, stp, (name,), f"S={S} front {name}")
        assert front.order.size == (1 if n_ok else 0)
    # the checker reads the record as the header lays it out: word i is key KAS_KEY_TOPIC_BASE + i, and word 15 is no key
    words = stp.view(np.int32).reshape(S, 16)
    for i, name in enumerate(TOPIC_NAMES):
        assert np.array_equal(R.criterion(sr, si, None, stp, abi.KAS_KEY_TOPIC_BASE + i), words[:, i]) and abi.TOPIC_KEYS[name] == 48 + i
    assert len(TOPIC_NAMES) == 15 and abi.SCENARIO_TOPIC_IMPACT_DTYPE.names[15] == "reserved"


@pytest.mark.parametrize("S", S_VALUES)
def test_emulated_specs_mixing_the_three_key_sets(S):
    """two specs of four criteria from the three sets: rankings for every k, and fronts of values from {0..63} for every k; the
    second spec once with four bounds"""
    sr, si, srk, stp = records(S, 2)
    n_ok = int((sr["status"] == 0).sum())
    for keys in MIXED:
        for k in _ks(S, n_ok):
            _check_rank(sr, si, srk, stp, keys, k, f"S={S} {keys} k={k}")
    _check_rank(sr, si, srk, stp, MIXED[0], min(S, 3), f"S={S} rank only", sized=False)
    sr, si, srk, stp = records(S, 2, values=64)
    for keys in MIXED:
        want = _front_every_k(sr, si, srk, stp, keys, f"S={S} wide {keys}")
        if S >= 257:
            assert want.order.size >= 10, want.order.size
    four = {"max_topic_outbound": 50, "max_rack_inbound": 50, "leaders_moved": 50, "topics_departed": 40}
    want = _front_every_k(sr, si, srk, stp, MIXED[1], f"S={S} four bounds", four)
    if S >= 257:
        assert (want.classes == OVER_LIMIT).any() and want.order.size >= 2
    _check_front(sr, si, srk, stp, MIXED[1], min(S, 3), f"S={S} front, rank only", sized=False)


@pytest.mark.parametrize("S", [2, 257, 1025])
def test_emulated_extreme_values(S):
    """topic words at 0 and at 2^31 - 1, among failed scenarios"""
    sr, si, srk, stp = records(S, 4, values=[0, TOP], failed="alternate")
    for keys in [(name,) for name in TOPIC_NAMES] + MIXED:
        assert set(np.unique(R.criterion(sr, si, srk, stp, keys[0]))) <= {0, TOP}
        _check_rank(sr, si, srk, stp, keys, S, f"S={S} extremes {keys}")
    for keys in MIXED + [("max_topic_replica_spread", "sum_topic_replica_spread")]:
        _check_front(sr, si, srk, stp, keys, S, f"S={S} extremes front {keys}")
    sr, si, srk, stp = records(S, 5, values=[TOP])
    _check_rank(sr, si, srk, stp, MIXED[1], S, f"S={S} every criterion 2^31 - 1")
    _check_front(sr, si, srk, stp, MIXED[0], S, f"S={S} every criterion 2^31 - 1", within={"max_topic_inbound": TOP})


@pytest.mark.parametrize("S", S_VALUES)
@pytest.mark.parametrize("failed", ["none", "alternate", "all"])
def test_emulated_failed_scenarios_and_every_k(S, failed):
    sr, si, srk, stp = records(S, 2, failed=failed)
    n_ok = int((sr["status"] == 0).sum())
    assert n_ok == {"none": S, "alternate": (S + 1) // 2, "all": 0}[failed]
    for k in _ks(S, n_ok):
        want = _check_rank(sr, si, srk, stp, ("topics_departed", "max_outbound"), k, f"S={S} failed={failed} k={k}")
        if failed == "all":
            assert want.n_ok == 0 and (want.chosen == -1).all() and (want.rank == -1).all()
    # an antichain over a topic criterion and a broker criterion: every OK scenario is a member, and k cuts the front
    perm = np.random.default_rng(S).permutation(S).astype(np.int32)
    stp["max_topic_inbound"], sr["moved_replicas"] = perm, S - perm
    want = _front_every_k(sr, si, srk, stp, ("max_topic_inbound", "moved_replicas"), f"S={S} antichain {failed}")
    assert want.order.size == n_ok and (want.classes[sr["status"] == 0] == 0).all()
    if failed == "all":
        assert (want.chosen == -1).all() and (want.rank == NOT_OK).all() and want.counts.tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("fill", [0, 0xFFFFFFFF])
def test_emulated_whatever_the_lds_holds(fill):
    """LDS is uninitialised on hardware: zeros (the smallest key, flags clear) and all ones (flags set everywhere)"""
    for S in (65, 1025):
        sr, si, srk, stp = records(S, 6, values=64)
        _check_rank(sr, si, srk, stp, MIXED[1], S // 2, f"S={S} lds {fill:#x}", lds_fill=fill)
        _check_front(sr, si, srk, stp, MIXED[0], S // 2, f"S={S} lds {fill:#x}", within={"max_topic_outbound": 40}, lds_fill=fill)


@pytest.mark.parametrize("S", [1, 65, 257, 1025, 2049])
def test_emulated_bounds_on_topic_keys(S):
    """bounds on topic criteria inside and outside the spec, beside a broker and a rack bound, limit 2^31 - 1, and a bound nobody meets"""
    sr, si, srk, stp = records(S, 7, values=64)
    keys = ("max_topic_inbound", "moved_replicas")
    free = R.front_of(sr, si, srk, stp, keys, 0)
    cases = [{}, {"max_topic_inbound": 30}, {"max_topic_outbound": 20}, {"sum_topic_replica_spread": 20, "moved_replicas": 40},
             {"max_topic_outbound": 30, "leaders_moved": 30, "colocated_after": 30, "max_topic_inbound": 50},
             {"max_topic_leader_spread": TOP}, {"topics_departed": TOP, "max_inbound": TOP}]
    for within in cases:
        want = _front_every_k(sr, si, srk, stp, keys, f"S={S} within {within}", within)
        if S >= 257 and within == {"max_topic_inbound": 30}:                # inside the spec: the bound only filters the front
            assert set(want.order) <= set(free.order) and (want.classes == OVER_LIMIT).any()
        if S >= 257 and within == {"max_topic_outbound": 20}:               # outside: it creates members
            assert not set(want.order) <= set(free.order)
        if TOP in within.values():
            assert np.array_equal(want.rank, free.rank)
    stp["topics_departed"] += 1                                             # a bound nobody meets: the front is empty
    want = _check_front(sr, si, srk, stp, keys, min(S, 3), f"S={S} nobody", within={"topics_departed": 0})
    assert want.counts[1] == 0 and want.counts[2] == 0 and (want.chosen == -1).all() and (want.row_off == 0).all()
    assert set(np.unique(want.rank)) <= {NOT_OK, OVER_LIMIT}


@pytest.mark.parametrize("S", [65, 1025])
def test_garbage_in_the_reserved_word_changes_nothing(S):
    """word 15 of the record is no criterion: whatever it holds, every output's bytes are those of a record with 0 there"""
    sr, si, srk, stp = records(S, 9)
    junk = stp.copy()
    junk["reserved"] = np.random.default_rng(S).integers(-2**31, 2**31, S).astype(np.int32)
    assert (junk["reserved"] != 0).sum() >= S - 1
    k = S // 2
    cells, n_nodes = _sizes(S, k)
    for keys, within in ((("sum_topic_leader_spread",), None), (MIXED[1], None), (MIXED[0], {"sum_topic_leader_spread": 2}),
                         (("sum_topic_leader_spread", "max_topic_leaders_after"), {})):
        a = emu_topic_rank(sr, si, srk, stp, keys, k, within, cells, n_nodes)
        b = emu_topic_rank(sr, si, srk, junk, keys, k, within, cells, n_nodes)
        for f in ("rank", "chosen", "row_off", "node_off", "counts"):
            assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), (keys, f)
        assert a.n_ok == b.n_ok


@pytest.mark.parametrize("S", [1, 65, 256, 1025])
def test_specs_without_topic_keys_give_the_parent_code_paths_bytes(S):
    """a spec without a topic criterion through the new code path (the instance the library launches, and the topic instance with
    srk NULL and non-NULL): the bytes of the *_racks path and, without a rack criterion, of the oldest path"""
    sr, si, srk, stp = records(S, 8)
    k = S // 2
    cells, n_nodes = _sizes(S, k)
    fields = ("rank", "chosen", "row_off", "node_off")
    for keys in (tc.MULTI_SPECS[0], tc.MULTI_SPECS[2]):                     # broker keys only: srk may be NULL
        oldest = tc.emu_rank(sr, si, keys, k, cells, n_nodes)
        racks = trc.emu_rack_rank(sr, si, srk, keys, k, None, cells, n_nodes, path=1)
        for given, topics, path in ((None, None, 0), (srk, stp, 0), (None, stp, 2), (srk, stp, 2), (srk, stp, 1)):
            mine = emu_topic_rank(sr, si, given, topics, keys, k, None, cells, n_nodes, path=path)
            for f in fields:
                assert getattr(mine, f).tobytes() == getattr(oldest, f).tobytes() == getattr(racks, f).tobytes(), (keys, f, path)
            assert mine.n_ok == oldest.n_ok
        within = {"max_outbound": 2}
        oldest = tf.emu_front_rank(sr, si, keys, k, within, cells, n_nodes)
        for given, topics, path in ((None, None, 0), (srk, stp, 0), (None, stp, 2), (srk, stp, 2)):
            mine = emu_topic_rank(sr, si, given, topics, keys, k, within, cells, n_nodes, path=path)
            for f in fields + ("counts",):
                assert getattr(mine, f).tobytes() == getattr(oldest, f).tobytes(), (keys, f, path)
    for keys, within in ((trc.MIXED[0], None), (trc.MIXED[2], None), (trc.MIXED[1], {"max_rack_outbound": 2})):   # rack keys: srk is read
        racks = trc.emu_rack_rank(sr, si, srk, keys, k, within, cells, n_nodes)
        for topics, path in ((None, 0), (stp, 0), (stp, 2)):
            mine = emu_topic_rank(sr, si, srk, topics, keys, k, within, cells, n_nodes, path=path)
            for f in fields + ("counts",):
                assert getattr(mine, f).tobytes() == getattr(racks, f).tobytes(), (keys, f, path)


def test_refusals_in_their_order_each_with_its_text():
    """the spec refusals of the parents with the key set widened twice and the same texts, then the missing rack records, then the
    missing topic records; every case has every later refusal pending"""
    sr, si, srk, stp = records(8, 7)
    good = ("max_topic_inbound", "colocated_after")
    cases = [(dict(keys=good, k=1, n_keys=0), "kas_choose_spec: n_keys outside 1..4"), (dict(keys=good, k=1, n_keys=5), "n_keys outside 1..4"),
             (dict(keys=(10,), k=-1), "kas_choose_spec: unknown criterion"), (dict(keys=(15,), k=-1), "unknown criterion"),
             (dict(keys=(33,), k=-1), "unknown criterion"), (dict(keys=(47,), k=-1), "unknown criterion"),
             (dict(keys=(63,), k=-1), "unknown criterion"), (dict(keys=(55, -1), k=-1), "unknown criterion"),
             (dict(keys=good, k=-1), "kas_choose_spec: k outside"), (dict(keys=good, k=9), "k outside"),
             (dict(keys=(63,), k=-1, within=[(63, -1)], n_keys=0, n_limits=5), "kas_front_spec: n_keys outside 1..4"),
             (dict(keys=(63,), k=-1, within=[(63, -1)], n_limits=5), "kas_front_spec: unknown criterion"),
             (dict(keys=good, k=-1, within=[(63, -1)], n_limits=5), "n_limits outside 0..4"),
             (dict(keys=good, k=-1, within=[(55, -1), (47, -1)]), "unknown limit criterion"),
             (dict(keys=good, k=-1, within=[(55, -1), (33, -1)]), "unknown limit criterion"),
             (dict(keys=good, k=-1, within=[(55, -1), (15, -1)]), "unknown limit criterion"),
             (dict(keys=good, k=-1, within=[(55, 3), (62, -1)]), "negative limit"),
             (dict(keys=good, k=-1, within=[(62, 3)]), "kas_front_spec: k outside")]
    for kw, text in cases:
        for given, topics in ((srk, stp), (None, None)):                    # (the spec's refusals come before the missing records)
            rc, err = emu_refusal(sr, si, given, topics, **kw)
            assert rc == E_INVALID and text in err, (kw, rc, err)
    for kw in (dict(keys=good, k=1), dict(keys=good, k=1, within=[]), dict(keys=("max_topic_inbound",), k=1, within=[("n_racks", 3)]),
               dict(keys=("colocated_after",), k=1, within=[("topics_moved", 3)])):
        rc, err = emu_refusal(sr, si, None, None, **kw)                     # both missing: the rack records first
        assert rc == E_INVALID and err == NO_RACKS, (kw, rc, err)
        rc, err = emu_refusal(sr, si, None, stp, **kw)
        assert rc == E_INVALID and err == NO_RACKS, (kw, rc, err)
        rc, err = emu_refusal(sr, si, srk, None, **kw)
        assert rc == E_INVALID and err == NO_TOPICS, (kw, rc, err)
        assert emu_refusal(sr, si, srk, stp, **kw)[0] == 0
    # the two sources are independent
    assert emu_refusal(sr, si, None, stp, keys=("max_topic_inbound", "moved_replicas"), k=1)[0] == 0
    assert emu_refusal(sr, si, srk, None, keys=("colocated_after", "moved_replicas"), k=1)[0] == 0
    assert emu_refusal(sr, si, None, None, keys=("moved_replicas",), k=1, within=[("max_inbound", 3)])[0] == 0
    rc, err = emu_refusal(sr, si, None, None, keys=("moved_replicas",), k=1, within=[("topics_ok", 3)])
    assert rc == E_INVALID and err == NO_TOPICS
    # the entries that were there know no topic criterion: the *_racks code path and the oldest
    for keys, within in ((("max_topic_inbound",), None), (("moved_replicas",), [(48, 1)]), ((62,), None)):
        rc, err = trc.emu_refusal(sr, si, srk, keys=[_id(x) for x in keys], k=1, within=within)
        assert rc == E_INVALID and "unknown" in err and "criterion" in err, (keys, rc, err)
    out = np.zeros(16, np.int32)
    err = C.create_string_buffer(256)
    spec = _cspec(("topics_ok",), 1)
    rc = tc._emu_lib().kas_emu_rank(sr.ctypes.data, si.ctypes.data, 8, C.byref(spec), None, None, out.ctypes.data, out.ctypes.data, None, None,
                                    out.ctypes.data, 0, err, 256)
    assert rc == E_INVALID and "unknown criterion" in err.value.decode()


# ---- rank / mark / front rank and gather over solved batches ----------------------------------------------------------------
GUARD_CELLS, GUARD_NODES = 64, 3


def emu_topic_choose(fb, out, sr, imp, srk, stp, keys, k, within=None, mode=0, lds_fill=0xCDCDCDCD):
    """kas_emu_topic_choose over the tables of a solve, its impact records, its scenario rack records and its scenario topic
    records: a choice (within is None) or a front; capacities exactly the k largest scenarios', guards behind them"""
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
    rc = _emu_lib().kas_emu_topic_choose(C.byref(bd), C.byref(t), C.byref(itab), _p(srk), _p(stp), mode,
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


_WHATIF_TOPICS = None


def whatif_topics():
    """(WhatIf, variants, fb, the oracle's solve, the checker's impact records, the checker's scenario rack records, the report
    table, the rack names, the checker's topic records, its scenario topic records), computed once"""
    global _WHATIF_TOPICS
    if _WHATIF_TOPICS is None:
        w, vs, fb, ho, imp, srk, table, names = trc.whatif_racks()
        tt, stp = topic_ref(fb, ho)
        _WHATIF_TOPICS = (w, vs, fb, ho, imp, srk, table, names, tt, stp)
    return _WHATIF_TOPICS


WHATIF_MAX = ("max_topic_replica_spread", "moved_replicas")
WHATIF_SUM = ("sum_topic_replica_spread", "moved_replicas")
WHATIF_FRONT_A = (("moved_replicas", "max_topic_replica_spread"), {"topics_departed": 0})
WHATIF_FRONT_B = (("moved_replicas", "max_topic_inbound", "sum_topic_leader_spread"), {})


def test_emulated_choice_of_the_whatif_batch_by_topic_criteria():
    _, _, fb, ho, imp, srk, _, _, _, stp = whatif_topics()
    S = fb.n_scenarios
    sr, si = ho.scenario_results[:S], imp[1][:S]
    ok = sr["status"] == 0
    n_ok = int(ok.sum())
    assert S == 302 and n_ok == 184 and int(fb.scen["topic_count"][0]) == 2
    # the guards, on the reference alone: the topic figures order the variants differently from the broker figures, and at least
    # 20 solved variants tie on the first criterion of each spec
    broker = R.rank_ref(sr, si, srk, stp, ("replica_spread", "moved_replicas"), 4).chosen.tolist()
    by_max = R.rank_ref(sr, si, srk, stp, WHATIF_MAX, 4).chosen.tolist()
    by_sum = R.rank_ref(sr, si, srk, stp, WHATIF_SUM, 4).chosen.tolist()
    print("what-if rankings start", broker, by_max, by_sum)
    assert broker == [46, 73, 273, 23] and by_max == [233, 46, 59, 4] and by_sum == [115, 233, 242, 269]
    for keys in (WHATIF_MAX, WHATIF_SUM):
        first = stp[keys[0]][ok]
        ties = int(first.size - np.unique(first).size)
        print("what-if ties on", keys[0], ties)
        assert ties >= 20
    assert int((stp["topics_departed"][ok] == 0).sum()) == 36 and int((stp["max_topic_inbound"][ok] <= 40).sum()) == 80
    for keys, ks in ((WHATIF_MAX, (1, 5, n_ok, n_ok + 1, S)), (WHATIF_SUM, (5,)), (MIXED[0], (5,))):
        for k in ks:
            want = R.choose_of(fb, sr, ho.out, imp, srk, stp, keys, k)
            got = emu_topic_choose(fb, ho.out, sr, imp, srk if keys == MIXED[0] else None, stp, keys, k)
            assert_same_choice(want, got, f"what-if {keys} k {k}")
    # 16-bit cells and the narrowing gather, at one k
    fb16 = own_cur_form(fb)
    for mode, out, ref_out in tc._forms(fb16, ho)[1:]:
        want = R.choose_of(fb16, sr, ref_out, imp, srk, stp, WHATIF_SUM, 5)
        assert_same_choice(want, emu_topic_choose(fb16, out, sr, imp, None, stp, WHATIF_SUM, 5, mode=mode), f"what-if mode {mode}")


def _same(want, got, what):
    assert_same_front(want, got, what)
    assert_same_choice(want, got, what)


def test_emulated_front_of_the_whatif_batch_by_topic_criteria():
    _, _, fb, ho, imp, srk, _, _, _, stp = whatif_topics()
    S = fb.n_scenarios
    sr, si = ho.scenario_results[:S], imp[1][:S]
    fronts = []
    for keys, within in (WHATIF_FRONT_A, WHATIF_FRONT_B):
        f = R.front_of(sr, si, srk, stp, keys, 0, within)
        n_front, n_eligible = int(f.counts[2]), int(f.counts[1])
        print("what-if front", keys, within, "members", n_front, "eligible", n_eligible)
        assert 2 <= n_front < n_eligible                                    # the guards, on the reference alone
        fronts.append((keys, within, n_front))
    bounded = R.front_of(sr, si, srk, stp, *WHATIF_FRONT_A[:1], 0, WHATIF_FRONT_A[1])
    assert 1 <= int(bounded.counts[1]) <= 183 and int(bounded.counts[1]) == 36 and (bounded.classes == OVER_LIMIT).any()
    fb16 = own_cur_form(fb)
    forms = tc._forms(fb16, ho)
    for keys, within, n_front in fronts:
        for k in (1, n_front, n_front + 1, S) if within else (n_front,):
            for mode, out, ref_out in forms if k == n_front else forms[:1]:
                want = R.front_choice_of(fb16 if mode else fb, sr, ref_out, imp, srk, stp, keys, k, within)
                got = emu_topic_choose(fb16 if mode else fb, out, sr, imp, None, stp, keys, k, within, mode=mode)
                _same(want, got, f"what-if {keys} {within} k {k} mode {mode}")
                assert want.counts[2] == n_front
        # the moves of the members, in member order (the moves pass takes the front's chosen[], -1 tail and all)
        want = R.front_of(sr, si, srk, stp, keys, n_front + 1, within)
        assert want.chosen[-1] == -1
        tm.check(fb, fb.cur, ho, [int(s) for s in want.chosen], 7, 0, f"what-if moves {keys} {within}")


@pytest.mark.parametrize("name", ["mixed42", "degenerate"])
def test_emulated_choice_front_and_gather_for_every_k(name):
    """oracle-solved batches: every k, both cell layouts and the narrowing gather, topic keys alone (srk NULL) and mixed"""
    fb, ho, imp = solved(name)
    S = fb.n_scenarios
    forms = tc._forms(fb, ho)
    srk = rack_ref(fb, ho, None)[1]
    stp = topic_ref(fb, ho)[1]
    for k in range(0, S + 1):
        for mode, out, ref_out in forms if k in (1, S) else forms[:1]:
            keys = ("max_topic_inbound", "moved_replicas") if k % 2 else ("sum_topic_replica_spread", "rack_replica_spread", "leaders_moved", "topics_moved")
            given = None if k % 2 else srk
            want = R.choose_of(fb, ho.scenario_results, ref_out, imp, srk, stp, keys, k)
            got = emu_topic_choose(fb, out, ho.scenario_results[:S], imp, given, stp, keys, k, mode=mode)
            assert_same_choice(want, got, f"{name} mode {mode} k {k} {keys}")
            want = R.front_choice_of(fb, ho.scenario_results, ref_out, imp, srk, stp, keys, k, {"max_topic_outbound": 10**6})
            got = emu_topic_choose(fb, out, ho.scenario_results[:S], imp, given, stp, keys, k, {"max_topic_outbound": 10**6}, mode=mode)
            _same(want, got, f"{name} front mode {mode} k {k} {keys}")


# ---- the planner ----------------------------------------------------------------------------------------------------------
HOST_BUFS = ttp.HOST_BUFS
MISSING = dict(trc.MISSING, imp_nodes=64, tp_topics=524288, tp_scenarios=1048576)
HEAD = trc.HEAD + ("region_ints",)
_BUF = np.zeros(16, np.int64)


def topic_choose_host_call(fb, front=None, spec=None, mv=None, rows_cap=None, nodes_cap=None, racks_cap=None, racks=True, rack_keys=True,
                           topics=True, topic_keys=True, report_rack=None, missing=(), cells16=False, n_select=0):
    """kas_plan_host_call for a kas_solve_host_front_topics call (front) or a kas_solve_host_choose_topics call (spec); rack_keys /
    topic_keys False plan the call of the same arguments that knows no criterion of that set; neither front nor spec: the
    topic-impact call (topics) or the impact call: (rc, plan or None, text)"""
    L = _emu_lib()
    assert L.kas_emu_topic_choose_buffers() == len(HOST_BUFS)
    bd = batch_desc(fb)
    if cells16:
        bd.node_id = None
    choice = front or spec
    need = k_largest(fb, choice.k) if choice else (0, 0)
    rep = None if report_rack is None else np.ascontiguousarray(report_rack, dtype=np.int32)
    try:
        rk_need = int(rack_counts(fb, rep).sum()) if racks else 0
    except ValueError:
        rk_need = 0
    lens = (C.c_int64 * 7)(int(fb.cur.shape[0]), int(fb.aux.shape[0]), int(fb.ctx.shape[0]), need[0] if rows_cap is None else rows_cap,
                           need[1] if nodes_cap is None else nodes_cap, rk_need if racks_cap is None else racks_cap, int(fb.out_len))
    head, nbytes = (C.c_int64 * len(HEAD))(), (C.c_int64 * len(HOST_BUFS))()
    err = C.create_string_buffer(512)
    rc = L.kas_emu_topic_choose_host_call(C.byref(bd), lens, sum(MISSING[m] for m in missing), int(cells16),
                                          None if front is None else C.byref(front), None if spec is None else C.byref(spec),
                                          None if mv is None else C.byref(mv), int(racks), int(rack_keys), int(topics), int(topic_keys),
                                          None if rep is None else rep.ctypes.data, n_select, head, nbytes, err, 512)
    if rc != 0:
        return rc, None, err.value.decode()
    plan = dict(zip(HEAD, [int(v) for v in head]))
    plan["bytes"] = dict(zip(HOST_BUFS, [int(v) for v in nbytes]))
    return rc, plan, ""


def _mv(mask=7, moves_cap=10**6, cells_cap=10**7):
    b = _BUF.ctypes.data
    return abi.Moves(mask, 0, b, b, b, moves_cap, b, cells_cap)


def test_planner_refuses_in_order_each_with_its_text():
    """the spec (key set widened twice, the parents' texts), the missing rack records, the missing topic records, everything the
    *_racks call refuses in its order (the rack refusals last), then the topic refusals of kas_solve_host_topic_impact in their
    order: every case has every later refusal pending too"""
    fb, _, _ = solved("mixed42")
    S = fb.n_scenarios
    good = ("max_topic_inbound", "colocated_after", "leaders_moved")
    rows, nodes = k_largest(fb, 2)
    need = int(rack_counts(fb).sum())
    bad_mv = abi.Moves(9, 0, None, None, None, -1, None, -1)
    neg = fb.node_rack.copy(); neg[3] = -1
    big = fb.node_rack.copy(); big[5] = abi.KAS_RACK_LIMIT
    both = big.copy(); both[int(fb.scen["node_off"][1]) + 2] = -1
    tp_null = ("tp_topics", "tp_scenarios")
    late = dict(report_rack=both, racks_cap=0, missing=("rank", "counts", "rk_off") + tp_null, mv=bad_mv)
    every = dict(rows_cap=0, nodes_cap=0, **late)
    rk = dict(report_rack=both, racks_cap=0, missing=("rk_off",) + tp_null)
    order = [(dict(front=_fspec((63,), -1, [(63, -1)], n_keys=0, n_limits=5), **every), E_INVALID, "kas_front_spec: n_keys outside 1..4"),
             (dict(front=_fspec((63,), -1, [(63, -1)], n_limits=5), **every), E_INVALID, "kas_front_spec: unknown criterion"),
             (dict(front=_fspec((47,), -1, [(63, -1)], n_limits=5), **every), E_INVALID, "kas_front_spec: unknown criterion"),
             (dict(front=_fspec(good, -1, [(63, -1)], n_limits=5), **every), E_INVALID, "n_limits outside 0..4"),
             (dict(front=_fspec(good, -1, [(33, -1)]), **every), E_INVALID, "unknown limit criterion"),
             (dict(front=_fspec(good, -1, [(15, -1)]), **every), E_INVALID, "unknown limit criterion"),
             (dict(front=_fspec(good, -1, [(55, -1)]), **every), E_INVALID, "negative limit"),
             (dict(front=_fspec(good, -1, [(55, 1)]), **every), E_INVALID, "kas_front_spec: k outside"),
             (dict(front=_fspec(good, S + 1, [(55, 1)]), **every), E_INVALID, "k outside"),
             (dict(spec=_cspec(good, 2, n_keys=5), **every), E_INVALID, "kas_choose_spec: n_keys outside 1..4"),
             (dict(spec=_cspec((63,), -1), **every), E_INVALID, "kas_choose_spec: unknown criterion"),
             (dict(spec=_cspec((33,), -1), **every), E_INVALID, "kas_choose_spec: unknown criterion"),
             (dict(spec=_cspec(good, -1), **every), E_INVALID, "kas_choose_spec: k outside"),
             (dict(front=_fspec(good, 2), racks=False, topics=False, **every), E_INVALID, NO_RACKS),
             (dict(front=_fspec(("moved_replicas",), 2, [(32, 5), (48, 5)]), racks=False, topics=False, **every), E_INVALID, NO_RACKS),
             (dict(spec=_cspec(good, 2), racks=False, topics=False, **every), E_INVALID, NO_RACKS),
             (dict(front=_fspec(good, 2), topics=False, **every), E_INVALID, NO_TOPICS),
             (dict(front=_fspec(("moved_replicas",), 2, [(32, 5), (48, 5)]), topics=False, **every), E_INVALID, NO_TOPICS),
             (dict(spec=_cspec(good, 2), topics=False, **every), E_INVALID, NO_TOPICS),
             (dict(spec=_cspec(("topics_ok",), 2), racks=False, topics=False, **every), E_INVALID, NO_TOPICS),
             (dict(front=_fspec(good, 2), rows_cap=rows - 1, nodes_cap=0, **late), E_INVALID, "rows_cap below"),
             (dict(spec=_cspec(good, 2), rows_cap=rows - 1, nodes_cap=0, **late), E_INVALID, "rows_cap below"),
             (dict(front=_fspec(good, 2), nodes_cap=nodes - 1, **late), E_INVALID, "nodes_cap below"),
             (dict(front=_fspec(good, 2), **late), E_INVALID, "an array the call writes is NULL"),
             (dict(spec=_cspec(good, 2), mv=bad_mv, **rk), E_INVALID, "mask outside 1..7"),
             (dict(spec=_cspec(good, 2), **rk), E_INVALID, "negative"),
             (dict(front=_fspec(good, 2), mv=_mv(), **rk), E_INVALID, "negative"),
             (dict(spec=_cspec(good, 2), report_rack=neg, racks_cap=0, missing=("rk_off",) + tp_null), E_INVALID, "negative"),
             (dict(spec=_cspec(good, 2), report_rack=big, racks_cap=0, missing=("rk_off",) + tp_null), E_UNSUPPORTED, "KAS_RACK_LIMIT"),
             (dict(spec=_cspec(good, 2), racks_cap=need - 1, missing=("rk_off",) + tp_null), E_INVALID, "racks_cap below"),
             (dict(front=_fspec(good, 2), missing=("rk_off",) + tp_null), E_INVALID, "racks / scenarios / rack_off == NULL"),
             (dict(spec=_cspec(good, 2), missing=("rk_racks",) + tp_null), E_INVALID, "racks / scenarios / rack_off == NULL"),
             (dict(spec=_cspec(good, 2), missing=tp_null), E_INVALID, "kas_topic_impact_tables: topics / scenarios == NULL"),
             (dict(front=_fspec(good, 2), missing=("tp_topics",)), E_INVALID, "kas_topic_impact_tables: topics / scenarios == NULL"),
             (dict(spec=_cspec(good, 2), missing=("tp_scenarios",), mv=_mv()), E_INVALID, "kas_topic_impact_tables: topics / scenarios == NULL")]
    for kw, code, text in order:
        rc, _, err = topic_choose_host_call(fb, **kw)
        assert rc == code and text in err, (text, rc, err)
    assert topic_choose_host_call(fb, spec=_cspec(good, 2))[0] == 0 and topic_choose_host_call(fb, front=_fspec(good, 2), mv=_mv())[0] == 0
    # the two sources are independent: a rack pass without a topic pass and the other way round
    assert topic_choose_host_call(fb, spec=_cspec(("colocated_after",), 2), topics=False)[0] == 0
    assert topic_choose_host_call(fb, spec=_cspec(("topics_ok",), 2), racks=False)[0] == 0
    assert topic_choose_host_call(fb, spec=_cspec(("moved_replicas",), 2), racks=False, topics=False)[0] == 0
    # the scratch limit, KAS_E_UNSUPPORTED, last of all: behind the NULL arrays of kas_topic_impact_tables
    over = ttp._many_global_topics(abi.KAS_TOPIC_SCRATCH_LIMIT // (4 * (4 * 11000 + 2)) + 1)
    spec = _cspec(("max_topic_inbound",), 0)
    rc, _, err = topic_choose_host_call(over, spec=spec, racks=False, missing=("tp_topics",))
    assert rc == E_INVALID and "kas_topic_impact_tables" in err, (rc, err)
    rc, _, err = topic_choose_host_call(over, spec=spec, racks=False)
    assert rc == E_UNSUPPORTED and "KAS_TOPIC_SCRATCH_LIMIT" in err, (rc, err)
    rc, _, err = topic_choose_host_call(over, spec=spec, racks=False, missing=("n_ok",))
    assert rc == E_INVALID and "an array the call writes is NULL" in err, (rc, err)
    assert topic_choose_host_call(over, spec=_cspec(("moved_replicas",), 0), racks=False, topics=False)[0] == 0
    # the calls that were there refuse every topic criterion as unknown, with topic records or without: the *_racks switches ...
    for topics in (True, False):
        rc, _, err = topic_choose_host_call(fb, spec=_cspec(good, 2), topic_keys=False, topics=topics)
        assert rc == E_INVALID and "unknown criterion" in err
        rc, _, err = topic_choose_host_call(fb, front=_fspec(("moved_replicas",), 2, [(55, 0)]), topic_keys=False, topics=topics)
        assert rc == E_INVALID and "unknown limit criterion" in err
        # ... and the oldest
        rc, _, err = topic_choose_host_call(fb, spec=_cspec(("topics_ok",), 2), rack_keys=False, topic_keys=False, topics=topics, racks=False)
        assert rc == E_INVALID and "unknown criterion" in err
    # ... through the driver that was there too
    rc, _, err = trc.rack_choose_host_call(fb, spec=_cspec(("topics_ok",), 2))
    assert rc == E_INVALID and "unknown criterion" in err


@pytest.mark.parametrize("cells16", [False, True], ids=["int32", "cells16"])
def test_planner_decisions_of_the_combined_call_and_bytes_of_the_calls_that_were_there(cells16):
    import emu_lib
    fb, _, _ = solved("mixed42")
    S, Tn, k = fb.n_scenarios, fb.n_topics, 3
    need = int(rack_counts(fb).sum())
    n_rack, n_front, n_moves = len(trc.HOST_BUFS), len(tf.HOST_BUFS), len(tm.HOST_BUFS)
    broker = ("moved_replicas", "leaders_moved")
    rack_keys = ("colocated_after", "leaders_moved")
    keys = ("max_topic_inbound", "colocated_after", "leaders_moved")
    shapes = (("choose", {}), ("choose_moves", dict(mv=_mv())), ("choose_moves_norows", dict(mv=_mv(), rows_cap=0, missing=("rows",))))
    for what, kw in shapes:
        want = tf.PARENT[(what, cells16)]
        # a plain choose through this driver: byte for byte what the Pareto front's tests pin, nothing behind
        rc, plan, err = topic_choose_host_call(fb, spec=_cspec(broker, k), racks=False, rack_keys=False, topics=False, topic_keys=False,
                                               cells16=cells16, **kw)
        assert rc == 0, err
        got = [plan["bytes"][n] for n in HOST_BUFS]
        assert got[:len(want)] == want and not any(got[len(want):]), (what, got)
        # the combined call without either pass (host_racks == NULL, host_topics == NULL): the same bytes whatever the switches say
        rc, plan, err = topic_choose_host_call(fb, spec=_cspec(broker, k), racks=False, topics=False, cells16=cells16, **kw)
        assert rc == 0 and [plan["bytes"][n] for n in HOST_BUFS] == got, err
        # a plain front and a racks choose / front through this driver and through the drivers that were there: the same
        fs = _fspec(broker, k, {"max_inbound": 100})
        rc, plan, err = topic_choose_host_call(fb, front=fs, racks=False, rack_keys=False, topics=False, topic_keys=False, cells16=cells16, **kw)
        rc2, theirs, err2 = tf.front_host_call(fb, front=fs, cells16=cells16, **kw)
        assert rc == 0 and rc2 == 0 and [plan["bytes"][n] for n in tf.HOST_BUFS] == [theirs["bytes"][n] for n in tf.HOST_BUFS], (err, err2)
        assert not any(plan["bytes"][n] for n in HOST_BUFS[n_front:])
        for spec_kw in (dict(spec=_cspec(rack_keys, k)), dict(front=_fspec(rack_keys, k, {"max_rack_inbound": 100}))):
            rc, theirs, err = trc.rack_choose_host_call(fb, cells16=cells16, **spec_kw, **kw)
            assert rc == 0, err
            rc, plan, err = topic_choose_host_call(fb, topics=False, topic_keys=False, cells16=cells16, **spec_kw, **kw)
            assert rc == 0 and [plan["bytes"][n] for n in trc.HOST_BUFS] == [theirs["bytes"][n] for n in trc.HOST_BUFS], err
            assert plan["bytes"]["tp_topics"] == 0 and plan["bytes"]["tp_scen"] == 0
            # the combined call: the *_racks call's bytes plus the two buffers of kas_solve_host_topic_impact
            for mixed in (dict(spec=_cspec(keys, k)), dict(front=_fspec(keys, k, {"max_topic_outbound": 100, "max_rack_inbound": 100}))):
                if ("front" in mixed) != ("front" in spec_kw):
                    continue
                rc, mine, err = topic_choose_host_call(fb, cells16=cells16, **mixed, **kw)
                assert rc == 0, err
                assert [mine["bytes"][n] for n in trc.HOST_BUFS] == [theirs["bytes"][n] for n in trc.HOST_BUFS], (what, mixed)
                assert mine["bytes"]["tp_topics"] == 32 * (Tn + 1) and mine["bytes"]["tp_scen"] == 64 * (S + 1)
                assert mine["rack_records"] == need and mine["head_bytes"] == 16 * (k + 1) + 4 * S + 4 * k + 4 and mine["region_ints"] == 0
                assert mine["listed"] == (k if "mv" in kw else 0) and mine["gather_rows"] == (0 if "rows_cap" in kw else 1)
        # topic criteria without a rack pass: the plain call's bytes plus the two topic buffers
        rc, mine, err = topic_choose_host_call(fb, spec=_cspec(("max_topic_inbound", "moved_replicas"), k), racks=False, cells16=cells16, **kw)
        assert rc == 0, err
        assert [mine["bytes"][n] for n in HOST_BUFS[:-2]] == got[:-2] and mine["bytes"]["rk_racks"] == 0 and mine["bytes"]["rk_scen"] == 0
        assert mine["bytes"]["tp_topics"] == 32 * (Tn + 1) and mine["bytes"]["tp_scen"] == 64 * (S + 1)
    # the topic-impact call through this driver and through the driver that was there: unchanged (tests/test_topics_cpu.py and
    # tests/test_racks_cpu.py pin the bytes)
    for n_select in (-1, 0):
        rc, mine, err = topic_choose_host_call(fb, racks=False, rack_keys=False, topic_keys=False, cells16=cells16, n_select=n_select)
        rc2, theirs, err2 = ttp.topic_host_call(fb, n_select=n_select, cells16=cells16)
        assert rc == 0 and rc2 == 0 and mine["bytes"] == theirs["bytes"], (err, err2)
        assert [mine["bytes"][n] for n in emu_lib.HOST_BUFS] == ttp.PARENT[(cells16, n_select)]
        assert mine["bytes"]["tp_topics"] == 32 * (Tn + 1) and not any(mine["bytes"][n] for n in HOST_BUFS[len(emu_lib.HOST_BUFS):n_rack])
    # a choice by topic criteria without moves and without rows: the size table without cells is the only moves buffer
    rc, plan, err = topic_choose_host_call(fb, spec=_cspec(keys, k), cells16=cells16, rows_cap=0, missing=("rows",))
    assert rc == 0 and plan["gather_rows"] == 0 and plan["bytes"]["mv_sizes0"] == 32 * (S + 1), err
    assert not any(plan["bytes"][n] for n in tm.HOST_BUFS[20:] if n != "mv_sizes0")


# ---- ABI ------------------------------------------------------------------------------------------------------------------
def test_abi_declares_the_topic_criteria_and_entries(tmp_path):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(kas_[a-z_0-9]+)\s*\(", src))
    assert len(abi.TOPIC_CHOOSE_ENTRIES) == 10
    for name in abi.TOPIC_CHOOSE_ENTRIES:
        assert name in declared and name in native.SYMBOLS, name
        assert name.replace("_topics", "_racks") in abi.RACK_CHOOSE_ENTRIES
    assert re.search(r"#define KAS_ABI_VERSION (\d+)", src).group(1) == str(abi.KAS_ABI_VERSION) == "6"
    probe = tmp_path / "probe.c"
    fields = abi.SCENARIO_TOPIC_FIELDS
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kas_abi.h"\nint main(void) {\n'
                     + "".join('  printf("%%d %%zu\\n", KAS_KEY_%s, offsetof(kas_scenario_topic_impact, %s));\n' % (f.upper(), f) for f in fields)
                     + '  printf("%d %d %d %d %d\\n", KAS_KEY_TOPIC_BASE, KAS_KEY_TOPIC_END, KAS_KEY_RACK_BASE, KAS_KEY_RACK_END, KAS_KEY_COUNT);\n'
                     + '  printf("%zu %zu %zu %zu\\n", sizeof(kas_choose_spec), sizeof(kas_front_spec), sizeof(kas_scenario_topic_impact),\n'
                     + '         offsetof(kas_scenario_topic_impact, reserved));\n'
                     + "".join("  (void)sizeof(&%s);\n" % n for n in abi.TOPIC_CHOOSE_ENTRIES)      # (declared; nothing is linked)
                     + '  return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c11", "-Werror=implicit-function-declaration", "-I" + os.path.join(ROOT, "include"), str(probe),
                           "-o", str(exe)])
    lines = subprocess.check_output([str(exe)], text=True).splitlines()
    for i, f in enumerate(fields):
        key, off = (int(v) for v in lines[i].split())
        assert key == abi.TOPIC_KEYS[f] == 48 + i and off == 4 * (key - 48) == abi.SCENARIO_TOPIC_IMPACT_DTYPE.fields[f][1], f
    assert [int(v) for v in lines[15].split()] == [abi.KAS_KEY_TOPIC_BASE, abi.KAS_KEY_TOPIC_END, abi.KAS_KEY_RACK_BASE, abi.KAS_KEY_RACK_END,
                                                   abi.KAS_KEY_COUNT] == [48, 63, 16, 33, 10]
    assert lines[16].split() == ["24", "60", "64", "60"]                    # (the specs are reused unchanged; word 15 is reserved)
    assert abi.TOPIC_KEY_NAMES == abi.SCENARIO_TOPIC_FIELDS and sorted(abi.TOPIC_KEYS.values()) == list(range(48, 63))
    assert sorted(abi.RACK_KEYS.values()) == list(range(16, 33)) and len(abi.KEYS) == 10
    assert abi.is_topic_key("topics_ok") and abi.is_topic_key(62) and not abi.is_topic_key(63) and not abi.is_topic_key("colocated_after")
    spec = abi.topic_choose_spec(("max_topic_inbound", "colocated_after", "replica_spread"), 3)
    assert (spec.n_keys, list(spec.key)[:3], spec.k) == (3, [55, 17, 6], 3)
    fs = abi.topic_front_spec(("moved_replicas", "sum_topic_leader_spread"), {"topics_departed": 0, "rack_leader_spread": 2}, 4)
    assert (fs.n_keys, list(fs.key)[:2], fs.n_limits, list(fs.limit_key)[:2], list(fs.limit)[:2], fs.k) == (2, [0, 62], 2, [51, 32], [0, 2], 4)
    for bad in (lambda: abi.topic_choose_spec(("nope",), 1), lambda: abi.topic_front_spec(("moved_replicas",), {"reserved": 1}),
                lambda: abi.rack_choose_spec(("topics_ok",), 1), lambda: abi.choose_spec(("topics_ok",), 1),
                lambda: abi.rack_front_spec(("moved_replicas",), {"topics_ok": 1})):
        with pytest.raises(ValueError):
            bad()


def test_library_exports_the_topic_choose_entries():
    from kafka_assigner_amd import build
    build.build()
    L = native.load()
    for name in abi.TOPIC_CHOOSE_ENTRIES:
        assert hasattr(L, name), name
    assert L.kas_abi_version() == 6
    blob = open(build.LIB, "rb").read()
    for kernel in (b"kas_rank_topics_kernel", b"kas_front_mark_topics_kernel", b"kas_front_rank_topics_kernel",
                   b"kas_rank_racks_kernel", b"kas_front_mark_racks_kernel", b"kas_front_rank_racks_kernel",
                   b"kas_rank_kernel", b"kas_front_mark_kernel", b"kas_front_rank_kernel", b"kas_gather_kernel"):
        assert kernel in blob, kernel


# ---- WhatIf ---------------------------------------------------------------------------------------------------------------
def _fake_host_calls(monkeypatch):
    """native.solve_host_choose_topics / solve_host_front_topics over the emulator (the oracle's solve, the checkers' impact, rack and
    topic records, and the kernels' code for the ranking, the front and the gather); every other choice entry records its name"""
    from impact_ref import impact_ref
    from oracle_lib import oracle_solve
    calls = []

    def run(fb, keys, k, within, racks, report_rack):
        ho = oracle_solve(fb)
        imp = impact_ref(fb, ho)
        S = fb.n_scenarios
        rr = srk = None
        if racks:
            rack_recs, srk, rack_off = rack_ref(fb, ho, report_rack)
            rr = native.RackReport(racks=rack_recs, scenarios=srk, rack_off=rack_off, impact=imp[1])
        tt, stp = topic_ref(fb, ho)
        got = emu_topic_choose(fb, ho.out, ho.scenario_results[:S], imp, srk, stp, keys, k, within)
        used, recs = int(got.row_off[k]), int(got.node_off[k])
        return ho, got, rr, native.TopicReport(topics=tt, scenarios=stp, impact=imp[1]), dict(
            rank=got.rank, chosen=got.chosen, row_off=got.row_off, node_off=got.node_off, n_ok=got.n_ok, rows=got.rows[:used],
            nodes=got.nodes[:recs], scenarios=imp[1])

    def choose(fb, keys, k, racks=False, report_rack=None, mask=None, rows=True, **kw):
        calls.append(("choose_topics", tuple(abi.topic_key_id(x) for x in keys), bool(racks), report_rack is not None))
        ho, got, rr, tr, fields = run(fb, list(keys), k, None, racks, report_rack)
        return ho, native.Choice(**fields), None, rr, tr

    def front(fb, spec, racks=False, report_rack=None, mask=None, rows=True, **kw):
        calls.append(("front_topics", tuple(spec.key)[:spec.n_keys], bool(racks), report_rack is not None))
        within = [(spec.limit_key[i], spec.limit[i]) for i in range(spec.n_limits)]
        ho, got, rr, tr, fields = run(fb, list(spec.key)[:spec.n_keys], spec.k, within, racks, report_rack)
        return ho, native.Front(n_eligible=int(got.counts[1]), n_front=int(got.counts[2]), **fields), None, rr, tr

    class Elsewhere(Exception):
        pass

    def other(name):
        def call(*a, **kw):
            calls.append((name,))
            raise Elsewhere(name)
        return call
    monkeypatch.setattr(native, "solve_host_choose_topics", choose)
    monkeypatch.setattr(native, "solve_host_front_topics", front)
    for name in ("solve_host_choose_racks", "solve_host_front_racks", "solve_host_choose", "solve_host_front", "solve_host_choose_moves"):
        monkeypatch.setattr(native, name, other(name))
    return calls, Elsewhere


def test_whatif_best_and_front_route_by_criterion_name_without_a_gpu(monkeypatch):
    w, vs, fb, ho, imp, srk, table, names, tt, stp = whatif_topics()
    calls, Elsewhere = _fake_host_calls(monkeypatch)
    S = fb.n_scenarios
    sr, si = ho.scenario_results[:S], imp[1][:S]
    best = w.best(vs, k=5, by=WHATIF_MAX)
    want = R.rank_ref(sr, si, srk, stp, WHATIF_MAX, 5)
    assert [r._index for r in best] == want.chosen.tolist() and [r.rank for r in best] == list(range(5)) and best[0]._index == 233
    for r in best:
        s = r._index
        assert r.max_topic_replica_spread == int(stp["max_topic_replica_spread"][s]) and r.topics_ok == 2
        assert r.colocated_after is None                                    # (no rack pass: no rack name, racks=False)
        ti = r.topic_impact()
        assert list(ti) == w.topic_names and max(v["max_inbound"] for v in ti.values()) == r.max_topic_inbound
        assert [ti[n]["max_replicas_after"] for n in w.topic_names] == tt["max_replicas_after"][2 * s:2 * s + 2].tolist()
        assert r.assignment(w.topic_names[0]) and r.broker_impact()
        with pytest.raises(ValueError):
            r.rack_impact()
    # a rack name beside a topic name: the rack pass runs too, against the real racks
    both = w.best(vs, k=3, by=("max_topic_inbound", "colocated_after", "moved_replicas"))
    assert [r._index for r in both] == R.rank_ref(sr, si, srk, stp, ("max_topic_inbound", "colocated_after", "moved_replicas"), 3).chosen.tolist()
    assert both[0].rack_impact() and both[0].topic_impact() and both[0].colocated_after == int(srk["colocated_after"][both[0]._index])
    # topics=True with broker criteria: the same order as without, and the topic figures beside it; racks=True is passed along
    plain = w.best(vs, k=3, by=("replica_spread",), topics=True)
    assert [r._index for r in plain] == R.rank_ref(sr, si, srk, stp, ("replica_spread",), 3).chosen.tolist() and plain[0].topic_impact()
    w.best(vs, k=1, by=("replica_spread",), topics=True, racks=True)
    keys, within = WHATIF_FRONT_A
    full = w.front(vs, by=keys, within=within, k=S)
    ref = R.front_of(sr, si, srk, stp, keys, S, within)
    assert full.n_front == len(full) == int(ref.counts[2]) >= 2 and full.n_eligible == 36
    assert [r._index for r in full] == ref.chosen[:len(full)].tolist() and "over_limit" in full.classes and "failed" in full.classes
    assert all(r.topics_departed == 0 and r.topic_impact() for r in full)
    bound = w.front(vs, by=("moved_replicas", "replica_spread"), within={"max_topic_inbound": 40, "max_rack_inbound": 10**6}, k=S)
    assert bound.n_eligible == 80 and all(r.max_topic_inbound <= 40 and r.rack_impact() for r in bound)
    assert calls == [("choose_topics", (57, 0), False, False), ("choose_topics", (55, 17, 0), True, True), ("choose_topics", (6,), False, False),
                     ("choose_topics", (6,), True, True), ("front_topics", (0, 57), False, False), ("front_topics", (0, 6), True, True)]
    # calls that name no topic criterion and leave topics=False go where they went
    del calls[:]
    for call in (lambda: w.best(vs, by=("colocated_after",)), lambda: w.best(vs, by=("replica_spread",), racks=True),
                 lambda: w.best(vs, by=("replica_spread",)), lambda: w.front(vs, by=("moved_replicas", "rack_leader_spread")),
                 lambda: w.front(vs), lambda: w.best(vs, moves=("replicas",))):
        with pytest.raises(Elsewhere):
            call()
    assert calls == [("solve_host_choose_racks",), ("solve_host_choose_racks",), ("solve_host_choose",), ("solve_host_front_racks",),
                     ("solve_host_front",), ("solve_host_choose_moves",)]
    for call in (lambda: w.best(vs, by=("nope",)), lambda: w.front(vs, by=("reserved",)), lambda: w.front(vs, within={"nope": 1}),
                 lambda: w.best(vs, by=("topics_ok",), rows=False)):
        with pytest.raises(ValueError) as e:
            call()
        assert "rows=False" in str(e.value) or ("sum_topic_leader_spread" in str(e.value) and "rack_leader_spread" in str(e.value)
                                                and "moved_replicas" in str(e.value))

"""The Pareto front of the scenarios (include/kas_abi.h: kas_front_spec) without a GPU.

- The mark and front rank kernels' bodies (kafka-assigner_amd/csrc/kas_front_body.h) compiled with g++ against tests/emu/kas_wave.h
  and stepped on CPU fibers (tests/emu/front_driver.cpp) over synthetic records, against the NumPy checker (tests/front_ref.py): the
  S values around the workgroup and the LDS tile, every criterion, specs of 2 to 4 criteria, antichains, chains, twins, extremes,
  failed scenarios, bounds inside and outside the spec, every k.
- The what-if batch of 302 variants through mark, front rank, gather and the moves pass, with the guards that keep it meaningful.
- Gather and moves over oracle-solved batches for every k.
- The host call planner with the front arguments: refusals, the new buffers, and the plans of the existing calls byte for byte.
- The ABI: entries declared and exported, kas_front_spec against a compiled probe, version still 6.
"""
import ctypes as C
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import test_choose_cpu as tc
import test_moves_cpu as tm
from choose_ref import assert_same_choice, criterion, offsets_ref
from front_ref import DOMINATED, NOT_OK, OVER_LIMIT, assert_same_front, cut, front_choice_ref, front_ref
from impact_batches import solved
from kafka_assigner_amd import abi, native
from kafka_assigner_amd.flatten import batch_desc
from moves_ref import moves_ref
from test_choose_cpu import MULTI_SPECS, S_VALUES, SENTINEL, k_largest, own_cur_form, synthetic, whatif_solved

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "kafka-assigner_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "kas_abi.h")
E_INVALID = abi.KAS_E_INVALID_ARG
TOP = 2**31 - 1
WHATIF_A = ("moved_replicas", "leader_spread", "replica_spread")
WHATIF_B = ("replica_spread", "leader_spread", "leaders_moved", "moved_partitions")
WHATIF_BOUND = {"max_outbound": 24}
_LIB = None


# ---- the emulator ---------------------------------------------------------------------------------------------------------
def _emu_lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    so = os.path.join(EMU, "libkas_emu_front.so")
    srcs = [os.path.join(EMU, "front_driver.cpp"), os.path.join(EMU, "emu_driver.cpp")]
    deps = srcs + [os.path.join(EMU, "kas_wave.h"), HEADER] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        tmp = so + ".tmp%d" % os.getpid()
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unused-parameter", "-Wno-unknown-pragmas",
                               "-I" + os.path.join(ROOT, "tests"), "-I" + CSRC, "-I" + os.path.join(ROOT, "include"),
                               "-o", tmp] + srcs)
        os.replace(tmp, so)
    L = C.CDLL(so)
    L.kas_emu_front_rank.restype = C.c_int
    L.kas_emu_front_rank.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(abi.FrontSpec)] + [C.c_void_p] * 8 + [C.c_uint32, C.c_char_p, C.c_int]
    L.kas_emu_front.restype = C.c_int
    L.kas_emu_front.argtypes = [C.POINTER(abi.BatchDesc), C.POINTER(abi.Tables), C.POINTER(abi.ImpactTables), C.c_int,
                                C.POINTER(abi.FrontSpec), C.POINTER(abi.Choice), C.c_void_p, C.c_uint32, C.c_char_p, C.c_int]
    L.kas_emu_front_host_call.restype = C.c_int
    L.kas_emu_front_host_call.argtypes = [C.POINTER(abi.BatchDesc), C.POINTER(C.c_int64), C.c_uint, C.c_int, C.POINTER(abi.FrontSpec),
                                          C.POINTER(abi.ChooseSpec), C.POINTER(abi.Moves), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                          C.c_char_p, C.c_int]
    L.kas_emu_front_buffers.restype = C.c_int
    L.kas_emu_front_buffers.argtypes = [C.c_int]
    _LIB = L
    return L


def _spec(keys, k, within=(), n_keys=None, n_limits=None):
    """kas_front_spec without abi.front_spec's own checks (the refusals are the library's to make)"""
    spec = abi.FrontSpec()
    ids = [abi.KEYS[x] if isinstance(x, str) else int(x) for x in keys]
    spec.n_keys = len(ids) if n_keys is None else n_keys
    for i, v in enumerate(ids[:4]):
        spec.key[i] = v
    pairs = list(within.items()) if isinstance(within, dict) else list(within)
    spec.n_limits = len(pairs) if n_limits is None else n_limits
    for i, (name, limit) in enumerate(pairs[:4]):
        spec.limit_key[i] = abi.KEYS[name] if isinstance(name, str) else int(name)
        spec.limit[i] = limit
    spec.k = k
    return spec


def emu_front_rank(sr, si, keys, k, within=(), cells=None, n_nodes=None, lds_fill=0xCDCDCDCD):
    """kas_emu_front_rank: every output pre-filled with a sentinel, one element behind every array a guard"""
    S = int(sr.shape[0])
    got = SimpleNamespace(rank=np.full(S + 1, SENTINEL, np.int32), chosen=np.full(k + 1, SENTINEL, np.int32),
                          row_off=np.full(k + 2, SENTINEL, np.int64), node_off=np.full(k + 2, SENTINEL, np.int64),
                          n_ok=np.full(2, SENTINEL, np.int32), counts=np.full(5, SENTINEL, np.int32))
    sized = cells is not None
    if sized:
        cells, n_nodes = np.ascontiguousarray(cells, np.int64), np.ascontiguousarray(n_nodes, np.int32)
    err = C.create_string_buffer(512)
    spec = _spec(keys, k, within)
    rc = _emu_lib().kas_emu_front_rank(sr.ctypes.data, si.ctypes.data, S, C.byref(spec), cells.ctypes.data if sized else None,
                                       n_nodes.ctypes.data if sized else None, got.rank.ctypes.data, got.chosen.ctypes.data,
                                       got.row_off.ctypes.data if sized else None, got.node_off.ctypes.data if sized else None,
                                       got.n_ok.ctypes.data, got.counts.ctypes.data, lds_fill, err, 512)
    assert rc == 0, (rc, err.value.decode())
    assert got.rank[S] == SENTINEL and got.chosen[k] == SENTINEL and got.n_ok[1] == SENTINEL and got.counts[4] == SENTINEL
    assert got.row_off[k + 1] == SENTINEL and got.node_off[k + 1] == SENTINEL
    got.rank, got.chosen, got.n_ok, got.counts = got.rank[:S], got.chosen[:k], int(got.n_ok[0]), got.counts[:4]
    got.row_off, got.node_off = (got.row_off[:k + 1], got.node_off[:k + 1]) if sized else (None, None)
    return got


def _check(sr, si, keys, k, what, within=(), sized=True, lds_fill=0xCDCDCDCD, base=None):
    """base: the checker's front of the same records and spec at another k (the O(S^2) pass is then not repeated)"""
    S = int(sr.shape[0])
    rng = np.random.default_rng(S + k)
    cells = rng.integers(0, 7, S) * 3 + (np.arange(S) % 5 == 0) if sized else None       # (odd sizes and zeros among them)
    n_nodes = rng.integers(0, 50, S) if sized else None
    want = front_ref(sr, si, keys, k, within) if base is None else cut(base, k)
    if sized:
        want.row_off, want.node_off = offsets_ref(want.order, cells, k), offsets_ref(want.order, n_nodes, k)
    got = emu_front_rank(sr, si, keys, k, within, cells, n_nodes, lds_fill=lds_fill)
    assert got.n_ok == want.n_ok, (what, got.n_ok, want.n_ok)
    assert_same_front(want, got, what)
    return want


def _ks(S, n_front):
    return sorted({k for k in (0, 1, n_front - 1, n_front, n_front + 1, S) if 0 <= k <= S})


def _every_k(sr, si, keys, what, within=()):
    want = front_ref(sr, si, keys, 0, within)
    for k in _ks(int(sr.shape[0]), int(want.order.size)):
        _check(sr, si, keys, k, f"{what} k={k}", within, base=want)
    return want


# ---- synthetic records ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", S_VALUES)
def test_emulated_front_every_criterion_and_small_values(S):
    """every single criterion (the front is the first of the smallest) and specs of 2 to 4 criteria with values from {0..3}: most
    keys are equal, the index decides, and the front is a handful of scenarios"""
    sr, si = synthetic(S, 1, failed="random")
    n_ok = int((sr["status"] == 0).sum())
    for keys in [(name,) for name in abi.KEY_NAMES]:
        want = _check(sr, si, keys, min(S, 2), f"S={S} {keys}")
        assert want.order.size == (1 if n_ok else 0)
    for keys in MULTI_SPECS:
        want = _every_k(sr, si, keys, f"S={S} {keys}")
        if S >= 64:
            assert 1 <= want.order.size <= 16, want.order.size
    _check(sr, si, MULTI_SPECS[0], min(S, 3), f"S={S} rank only", sized=False)


@pytest.mark.parametrize("S", S_VALUES)
def test_emulated_front_wide_values(S):
    """values from {0..63}: fronts of tens of members (measured with seed 1: 14 / 33 / 52 / 72 at S = 65 / 257 / 1025 / 2049 under four
    criteria)"""
    sr, si = synthetic(S, 1, values=64, failed="random")
    for keys in MULTI_SPECS:
        want = _every_k(sr, si, keys, f"S={S} wide {keys}")
        if S >= 65 and len(keys) == 4:
            assert want.order.size >= 10, want.order.size


@pytest.mark.parametrize("S", S_VALUES)
@pytest.mark.parametrize("failed", ["none", "alternate", "all"])
def test_emulated_front_antichain_chain_and_twins(S, failed):
    sr, si = synthetic(S, 2, failed=failed)
    ok = sr["status"] == 0
    n_ok = int(ok.sum())
    assert n_ok == {"none": S, "alternate": (S + 1) // 2, "all": 0}[failed]
    perm = np.random.default_rng(S).permutation(S).astype(np.int32)
    keys = ("moved_replicas", "moved_partitions")
    # an antichain: every eligible scenario is a member, and k cuts the front
    sr["moved_replicas"], sr["moved_partitions"] = perm, S - perm
    want = _every_k(sr, si, keys, f"S={S} antichain {failed}")
    assert want.order.size == n_ok and (want.classes[ok] == 0).all()
    # a chain: every criterion grows with the index; the front is the first eligible scenario
    sr["moved_replicas"], sr["moved_partitions"] = np.arange(S), 2 * np.arange(S)
    want = _every_k(sr, si, keys, f"S={S} chain {failed}")
    assert want.order.tolist() == (np.nonzero(ok)[0][:1]).tolist()
    if failed == "all":
        assert (want.chosen == -1).all() and (want.rank == NOT_OK).all() and want.counts.tolist() == [0, 0, 0, 0]
    # every key twice: the earlier of each pair only
    half = (S + 1) // 2
    sr["status"] = 0
    sr["moved_replicas"], sr["moved_partitions"] = np.tile(perm[:half], 2)[:S] % half, (half - np.tile(perm[:half], 2)[:S] % half)
    want = _every_k(sr, si, keys, f"S={S} twins")
    assert want.order.size == np.unique(sr["moved_replicas"]).size and (want.order < half).all()
    assert (want.classes[half:] == DOMINATED).all()


@pytest.mark.parametrize("S", [2, 257, 1025])
def test_emulated_front_extreme_values_and_equal_keys(S):
    sr, si = synthetic(S, 4, values=[0, TOP], failed="alternate")
    for keys in [(name,) for name in abi.KEY_NAMES] + MULTI_SPECS:
        assert set(np.unique(criterion(sr, si, keys[0]))) <= {0, TOP}
        _check(sr, si, keys, S, f"S={S} extremes {keys}")
    for failed in ("none", "alternate"):                                    # all keys equal: the first OK scenario alone
        sr, si = synthetic(S, 3, values=[5], failed=failed)
        want = _check(sr, si, MULTI_SPECS[2], S, f"S={S} equal keys")
        assert want.order.tolist() == [0] and want.counts[2] == 1
    sr, si = synthetic(S, 5, values=[TOP], failed="random")
    _check(sr, si, MULTI_SPECS[2], S, f"S={S} every criterion 2^31 - 1", within={"max_inbound": TOP})


@pytest.mark.parametrize("fill", [0, 0xFFFFFFFF, 0x00000001, 0xCDCDCDCD])
def test_emulated_front_whatever_the_lds_holds(fill):
    """LDS is uninitialised on hardware: zeros (the smallest criteria, flags clear), all ones, flags set everywhere"""
    for S in (65, 1025, 1500):
        sr, si = synthetic(S, 6, values=64, failed="random")
        _check(sr, si, MULTI_SPECS[1], S // 2, f"S={S} lds {fill:#x}", within={"max_outbound": 40}, lds_fill=fill)


@pytest.mark.parametrize("S", [1, 65, 257, 1025, 2049])
def test_emulated_front_bounds(S):
    """0 to 4 bounds on criteria inside and outside the spec, a bound nobody meets, limit 2^31 - 1"""
    sr, si = synthetic(S, 7, values=64, failed="random")
    keys = ("max_inbound", "moved_replicas")
    free = front_ref(sr, si, keys, 0)
    cases = [{}, {"max_inbound": 30}, {"max_outbound": 20}, {"max_outbound": 20, "moved_replicas": 40},
             {"max_outbound": 30, "leaders_moved": 30, "moved_partitions": 30, "max_inbound": 50},
             {"leader_spread": TOP}, {"max_outbound": TOP, "max_inbound": TOP}]
    for within in cases:
        want = _every_k(sr, si, keys, f"S={S} within {within}", within)
        if S >= 257 and within == {"max_inbound": 30}:                      # inside the spec: the bound only filters the front
            assert set(want.order) <= set(free.order) and (want.classes == OVER_LIMIT).any()
        if S >= 257 and within == {"max_outbound": 20}:                     # outside: it creates members
            assert not set(want.order) <= set(free.order)
        if TOP in within.values():
            assert np.array_equal(want.rank, free.rank)
    # a bound nobody meets: nobody is eligible, the front is empty
    sr["moved_partitions"] += 1
    want = _check(sr, si, keys, min(S, 3), f"S={S} nobody", within={"moved_partitions": 0})
    assert want.counts[1] == 0 and want.counts[2] == 0 and (want.chosen == -1).all() and (want.row_off == 0).all()
    assert set(np.unique(want.rank)) <= {NOT_OK, OVER_LIMIT}


def test_emulated_front_refuses_bad_specs_in_order():
    sr, si = synthetic(8, 7)
    L = _emu_lib()
    out = np.zeros(16, np.int32)
    good = ("moved_replicas",)
    cases = [(_spec((10,), -1, [(10, -1)], n_keys=0, n_limits=5), "n_keys outside 1..4"),
             (_spec(good, 1, n_keys=5), "n_keys outside 1..4"),
             (_spec((10,), -1, [(10, -1)], n_limits=5), "unknown criterion"),
             (_spec((0, -1), 1), "unknown criterion"),
             (_spec(good, -1, [(10, -1)], n_limits=5), "n_limits outside 0..4"),
             (_spec(good, 1, n_limits=-1), "n_limits outside 0..4"),
             (_spec(good, -1, [(0, -1), (10, -1)]), "unknown limit criterion"),
             (_spec(good, 1, [(-1, 3)]), "unknown limit criterion"),
             (_spec(good, -1, [(0, 3), (1, -1)]), "negative limit"),
             (_spec(good, -1, [(0, 3)]), "k outside"),
             (_spec(good, 9), "k outside")]
    for spec, text in cases:
        err = C.create_string_buffer(256)
        rc = L.kas_emu_front_rank(sr.ctypes.data, si.ctypes.data, 8, C.byref(spec), None, None, out.ctypes.data, out.ctypes.data, None, None,
                                  out.ctypes.data, out.ctypes.data, 0, err, 256)
        assert rc == E_INVALID and text in err.value.decode(), (rc, err.value.decode(), text)


# ---- mark, front rank and gather over solved batches ------------------------------------------------------------------------
GUARD_CELLS, GUARD_NODES = 64, 3


def emu_front(fb, out, sr, imp, keys, k, within=(), mode=0, lds_fill=0xCDCDCDCD):
    """kas_emu_front over the tables of a solve (`out`: the out pool, every row in place; mode 0 int32 cells, 1 uint16 cells, 2 int32
    cells gathered into uint16 rows) and its impact records: capacities exactly the k largest scenarios', guards behind them"""
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
    spec = _spec(keys, k, within)
    rc = _emu_lib().kas_emu_front(C.byref(bd), C.byref(t), C.byref(itab), mode, C.byref(spec), C.byref(ch), got.counts.ctypes.data,
                                  lds_fill, err, 512)
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


def _same(want, got, what):
    assert_same_front(want, got, what)
    assert_same_choice(want, got, what)


def _moves_of(fb, cur, ho, chosen, mask, mode, what):
    """the moves pass (tests/emu/moves_driver.cpp) over the front's chosen[], -1 tail and all, against the checker's list"""
    tm.check(fb, cur, ho, [int(s) for s in chosen], mask, mode, what)


@pytest.mark.parametrize("name", ["mixed42", "degenerate", "widths_4_5"])
def test_emulated_front_gather_and_moves_for_every_k(name):
    fb, ho, imp = solved(name)
    S = fb.n_scenarios
    forms = tc._forms(fb, ho)
    for k in range(0, S + 1):
        for keys in (("moved_replicas", "max_inbound"), ("leaders_moved", "replica_spread", "moved_partitions")) if k in (1, S) else (("max_inbound", "moved_replicas"),):
            for mode, out, ref_out in forms:
                want = front_choice_ref(fb, ho.scenario_results, ref_out, imp, keys, k)
                got = emu_front(fb, out, ho.scenario_results[:S], imp, keys, k, mode=mode)
                _same(want, got, f"{name} mode {mode} k {k} {keys}")
            for mode in (0, 1) if k else ():
                mfb, cur, mho = tm.forms(name)[mode]
                _moves_of(mfb, cur, mho, want.chosen, 7 if k % 2 else 1, mode, f"{name} moves mode {mode} k {k}")


def test_emulated_front_of_the_whatif_batch():
    _, _, fb, ho, imp = whatif_solved()
    S = fb.n_scenarios
    sr, si = ho.scenario_results[:S], imp[1][:S]
    a = front_ref(sr, si, WHATIF_A, 0)
    ab = front_ref(sr, si, WHATIF_A, 0, WHATIF_BOUND)
    b = front_ref(sr, si, WHATIF_B, 0)
    bb = front_ref(sr, si, WHATIF_B, 0, WHATIF_BOUND)
    # the oracle's fronts, and the guards that keep the batch meaningful
    assert a.order.size == 6 and sorted(a.order.tolist()) == [0, 46, 47, 83, 175, 210] and a.classes[1] == DOMINATED
    assert ab.counts.tolist()[1:3] == [128, 8] and int((ab.classes == OVER_LIMIT).sum()) == 56
    assert sorted(set(ab.order.tolist()) - set(a.order.tolist())) == [135, 184, 208, 211] and (a.classes[[135, 184, 208, 211]] == DOMINATED).all()
    assert b.order.size == 14 and bb.order.size == 16
    assert a.order.size >= 5 and int((a.classes == DOMINATED).sum()) >= 100 and int((a.classes == NOT_OK).sum()) >= 50
    assert set(a.order.tolist()) - set(ab.order.tolist()) and set(ab.order.tolist()) - set(a.order.tolist())   # the bound removes and creates
    fb16 = own_cur_form(fb)                                                 # (16-bit cells are indices into a variant's own broker set)
    forms = tc._forms(fb16, ho)
    for keys, within, n_front in ((WHATIF_A, (), 6), (WHATIF_A, WHATIF_BOUND, 8), (WHATIF_B, (), 14), (WHATIF_B, WHATIF_BOUND, 16)):
        for k in (1, n_front, n_front + 1, S) if keys == WHATIF_A else (n_front,):
            for mode, out, ref_out in forms if k == n_front else forms[:1]:
                want = front_choice_ref(fb16 if mode else fb, sr, ref_out, imp, keys, k, within)
                got = emu_front(fb16 if mode else fb, out, sr, imp, keys, k, within, mode=mode)
                _same(want, got, f"what-if {keys} {within} k {k} mode {mode}")
                assert want.counts[2] == n_front
        # the moves of the members, in member order
        want = front_ref(sr, si, keys, n_front + 1, within)
        assert want.chosen[-1] == -1
        _moves_of(fb, fb.cur, ho, want.chosen, 7, 0, f"what-if moves {keys} {within}")


# ---- the planner ----------------------------------------------------------------------------------------------------------
HOST_BUFS = tm.HOST_BUFS + ("fr_cls", "fr_counts", "fr_counts_pin")
MISSING = dict(tc.MISSING, counts=32768)
HEAD = ("rows_need", "nodes_need", "chunks", "head_bytes", "gather_rows", "K", "native16", "listed")
_BUF = np.zeros(16, np.int64)


def front_host_call(fb, front=None, spec=None, mv=None, rows_cap=None, nodes_cap=None, missing=(), cells16=False):
    """kas_plan_host_call for a kas_solve_host_front call (front) or a choose / choose_moves call (spec): (rc, plan or None, text)"""
    L = _emu_lib()
    assert L.kas_emu_front_buffers(0) == len(HOST_BUFS) and L.kas_emu_front_buffers(1) == len(tm.HOST_BUFS)
    bd = batch_desc(fb)
    if cells16:
        bd.node_id = None
    need = k_largest(fb, (front or spec).k)
    lens = (C.c_int64 * 5)(int(fb.cur.shape[0]), int(fb.aux.shape[0]), int(fb.ctx.shape[0]), need[0] if rows_cap is None else rows_cap,
                           need[1] if nodes_cap is None else nodes_cap)
    head, nbytes = (C.c_int64 * 8)(), (C.c_int64 * len(HOST_BUFS))()
    err = C.create_string_buffer(512)
    rc = L.kas_emu_front_host_call(C.byref(bd), lens, sum(MISSING[m] for m in missing), int(cells16), None if front is None else C.byref(front),
                                   None if spec is None else C.byref(spec), None if mv is None else C.byref(mv), head, nbytes, err, 512)
    if rc != 0:
        return rc, None, err.value.decode()
    plan = dict(zip(HEAD, [int(v) for v in head]))
    plan["bytes"] = dict(zip(HOST_BUFS, [int(v) for v in nbytes]))
    return rc, plan, ""


def _mv(mask=7, moves_cap=10**6, cells_cap=10**7):
    b = _BUF.ctypes.data
    return abi.Moves(mask, 0, b, b, b, moves_cap, b, cells_cap)


def test_planner_refuses_in_order_each_with_its_text():
    fb, _, _ = solved("mixed42")
    S = fb.n_scenarios
    good = ("moved_replicas", "leaders_moved")
    rows, nodes = k_largest(fb, 2)
    bad_mv = abi.Moves(9, 0, None, None, None, -1, None, -1)
    every = dict(rows_cap=0, nodes_cap=0, missing=("rank", "counts"), mv=bad_mv)
    order = [(dict(front=_spec((10,), -1, [(10, -1)], n_keys=0, n_limits=5), **every), "n_keys outside 1..4"),
             (dict(front=_spec((10,), -1, [(10, -1)], n_limits=5), **every), "unknown criterion"),
             (dict(front=_spec(good, -1, [(10, -1)], n_limits=5), **every), "n_limits outside 0..4"),
             (dict(front=_spec(good, -1, [(10, -1)]), **every), "unknown limit criterion"),
             (dict(front=_spec(good, -1, [(0, -1)]), **every), "negative limit"),
             (dict(front=_spec(good, -1, [(0, 1)]), **every), "k outside"),
             (dict(front=_spec(good, S + 1, [(0, 1)]), **every), "k outside"),
             (dict(front=_spec(good, 2), rows_cap=rows - 1, nodes_cap=0, missing=("rank", "counts"), mv=bad_mv), "rows_cap below"),
             (dict(front=_spec(good, 2), nodes_cap=nodes - 1, missing=("rank", "counts"), mv=bad_mv), "nodes_cap below"),
             (dict(front=_spec(good, 2), missing=("counts",), mv=bad_mv), "an array the call writes is NULL"),
             (dict(front=_spec(good, 2), mv=bad_mv), "mask outside 1..7")]
    order += [(dict(front=_spec(good, 2), missing=(m,)), "an array the call writes is NULL") for m in ("rank", "chosen", "row_off", "node_off", "n_ok", "nodes", "counts")]
    for kw, text in order:
        rc, _, err = front_host_call(fb, **kw)
        assert rc == E_INVALID and text in err, (text, rc, err)
    assert "kas_front_spec" in front_host_call(fb, front=_spec(good, -1))[2]
    # rows == NULL with rows_cap == 0 gathers no rows, with moves or without; NULL with a capacity is refused
    for mv in (None, _mv()):
        rc, plan, err = front_host_call(fb, front=_spec(good, 2), rows_cap=0, missing=("rows",), mv=mv)
        assert rc == 0 and plan["gather_rows"] == 0 and plan["rows_need"] == 0 and plan["bytes"]["mv_sizes0"] == 32 * (S + 1), err
        assert front_host_call(fb, front=_spec(good, 2), missing=("rows",), mv=mv)[0] == E_INVALID
    # k = 0 classifies only
    rc, plan, err = front_host_call(fb, front=_spec(good, 0, {"max_inbound": 5}), missing=("chosen", "rows", "nodes"))
    assert rc == 0 and plan["rows_need"] == 0 and plan["nodes_need"] == 0, err


# what the parent of this change planned for mixed42, k = 3 by (moved_replicas, leaders_moved): bytes of every buffer in
# tm.HOST_BUFS order, for kas_solve_host_choose, kas_solve_host_choose_moves with rows and without, int32 cells and 16-bit cells
PARENT = {
    ("choose", False): [39028, 48644, 23936, 32, 0, 0, 208, 224, 208, 224, 6400, 224, 224, 416, 104, 32996, 3488, 104, 32996, 3488],
    ("choose_moves", False): [39028, 48644, 23936, 32, 0, 0, 208, 224, 208, 224, 6400, 224, 224, 416, 104, 32996, 3488, 104, 32996, 3488,
                              224, 728, 0, 160, 64, 43968, 32996, 0, 64],
    ("choose_moves_norows", False): [39028, 48644, 23936, 32, 0, 0, 208, 224, 208, 224, 6400, 224, 224, 416, 104, 32, 3488, 104, 32, 3488,
                                     224, 728, 0, 160, 64, 43968, 32996, 224, 64],
    ("choose", True): [0, 0, 23936, 32, 19514, 24322, 208, 224, 208, 224, 6400, 224, 224, 416, 104, 16498, 3488, 104, 16498, 3488],
    ("choose_moves", True): [0, 0, 23936, 32, 19514, 24322, 208, 224, 208, 224, 6400, 224, 224, 416, 104, 16498, 3488, 104, 16498, 3488,
                             224, 728, 0, 160, 64, 43968, 16498, 0, 64],
    ("choose_moves_norows", True): [0, 0, 23936, 32, 19514, 24322, 208, 224, 208, 224, 6400, 224, 224, 416, 104, 16, 3488, 104, 16, 3488,
                                    224, 728, 0, 160, 64, 43968, 16498, 224, 64],
}


@pytest.mark.parametrize("cells16", [False, True], ids=["int32", "cells16"])
def test_planner_buffers_of_a_front_and_of_the_calls_that_were_there(cells16):
    fb, _, _ = solved("mixed42")
    S, k = fb.n_scenarios, 3
    keys = ("moved_replicas", "leaders_moved")
    cs = abi.choose_spec(keys, k)
    n_all = len(tm.HOST_BUFS)
    # the existing calls: byte for byte what the parent planned, and none of the new buffers
    for what, kw in (("choose", {}), ("choose_moves", dict(mv=_mv())), ("choose_moves_norows", dict(mv=_mv(), rows_cap=0, missing=("rows",)))):
        rc, plan, err = front_host_call(fb, spec=cs, cells16=cells16, **kw)
        assert rc == 0, err
        got = [plan["bytes"][n] for n in HOST_BUFS]
        want = PARENT[(what, cells16)]
        assert got[:len(want)] == want and not any(got[len(want):]), (what, got)
        assert plan["head_bytes"] == 16 * (k + 1) + 4 * S + 4 * k + 4
    # the same through the drivers that were there
    rc, theirs, _ = tc.choose_host_call(fb, cs, cells16=cells16)
    assert rc == 0 and [theirs["bytes"][n] for n in tc.HOST_BUFS] == PARENT[("choose", cells16)]
    rc, theirs, _ = tm.moves_host_call(fb, spec=cs, rows_cap=k_largest(fb, k)[0], cells16=cells16)
    assert rc == 0 and [theirs["bytes"][n] for n in tm.HOST_BUFS] == PARENT[("choose_moves", cells16)]
    # a front: the matching choice's buffers, and its own three behind them
    for what, kw in (("choose", {}), ("choose_moves", dict(mv=_mv())), ("choose_moves_norows", dict(mv=_mv(), rows_cap=0, missing=("rows",)))):
        rc, plan, err = front_host_call(fb, front=_spec(keys, k, {"max_inbound": 100}), cells16=cells16, **kw)
        assert rc == 0, err
        got = [plan["bytes"][n] for n in HOST_BUFS]
        want = PARENT[(what, cells16)]
        assert got[:len(want)] == want and not any(got[len(want):n_all]), (what, got)
        assert got[n_all:] == [4 * (S + 1), 16, 16]
        assert plan["head_bytes"] == 16 * (k + 1) + 4 * S + 4 * k + 4 and plan["listed"] == (k if "mv" in kw else 0)
    # a front without moves and without rows: the size table without cells is the only moves buffer
    rc, plan, err = front_host_call(fb, front=_spec(keys, k), cells16=cells16, rows_cap=0, missing=("rows",))
    assert rc == 0 and plan["bytes"]["mv_sizes0"] == 32 * (S + 1), err
    assert not any(plan["bytes"][n] for n in tm.HOST_BUFS[20:] if n != "mv_sizes0")


# ---- ABI ------------------------------------------------------------------------------------------------------------------
def test_abi_declares_the_front_entries_and_layout(tmp_path):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(kas_[a-z_0-9]+)\s*\(", src))
    assert len(abi.FRONT_ENTRIES) == 5
    for name in abi.FRONT_ENTRIES:
        assert name in declared and name in native.SYMBOLS, name
    assert re.search(r"#define KAS_ABI_VERSION (\d+)", src).group(1) == str(abi.KAS_ABI_VERSION) == "6"
    fields = ["n_keys", "key", "n_limits", "limit_key", "limit", "k"]
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kas_abi.h"\nint main(void) {\n'
                     '  printf("%zu\\n", sizeof(kas_front_spec));\n'
                     + "".join('  printf("%%zu\\n", offsetof(kas_front_spec, %s));\n' % f for f in fields)
                     + '  printf("%d %d %d\\n", KAS_FRONT_NOT_OK, KAS_FRONT_OVER_LIMIT, KAS_FRONT_DOMINATED);\n  return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c11", "-I" + os.path.join(ROOT, "include"), str(probe), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)], text=True).splitlines()
    assert int(lines[0]) == C.sizeof(abi.FrontSpec) == 60
    assert [int(v) for v in lines[1:7]] == [getattr(abi.FrontSpec, f).offset for f in fields]
    assert [int(v) for v in lines[7].split()] == [abi.KAS_FRONT_NOT_OK, abi.KAS_FRONT_OVER_LIMIT, abi.KAS_FRONT_DOMINATED] == [-1, -2, -3]
    spec = abi.front_spec(("moved_replicas", "replica_spread"), {"max_inbound": 200}, 16)
    assert (spec.n_keys, list(spec.key)[:2], spec.n_limits, spec.limit_key[0], spec.limit[0], spec.k) == (2, [0, 6], 1, 4, 200, 16)
    with pytest.raises(ValueError):
        abi.front_spec(("moved_replicas", "no_such_criterion"))
    with pytest.raises(ValueError):
        abi.front_spec(("moved_replicas",), {"no_such_criterion": 1})


def test_library_exports_the_front_entries():
    from kafka_assigner_amd import build
    build.build()
    L = native.load()
    for name in abi.FRONT_ENTRIES:
        assert hasattr(L, name), name
    assert L.kas_abi_version() == 6
    blob = open(build.LIB, "rb").read()
    assert b"kas_front_mark_kernel" in blob and b"kas_front_rank_kernel" in blob
    assert b"kas_rank_kernel" in blob and b"kas_gather_kernel" in blob


def test_whatif_front_without_a_gpu(monkeypatch):
    """WhatIf.front over a stand-in for the library's host call (the checker over the oracle's solve): members, order, classes, the
    counts, k smaller than the front, and the refusals of its own"""
    from oracle_lib import oracle_solve
    from impact_ref import impact_ref
    w, vs = tc.whatif_variants()
    vs = vs[:60]

    def fake(fb, spec, mask=None, rows=True, **kw):
        ho = oracle_solve(fb)
        imp = impact_ref(fb, ho)
        keys, k = list(spec.key)[:spec.n_keys], spec.k
        within = [(spec.limit_key[i], spec.limit[i]) for i in range(spec.n_limits)]
        r = front_choice_ref(fb, ho.scenario_results, ho.out, imp, keys, k, within)
        c = native.Front(rank=r.rank, chosen=r.chosen, row_off=r.row_off, node_off=r.node_off, n_ok=r.n_ok, rows=r.rows, nodes=r.nodes,
                         scenarios=imp[1], n_eligible=int(r.counts[1]), n_front=int(r.counts[2]))
        return ho, c, None
    monkeypatch.setattr(native, "solve_host_front", fake)
    by = ("moved_replicas", "leader_spread", "replica_spread")
    full = w.front(vs, by=by, k=60)
    assert full.n_front == len(full) >= 3 and [r.rank for r in full] == list(range(len(full)))
    assert full.classes.count("member") == full.n_front and full.classes[1] == "dominated" and "failed" in full.classes
    cut = w.front(vs, by=by, k=2)
    assert len(cut) == 2 and cut.n_front == full.n_front and [r._index for r in cut] == [r._index for r in full[:2]]
    bound = w.front(vs, by=by, within={"max_outbound": 24}, k=60)
    assert "over_limit" in bound.classes and bound.n_eligible < bound.n_ok
    assert full[0].assignment(w.topic_names[0]) and full[0].broker_impact()
    for kw in (dict(by=("nope",)), dict(by=()), dict(within={"nope": 1}), dict(within={"max_inbound": -1})):
        with pytest.raises(ValueError):
            w.front(vs, **kw)

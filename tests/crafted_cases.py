"""Crafted move lists for the batches pass and the rounds pass: out tables written by hand, so that a move lies at a chosen place
of the kernels' queue -- a group of KAS_BATCH_GROUP moves and its replay, the queue's remainder behind a tile, a cap exceeded by a
lane of wavefront 1, 2 or 3, more rounds than KAS_ROUND_WINDOW, a round word whose `used` bits are all ones, a scenario at the
node limit.  Shared by the emulator (tests/test_batches_cpu.py, tests/test_rounds_cpu.py) and the MI355X
(tests/test_batches_crafted_gpu.py, tests/test_rounds_crafted_gpu.py), which run every case on int32 cells and, where the form
exists, on 16-bit cells.  Test infrastructure.

A case is (fb, ho, the caps to run, what the checker must show for it): Case.show(i, want) holds the checker's result under
caps[i] (tests/batches_ref.py, tests/rounds_ref.py: the header's loops in plain Python) to what the case claims to reach, so a
case that stops reaching its path fails whoever runs it.  The tables come from crafted() / random_moves() / swap_in() of
tests/test_batches_cpu.py.
"""
from __future__ import annotations

from copy import copy
from dataclasses import dataclass, field
from functools import lru_cache
from types import SimpleNamespace
from typing import Callable

import numpy as np

import batches_ref as B
import rounds_ref as R
from kafka_assigner_amd import abi
from kafka_assigner_amd.flatten import to_cells16

BIG = 10 ** 6
ALL_BIG = {"inbound": BIG, "outbound": BIG, "max_moves": BIG}
GROUP, WINDOW = B.GROUP, R.WINDOW


def _tb():
    import test_batches_cpu as tb                           # (it imports this module for its case names)
    return tb


def cells16_form(fb, ho):
    """(ho with the out pool as uint16 node indices, cur16) of a crafted (fb, ho): -1 becomes KAS_CELL16_NONE.  An out list that
    names an id outside the broker set has no exact 16-bit form -- the id would become the pad and end the list there -- and
    raises ValueError: such a case runs on int32 cells only."""
    out16 = np.full(ho.out.shape, abi.KAS_CELL16_NONE, np.uint16)
    for s in range(fb.n_scenarios):
        n, off = int(fb.scen["n_nodes"][s]), int(fb.scen["node_off"][s])
        ids = fb.node_id[off:off + n].astype(np.int64)
        b, c = int(fb.scen["topic_begin"][s]), int(fb.scen["topic_count"][s])
        for t in range(b, b + c):
            td = fb.topics[t]
            oo, cells = int(td["out_off"]), int(td["n_partitions"]) * int(td["out_width"])
            v = ho.out[oo:oo + cells].astype(np.int64)
            pos = np.minimum(np.searchsorted(ids, v), max(n - 1, 0))
            hit = (ids[pos] == v) if n else np.zeros(cells, bool)
            if not (hit | (v == -1)).all():
                raise ValueError("an out list names an id outside the broker set: the case has no 16-bit form")
            out16[oo:oo + cells] = np.where(hit, pos, abi.KAS_CELL16_NONE).astype(np.uint16)
    ho16 = copy(ho)
    ho16.out = out16
    return ho16, to_cells16(fb)


@dataclass
class Case:
    kind: str                               # "batches" / "rounds"
    fb: object
    ho: object
    caps: tuple                             # the caps to run, one call each
    show: Callable                          # show(i, want): what the checker's result under caps[i] must show
    select: tuple = (0,)                    # the listed scenarios
    strides: tuple = (None,)                # rounds: (round_stride, move_stride) per call under every cap; None: room for everything;
                                            # a callable: of the checker's result
    _cache: dict = field(default_factory=dict)

    def tables(self, cells16: bool):
        """(fb, ho, cur16) for a cell type; ValueError where the case has no 16-bit form"""
        if not cells16:
            return self.fb, self.ho, None
        if "form16" not in self._cache:
            self._cache["form16"] = cells16_form(self.fb, self.ho)
        ho16, cur16 = self._cache["form16"]
        return self.fb, ho16, cur16

    def wants(self, cells16: bool):
        """the checker's result for scenario 0 under each of caps, computed once and left as it is"""
        if ("wants", cells16) not in self._cache:
            fb, ho, cur16 = self.tables(cells16)
            mv = B.scenario_moves(fb, ho, 0, cells16, cur16)
            out = []
            for caps in self.caps:
                if self.kind == "batches":
                    rec, bt = B.cut(mv, caps)
                    out.append(SimpleNamespace(record=rec, batches=bt, moves=mv))
                else:
                    ro, by_in, by_out = R.monotone(mv, caps)
                    rec, rd = R.records(mv, ro, by_in, by_out)
                    out.append(SimpleNamespace(record=rec, rounds=rd, round_of=ro, moves=mv))
            for i, w in enumerate(out):
                self.show(i, w)
            self._cache["wants", cells16] = out
        return self._cache["wants", cells16]

    def listed(self, want):
        """the checker's list for `select`: one scenario, so its result or None for an empty slot"""
        return [want if s == 0 else None for s in self.select]

    def strides_for(self, want):
        """[(round_stride, move_stride)] of a rounds case under the caps `want` is the result of"""
        out = []
        for st in self.strides:
            if st is None:
                st = (want.record["n_rounds"] + 2, want.record["n_moves"] + 3)
            elif callable(st):
                st = st(want)
            out.append(st)
        return out


def _closes(w):
    return [(b["first_move"], b["n_moves"], b["closed_by"]) for b in w.batches]


# ---- tables both passes run --------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _three_tiles(W):
    """2,600 rows with 1,500 moves W wide, then 300 rows with 120 moves 3 wide, on 24 brokers: three tiles and a second, narrower
    topic (cw < W); after the first tile the batches pass's queue keeps a remainder and the next tile's moves go behind it"""
    tb = _tb()
    fb, ho = tb.crafted([(2600, tb.random_moves(2600, 1500, 24, 24, 11, width=W, most=W), W), (300, tb.random_moves(300, 120, 24, 24, 12, most=3), 3)], N=24)
    assert [int(x) for x in fb.topics["cur_width"]] == [W, 3]
    return fb, ho


@lru_cache(maxsize=None)
def _node_limit(N, sparse, W=8):
    """N nodes, one topic of 1,300 rows W wide; the rows p with p mod 24 < 11 move: each brings one of the nodes 0, 1, 63, 64, 65,
    N-65, N-64, N-2, N-1 in place of its last replica.  sparse: ids 7 + 3 i, a range above 2 x n_cap: the sorted-id lookup; else
    ids 0..N-1: the direct table."""
    tb = _tb()
    special = (0, 1, 63, 64, 65, N - 65, N - 64, N - 2, N - 1)
    rows = [p for p in range(1300) if p % 24 < 11]
    moved = {p: [(p + i) % N for i in range(W - 1)] + [special[k % 9]] for k, p in enumerate(rows)}
    fb, ho = tb.crafted([(1300, moved)], N=N, width=W, ids=[7 + 3 * i for i in range(N)] if sparse else None)
    span = int(fb.node_id[N - 1]) - int(fb.node_id[0]) + 1
    assert int(fb.scen["n_nodes"][0]) == N and (span > 2 * N if sparse else span == N)       # which lookup the kernels stage
    assert int(fb.topics["cur_width"][0]) == int(fb.topics["out_width"][0]) == W
    return fb, ho, len(rows), special


def _show_node_limit(w, n_moves, special, N):
    assert len(w.moves) == n_moves >= 590
    brought = {b for m in w.moves for b in m[2]}
    assert brought == set(special) and N - 1 in brought and all(len(m[3]) == 1 for m in w.moves)


# ---- the batches pass ----------------------------------------------------------------------------------------------------------
def _b_group(n_moves, W):
    tb = _tb()
    fb, ho = tb.crafted([(700, tb.random_moves(700, n_moves, 12, 12, n_moves, width=W, most=W))], width=W)
    caps = (ALL_BIG, {"inbound": 8}, {"inbound": 1}, {"max_moves": GROUP})

    def show(i, w):
        assert len(w.moves) == n_moves
        r = B.replay(w.moves, caps[i])
        if i == 0:
            assert r.replayed == 0 and r.clean == -(-n_moves // GROUP)          # the clean path, every group
        if i == 2:
            assert r.replayed >= max(n_moves // GROUP, 1) and r.most_closes >= 4   # the replay of every group of some size
        if i == 3:
            assert r.replayed == (1 if n_moves > GROUP else 0)                  # max_moves reached by exactly one group
    return Case("batches", fb, ho, caps, show)


def _b_three_tiles(W):
    fb, ho = _three_tiles(W)
    caps = ({"inbound": 1}, {"inbound": 3, "outbound": 2, "max_moves": 50}, {"outbound": 1}, ALL_BIG)

    def show(i, w):
        assert len(w.moves) == 1620
        r = B.replay(w.moves, caps[i])
        assert (r.clean, r.replayed) == ((7, 0) if i == 3 else (0, 7))
    return Case("batches", fb, ho, caps, show)


def _b_tile_edges(W):
    """rows 1,023, 1,024 and 1,025 of a topic move (both sides of a tile), a batch spans the topic's end into the next, narrower
    topic, and a row that comes out empty is no move"""
    tb = _tb()
    moved = {p: tb.swap_in(p, (p + W + 2) % 12, width=W) for p in (3, 1022, 1023, 1024, 1025)}
    moved[7] = []
    fb, ho = tb.crafted([(1026, moved, W), (40, {0: tb.swap_in(0, 7), 39: tb.swap_in(39, 9)}, 3)])
    caps = ({"max_moves": 4}, {"inbound": 1})

    def show(i, w):
        assert [(t, p) for t, p, _, _ in w.moves] == [(0, 3), (0, 1022), (0, 1023), (0, 1024), (0, 1025), (1, 0), (1, 39)]
        assert all(len(m[2]) == 1 and len(m[3]) == 1 for m in w.moves)
        if i == 0:
            assert [(b["first_move"], b["n_moves"], b["topic"], b["partition"]) for b in w.batches] == [(0, 4, 0, 3), (4, 3, 0, 1025)]
    return Case("batches", fb, ho, caps, show)


def _b_exceed(rows11):
    """256 rows, all moves, on 11 current brokers plus node 11 under cap_inbound 2: the three rows of `rows11` bring node 11,
    every other row gains an id outside the set, so node 11 is the only receiver and the lanes of those three rows are the only
    ones that can see a counter above its cap.  Int32 cells only."""
    tb = _tb()
    a, b, c = rows11
    moved = {p: [p % 11, (p + 1) % 11, 11 if p in rows11 else 200] for p in range(256)}
    fb, ho = tb.crafted([(256, moved)], N=12, n_cur=11)
    caps = ({"inbound": 2},)

    def show(i, w):
        assert len(w.moves) == GROUP and [k for k, m in enumerate(w.moves) if m[2]] == [a, b, c]
        assert _closes(w) == [(0, c, B.INBOUND), (c, GROUP - c, B.END)]
        r = B.replay(w.moves, caps[0])
        assert (r.clean, r.replayed) == (0, 1)
    return Case("batches", fb, ho, caps, show)


def _b_cap_reached_in_group():
    """256 moves, one group: moves 100 and 255 (the group's last) bring node 11 under cap_inbound 2, every other move gains an id
    outside the set: the cap is reached and never exceeded, one batch, and the group is in as a whole.  Int32 cells only."""
    tb = _tb()
    moved = {p: [p % 11, (p + 1) % 11, 11 if p in (100, 255) else 200] for p in range(256)}
    fb, ho = tb.crafted([(256, moved)], N=12, n_cur=11)
    caps = ({"inbound": 2},)

    def show(i, w):
        assert len(w.moves) == GROUP and [k for k, m in enumerate(w.moves) if m[2]] == [100, 255]
        assert [(b["first_move"], b["n_moves"], b["max_inbound"], b["closed_by"]) for b in w.batches] == [(0, GROUP, 2, B.END)]
        r = B.replay(w.moves, caps[0])
        assert (r.clean, r.replayed) == (1, 0)
    return Case("batches", fb, ho, caps, show)


def _b_cap_at_group_end():
    """node 11 is taken by moves 100 and 255 (the group's last): cap 2 is reached and the group is clean; move 256 takes it again
    and closes.  Int32 cells only."""
    tb = _tb()
    rows = list(range(0, 600, 2))
    moved = {p: [p % 11, (p + 1) % 11, 11] if i in (100, 255, 256) else [p % 11, (p + 1) % 11, (p + 2) % 11 + 100] for i, p in enumerate(rows)}
    fb, ho = tb.crafted([(600, moved)], N=12, n_cur=11)
    caps = ({"inbound": 2},)

    def show(i, w):
        assert len(w.moves) == 300 and [k for k, m in enumerate(w.moves) if m[2]] == [100, 255, 256]
        assert [(b["first_move"], b["n_moves"], b["max_inbound"], b["closed_by"]) for b in w.batches] == [(0, 256, 2, B.INBOUND), (256, 44, 1, B.END)]
        r = B.replay(w.moves, caps[0])
        assert (r.clean, r.replayed) == (1, 1)
    return Case("batches", fb, ho, caps, show)


def _b_many_closes(W):
    """cap 1 on 12 brokers: a group of 256 closes many times, and a node at its cap in batch k is taken again in batch k + 1;
    every closed_by value in one call"""
    tb = _tb()
    fb, ho = tb.crafted([(900, tb.random_moves(900, 400, 12, 12, 5, width=W, most=W)), (300, tb.random_moves(300, 120, 12, 12, 6, width=W, most=W))], width=W)
    caps = ({"inbound": 1}, {"outbound": 1}, {"inbound": 2, "outbound": 2, "max_moves": 5})

    def show(i, w):
        assert len(w.moves) == 520
        if i < 2:
            assert B.replay(w.moves, caps[i]).most_closes >= 4
        else:
            assert {b["closed_by"] for b in w.batches} == {B.END, B.MAX_MOVES, B.INBOUND, B.OUTBOUND}
    return Case("batches", fb, ho, caps, show)


def _b_max_moves():
    tb = _tb()
    fb, ho = tb.crafted([(700, tb.random_moves(700, 300, 12, 12, 3))])
    sizes = (1, 64, 65, 256, 257)
    caps = tuple({"max_moves": m} for m in sizes)

    def show(i, w):
        m = sizes[i]
        assert [b["n_moves"] for b in w.batches] == [m] * (300 // m) + ([300 % m] if 300 % m else [])
        assert all(b["closed_by"] == B.MAX_MOVES for b in w.batches[:-1]) and w.batches[-1]["closed_by"] == B.END
    return Case("batches", fb, ho, caps, show)


def _b_node_limit(sparse, W=8, N=abi.KAS_BATCH_NODE_LIMIT):
    fb, ho, n_moves, special = _node_limit(N, sparse, W)
    caps = ({"inbound": 2},)

    def show(i, w):
        _show_node_limit(w, n_moves, special, N)
        assert w.record["n_batches"] >= 30 and w.record["closed_by_inbound"] == w.record["n_batches"] - 1
        assert B.replay(w.moves, caps[0]).replayed == 3
    return Case("batches", fb, ho, caps, show, select=(0, -1, 0))


# A kas_plan takes lists 8 wide up to 4,094 brokers and lists 5 wide up to 7,989 (tests/plan_edges.py, the ceilings of "rf8" and
# "rf5"), and 16-bit cells for lists up to 3 wide only: the library never launches the passes beyond that, so the node limits are
# reached at width 3 and the widest instances at the plan's own ceilings.  name -> (sparse, W[, N]); N: the pass's node limit
W8_CEILING, W5_CEILING = 4094, 7989
PLAN_LIMITS = {"node_limit_w3_dense": (False, 3), "node_limit_w3_sparse": (True, 3),
               "plan_limit_w5_dense": (False, 5, W5_CEILING), "plan_limit_w5_sparse": (True, 5, W5_CEILING),
               "plan_limit_w8_dense": (False, 8, W8_CEILING), "plan_limit_w8_sparse": (True, 8, W8_CEILING)}

EXCEED = {"exceed_at_%d" % pos: (3, pos - 1, pos) for pos in (64, 65, 127, 128, 200, 255)}
# ... and with no move of wavefront 0 among the three: only a ballot of wavefront 1, 2 or 3 sees the counter above its cap
EXCEED.update({"exceed_in_wave_%d" % w: (64 * w + 1, 64 * w + 5, 64 * w + 63) for w in (1, 2, 3)})
EXCEED["exceed_across_waves"] = (70, 130, 200)

_BATCHES = {}
for _n in (GROUP - 1, GROUP, GROUP + 1):
    for _w in (3, 5, 8):
        _BATCHES["group_%d_w%d" % (_n, _w)] = (_b_group, (_n, _w))
for _w in (3, 5, 8):
    _BATCHES["three_tiles_w%d" % _w] = (_b_three_tiles, (_w,))
    _BATCHES["tile_edges_w%d" % _w] = (_b_tile_edges, (_w,))
for _name, _rows in EXCEED.items():
    _BATCHES[_name] = (_b_exceed, (_rows,))
_BATCHES["cap_at_group_end"] = (_b_cap_at_group_end, ())
_BATCHES["cap_reached_in_group"] = (_b_cap_reached_in_group, ())
_BATCHES["many_closes_w3"] = (_b_many_closes, (3,))
_BATCHES["many_closes_w8"] = (_b_many_closes, (8,))
_BATCHES["max_moves"] = (_b_max_moves, ())
_BATCHES["node_limit_dense"] = (_b_node_limit, (False,))
_BATCHES["node_limit_sparse"] = (_b_node_limit, (True,))
for _name, _args in PLAN_LIMITS.items():
    _BATCHES[_name] = (_b_node_limit, _args + ((abi.KAS_BATCH_NODE_LIMIT,) if len(_args) == 2 else ()))


# ---- the rounds pass -------------------------------------------------------------------------------------------------------------
ROUND_CAPS = ({"inbound": 1}, {"inbound": 3, "outbound": 2}, {"outbound": 1}, {"inbound": BIG})
THREE_TILES_ROUNDS = {5: (702, 314, 518, 1), 8: (1070, 471, 900, 1)}     # n_rounds under ROUND_CAPS, from the checker


def _r_three_tiles(W):
    fb, ho = _three_tiles(W)

    def show(i, w):
        assert len(w.moves) == 1620
        if W in THREE_TILES_ROUNDS:
            assert w.record["n_rounds"] == THREE_TILES_ROUNDS[W][i], (W, i, w.record["n_rounds"])
        if i == 0:
            assert min(w.round_of[1100:]) > 0                                # a node's word is carried over a tile boundary
            assert W != 8 or w.record["n_rounds"] > WINDOW                    # a realistic list that crosses the window
        if i == 3:
            assert w.record["n_rounds"] == 1 and w.record["max_round_moves"] == 1620
    return Case("rounds", fb, ho, ROUND_CAPS, show)


def _r_window(n):
    """n moves that all bring a replica to node 11 under cap_inbound 1: n rounds; at 1,024 and 2,048 the last window is exactly
    full, at 1,025 and 2,049 the next one holds one round.  Round strides that cut inside either window."""
    tb = _tb()
    moved = {p: [p % 11, (p + 1) % 11, 11] for p in range(0, 2 * n, 2)}
    fb, ho = tb.crafted([(2 * n, moved)], N=12, n_cur=11)
    caps = ({"inbound": 1},)

    def show(i, w):
        assert len(w.moves) == n and all(m[2] == (11,) for m in w.moves)
        assert w.record["n_rounds"] == n and w.round_of == list(range(n))
    return Case("rounds", fb, ho, caps, show, select=(0, -1, 0), strides=(None, (n, n), (n - 1, n), (1025, n), (1024, n), (0, 0)))


def _r_window_1100_cap2():
    tb = _tb()
    moved = {p: [p % 11, (p + 1) % 11, 11] for p in list(range(0, 2400, 2))[:1100]}
    fb, ho = tb.crafted([(2400, moved)], N=12, n_cur=11)

    def show(i, w):
        assert len(w.moves) == 1100 and w.record["n_rounds"] == 550 and w.record["max_round_moves"] == 2   # one walk
    return Case("rounds", fb, ho, ({"inbound": 2},), show)


def _r_split(P):
    """every row brings node 11.  65,535 rows: 16 round bits and 16 `used` bits, and under cap 65,535 / 65,534 `used` reaches the
    all-ones mask / one below it; 65,536 rows: 17 round bits, 15 `used` bits, cap 32,767 is the mask."""
    tb = _tb()
    fb, ho = tb.crafted([(P, {p: [p % 11, (p + 1) % 11, 11] for p in range(P)})], N=12, n_cur=11)
    if P == 65535:
        caps, rounds = ({"inbound": 65535}, {"inbound": 65534}), (1, 2)
    else:
        assert P == 65536
        caps, rounds = ({"inbound": 32767}, {"inbound": 300}, {"inbound": 65537}), (3, 219, 1)

    def show(i, w):
        cap = caps[i]["inbound"]
        assert len(w.moves) == P and w.record["n_rounds"] == rounds[i]
        assert w.record["max_round_moves"] == min(cap, P) and w.record["raised_by_inbound"] == max(P - cap, 0)
        assert w.round_of == [k // cap for k in range(P)]
    return Case("rounds", fb, ho, caps, show, strides=(lambda w: (w.record["n_rounds"] + 2, P),))


def _r_node_limit(sparse, W=8, N=abi.KAS_ROUND_NODE_LIMIT):
    fb, ho, n_moves, special = _node_limit(N, sparse, W)

    def show(i, w):
        _show_node_limit(w, n_moves, special, N)
        assert w.record["n_rounds"] == R.lower_bound(w.moves, {"inbound": 2}) >= 30 and w.record["raised_by_outbound"] == 0
    return Case("rounds", fb, ho, ({"inbound": 2},), show, select=(0, -1, 0))


_ROUNDS = {"three_tiles_w%d" % w: (_r_three_tiles, (w,)) for w in (3, 5, 8)}
_ROUNDS.update({"window_%d" % n: (_r_window, (n,)) for n in (WINDOW, WINDOW + 1, 2 * WINDOW, 2 * WINDOW + 1)})
_ROUNDS["window_1100_cap2"] = (_r_window_1100_cap2, ())
_ROUNDS["split_65535"] = (_r_split, (65535,))
_ROUNDS["split_65536"] = (_r_split, (65536,))
_ROUNDS["node_limit_dense"] = (_r_node_limit, (False,))
_ROUNDS["node_limit_sparse"] = (_r_node_limit, (True,))
for _name, _args in PLAN_LIMITS.items():
    _ROUNDS[_name] = (_r_node_limit, _args + ((abi.KAS_ROUND_NODE_LIMIT,) if len(_args) == 2 else ()))

BATCH_CASES = tuple(_BATCHES)
ROUND_CASES = tuple(_ROUNDS)
# out lists that name an id outside the broker set: no 16-bit form (cells16_form raises), int32 cells only
INT32_ONLY = frozenset(EXCEED) | {"cap_at_group_end", "cap_reached_in_group"}


def width_of(case) -> int:
    """the plan's width class for the case's tables"""
    return max(int(x) for x in list(case.fb.topics["cur_width"]) + list(case.fb.topics["out_width"]))


def plan_refusal(name, case, cells16):
    """"" or the text a kas_plan refuses the case's shape with: the emulator drives the kernel bodies beyond what the library
    plans (held to the planner itself by tests/test_batches_cpu.py::test_crafted_cases_the_plan_refuses)"""
    if name in ("node_limit_dense", "node_limit_sparse"):
        return "x width 8 needs"
    if cells16 and width_of(case) > 3:
        return "16-bit cells: lists up to 3 wide"
    return ""


def runs(names):
    """(case name, cells16) for every run of the cases `names`: int32 cells, and 16-bit cells where the form exists"""
    return [(n, False) for n in names] + [(n, True) for n in names if n not in INT32_ONLY]


def run_id(run):
    return "%s-%s" % (run[0], "cells16" if run[1] else "int32")


@lru_cache(maxsize=None)
def batches_case(name) -> Case:
    make, args = _BATCHES[name]
    return make(*args)


@lru_cache(maxsize=None)
def rounds_case(name) -> Case:
    make, args = _ROUNDS[name]
    return make(*args)

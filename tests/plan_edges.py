"""Broker counts at which the plan changes kernels, workgroup widths or LDS layouts, and batches that solve exactly there.

kas_shape_batch (csrc/kas_plan_math.h) and the launch resolver (csrc/kas_launch_plan.h) choose from the largest broker count of
the batch.  Every change point is where a packed field, a 16-bit LDS offset or an LDS carve-up holds its last valid value, and the
ceiling of a family is a launch whose last node block ends on the last byte of the allocation.  EDGES pins the change points per
family; find_edges() bisects them out of the planner again (tests/test_emu_plan_edges.py holds the two together, so a threshold
that moves is a deliberate edit of the table); case() builds a batch whose largest broker count is a given one, for the emulator
(tests/test_emu_plan_edges.py) and the MI355X (tests/test_hip_plan_edges.py) to solve against the oracle.

The rows of EDGES for lists 3, 5 and 8 wide without a Context were measured once by hand and are kept as measured; the row of the
Context family is what the bisection over the planner found ('Plan edges').
"""
from __future__ import annotations

import re
from dataclasses import dataclass
from typing import Dict, Tuple

import numpy as np

import emu_lib
from impact_batches import slack
from kafka_assigner_amd import abi
from kafka_assigner_amd import generator as G
from kafka_assigner_amd.flatten import FlatBatch, index_form, node_set_batch

RACKS = 20                              # broker b on rack b mod 20, in the probe and in the cases (case_racks)
N_FIRST = 32                            # the bisection starts here
N_LIMIT = 32767                         # KAS_N_LIMIT: no family is probed beyond it
GRID = 64                               # the description is read at every multiple of GRID, and bisected between two that differ


@dataclass(frozen=True)
class Family:
    rf: int
    flags: int = 0                      # KAS_PLAN_* switches of the plan
    cells16: bool = False               # kas_plan_create16 / kas_solve_host16: uint16 node-index cells
    id_step: int = 1                    # broker b is known as id_step * b, in the broker set and in the rows
    ctx: bool = False                   # every scenario hands a Context in and wants it back (ctx_width == rf)
    rows: int = 20000                   # rows of the probe's topic.  Three of the pinned edges are not about the broker count but
                                        # about rows per broker, ceil(rows * rf / n), crossing a count-field bound (1,023 at 117
                                        # brokers of the ticket family and at 97 of RF 5; 2,039 at 49 of RF 5): they hold for
                                        # this row count, and case() gives its larger scenario as many rows where 3 a broker are fewer


FAMILIES: Dict[str, Family] = {
    "rf3": Family(3),
    "rf3_cells16": Family(3, cells16=True),
    "rf3_sparse": Family(3, id_step=3),
    "rf3_ticket": Family(3, flags=abi.KAS_PLAN_TICKET_ORDER, rows=40000),
    "rf5": Family(5),
    "rf8": Family(8),
    "rf3_ctx": Family(3, ctx=True),
}

# family -> (the last broker count before each change of the description, ascending; the ceiling: the last count the plan takes)
EDGES: Dict[str, Tuple[Tuple[int, ...], int]] = {
    "rf3": ((1219, 1392, 1646, 1880, 2047, 2499, 2856, 5059, 5782, 6745, 7931, 8096), 13492),
    "rf3_cells16": ((1219, 1392, 1646, 1880, 2499, 2856, 5059, 5782, 6745, 8096), 13492),
    "rf3_sparse": ((1084, 1219, 1463, 1646, 2047, 2222, 2499, 4497, 5059, 6226, 7358, 7931), 11564),
    "rf3_ticket": ((117, 1219, 1392, 1646, 1880, 2339, 2499, 2856, 5059, 5782, 6745, 8096, 8191), 13492),
    "rf5": ((49, 97, 5764), 7989),
    "rf8": ((4016,), 4094),
    "rf3_ctx": ((1219, 1392, 1646, 1880, 2499, 2856, 5059, 5287, 5782, 6745), 6824),     # (the round form must fit beside it)
}


# ---- the probe: descriptors only, nothing is solved ------------------------------------------------------------------------
def probe_batch(family: str, n: int) -> FlatBatch:
    """one scenario of one topic over n brokers (the descriptor pattern of tests/test_launch_plan.py::_batch)"""
    f = FAMILIES[family]
    ids = [(np.arange(n, dtype=np.int64) * f.id_step).astype(np.int32)]
    racks = [(np.arange(n) % RACKS).astype(np.int32)]
    fb = node_set_batch(ids, racks, f.rows, f.rf, f.rf)
    if f.ctx:
        fb.scen["ctx_off"][0] = 0
        fb.scen["ctx_width"][0] = f.rf
    return fb


def normalised(text: str) -> str:
    """a description without its lds= and grid= numbers: they move with every broker, the kernels and layouts do not"""
    return re.sub(r"\b(lds|grid)=\d+", r"\1=", text)


def probe(family: str, n: int):
    """(return code, normalised description or the refusal) of the family's plan at n brokers"""
    f = FAMILIES[family]
    rc, text = emu_lib.describe(probe_batch(family, n), f.flags, f.cells16)
    return rc, normalised(text) if rc == 0 else text


def find_edges(family: str) -> Tuple[Tuple[int, ...], int]:
    """(edges, ceiling) of a family, from the planner: the ceiling is the last broker count from N_FIRST on that is not refused,
    an edge is a count n below it whose description differs from that of n + 1.  The description is read on a grid and bisected
    between grid points that differ (a layout that changed and changed back inside one grid cell would be missed)."""
    seen: Dict[int, Tuple[int, str]] = {}

    def at(n):
        if n not in seen:
            seen[n] = probe(family, n)
        return seen[n]
    assert at(N_FIRST)[0] == 0, (family, at(N_FIRST))
    lo, hi = N_FIRST, 2 * N_FIRST                    # lo is taken, hi is refused (or N_LIMIT + 1)
    while hi <= N_LIMIT and at(hi)[0] == 0:
        lo, hi = hi, 2 * hi
    hi = min(hi, N_LIMIT + 1)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if at(mid)[0] == 0 else (lo, mid)
    ceiling = lo
    points = sorted(set(range(N_FIRST, ceiling, GRID)) | {ceiling})
    edges = []
    for a, b in zip(points, points[1:]):
        assert at(a)[0] == 0 and at(b)[0] == 0, (family, a, b, "refused below the ceiling")
        stack = [(a, b)]
        while stack:
            a, b = stack.pop()
            if at(a)[1] == at(b)[1]:
                continue
            if b - a == 1:
                edges.append(a)
                continue
            mid = (a + b) // 2
            stack += [(a, mid), (mid, b)]
    return tuple(sorted(edges)), ceiling


# ---- the cases: batches that solve at a given largest broker count ---------------------------------------------------------------
TAIL = 64                               # the smaller scenario has at least this many brokers fewer (where n leaves room for that)
ROWS_PER_BROKER = 3


def case_sizes(n: int) -> Tuple[int, int, int]:
    """(base0, add, base1): scenario 0 is a cluster of base0 brokers plus `add` new ones, n in all ('add_k'); scenario 1 a cluster of
    base1 brokers less one ('remove1'), at least TAIL brokers fewer than n.  From 2 * TAIL + N_FIRST brokers on the two share their
    base cluster.  Below that there is no room for a tail of 64 above the probe's first count (the pinned edges at 49, 97 and 117
    brokers): scenario 0 then adds a sixteenth of n and scenario 1 has half of n, which still leaves the layout's tail unused."""
    if n - TAIL >= TAIL + N_FIRST:
        return n - TAIL + 1, TAIL - 1, n - TAIL + 1
    add = max(n // 16, 1)
    return n - add, add, (n + 1) // 2 + 1


def roomy_rows(P: int, rf: int, n: int) -> int:
    """impact_batches.roomy_P among the row counts that keep P's cap: the P' in (P - n, P] with ceil(P' rf / n) == ceil(P rf / n)
    that leaves first fit the most free slots (the cap is what the planner's count-field bounds look at)"""
    cap = -(-P * rf // n)
    return max((q for q in range(max(P - n + 1, 1), P + 1) if -(-q * rf // n) == cap), key=lambda q: (slack(q, rf, n), q))


def _pool(fb_parts):
    return np.concatenate(fb_parts).astype(np.int32)


_CASES: Dict[Tuple[str, int], FlatBatch] = {}


def case_racks(n: int) -> int:
    """RACKS; 10 for the two cases below 64 brokers (RF 5, edge 49): on 20 racks of two or three brokers the reference's first fit
    strands a partition in both scenarios of the 50-broker case.  On 10 racks the smaller scenario of either case solves; the
    larger one (2,041 and 2,000 rows a broker, fewer than 50 free slots in 100,000) fails in the reference on 5, 7, 10 and 20
    racks alike, on either side of the edge — assert_case_counts holds either way, and the edge's two order kernels are reached by
    the smaller scenario"""
    return RACKS if n >= 64 else 10


TIGHT_SEED = {"rf3_ctx": 5}             # moves the tight scenario's draw on to one that the reference's first fit does strand


def tight(family: str, n: int) -> bool:
    """the family's ceiling: scenario 1 gets rows that fill every broker to the cap exactly (no free slot).  The reference's first fit
    then strands a partition, so the family compares a failing scenario's status and partition id too — at the broker count where
    the layouts are at their limit, next to a scenario that solves"""
    return n == EDGES[family][1]


def case(family: str, n: int) -> FlatBatch:
    """Two scenarios of one topic each (case_sizes): scenario 0 adds brokers up to exactly n, scenario 1 removes one from a cluster
    at least TAIL brokers smaller and so walks a layout sized for n with its tail unused.  Rows are generator.random_assignment's
    over the scenario's cluster before its action, at least ROWS_PER_BROKER per broker (scenario 0: at least the probe's row count
    too), cut to the count that leaves first fit the most room under the same cap (roomy_rows; none at all where tight() says so).
    Scenario 1's lists are one narrower than the batch's (RF 2 in an RF 3 family; not where it is tight()): its rows carry a pad
    cell through the order kernel, whose holder is the row behind the last broker's — the last one of a layout sized for n.
    n_max == n is asserted.  Built once per (family, n) and shared: the tests leave it as it is."""
    key = (family, n)
    if key in _CASES:
        return _CASES[key]
    f = FAMILIES[family]
    base0, add, base1 = case_sizes(n)
    R = case_racks(n)
    assert min(base0, base1 - 1) >= max(f.rf + 2, R), (family, n, base0, base1)
    sets = [(base0, G.perturb_brokers(base0, R, add=add)), (base1, G.perturb_brokers(base1, R, remove=[(7 * n + 3) % base1]))]
    S = len(sets)
    scen = np.zeros(S, dtype=abi.SCENARIO_DESC_DTYPE)
    topics = np.zeros(S, dtype=abi.TOPIC_DESC_DTYPE)
    curs, ctx = [], []
    node_off = cell_off = ctx_off = 0
    for s, (base, b) in enumerate(sets):
        nb = int(b.node_id.shape[0])
        strand = s == 1 and tight(family, n)
        w = f.rf if s == 0 or strand else f.rf - 1           # scenario 1: lists one narrower than the batch's
        seed = 1000 * f.rf + 2 * n + s
        if strand:
            P = (ROWS_PER_BROKER + 1) * nb
            assert slack(P, w, nb) == 0
            seed += TIGHT_SEED.get(family, 0)
        else:
            P = roomy_rows(max(ROWS_PER_BROKER * nb + nb // 2, f.rows if s == 0 else 0), w, nb)
        assert P >= ROWS_PER_BROKER * nb
        cur = G.random_assignment(seed, P, base, R, w)
        scen[s] = (nb, s, 1, f.rf if f.ctx else 0, node_off, ctx_off if f.ctx else -1)
        topics[s] = (3644, P, w, w, w, 0, cell_off, cell_off, -1, -1, -1)
        curs.append(cur.reshape(-1).astype(np.int64) * f.id_step)
        if f.ctx:
            ctx.append(np.random.default_rng([n, s, 0xC7]).integers(0, 60, size=nb * f.rf))
            ctx_off += nb * f.rf
        node_off += nb
        cell_off += P * w
    fb = FlatBatch(scen=scen, topics=topics, node_id=_pool([b.node_id.astype(np.int64) * f.id_step for _, b in sets]),
                   node_rack=_pool([b.node_rack for _, b in sets]), cur=_pool(curs), aux=np.zeros(0, np.int32),
                   ctx=_pool(ctx) if ctx else np.zeros(0, np.int32), out_len=cell_off)
    assert int(fb.scen["n_nodes"].max()) == n == int(fb.scen["n_nodes"][0]), (family, n, fb.scen["n_nodes"])
    assert int(fb.scen["n_nodes"][1]) <= n - min(TAIL, n // 2), (family, n, fb.scen["n_nodes"])
    _CASES[key] = fb
    return fb


_WANT: Dict[Tuple[str, int], object] = {}


def reference(family: str, n: int):
    """The oracle's solve of case(family, n), once per (family, n): of the batch itself, or of its index form with a uint16 out
    pool for the family with 16-bit cells (what kas_solve_host16 returns; tests/test_cells16.py holds the two forms together)."""
    key = (family, n)
    if key not in _WANT:
        from oracle_lib import oracle_solve
        fb = case(family, n)
        if FAMILIES[family].cells16:
            ho = oracle_solve(index_form(fb))
            ho.out = np.where(ho.out < 0, abi.KAS_CELL16_NONE, ho.out).astype(np.uint16)
        else:
            ho = oracle_solve(fb)
        _WANT[key] = ho
    return _WANT[key]


def sides(family: str):
    """every broker count the family is solved at: both sides of every edge, and the ceiling"""
    edges, ceiling = EDGES[family]
    return sorted({m for n in edges for m in (n, n + 1)} | {ceiling})


def assert_case_counts(family: str, n: int):
    """From the oracle's solve alone: some scenario of the case is KAS_OK and moved replicas (a failed scenario never reaches the
    preference ordering, an unmoved one compares a copy)."""
    sr = reference(family, n).scenario_results[:2]
    good = (sr["status"] == abi.KAS_OK) & (sr["moved_replicas"] > 0)
    assert good.any(), (family, n, sr["status"].tolist(), sr["moved_replicas"].tolist())


def first_fit_failures(family: str) -> int:
    """scenarios of the family's cases the oracle fails in first fit (KAS_FAIL_UNASSIGNABLE): their failing ids are compared too"""
    return sum(int((reference(family, n).scenario_results["status"][:2] == abi.KAS_FAIL_UNASSIGNABLE).sum()) for n in sides(family))

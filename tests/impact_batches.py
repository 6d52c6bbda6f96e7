"""Batches for the impact tests (tests/test_impact_cpu.py, tests/test_impact_gpu.py) and the guard that keeps them meaningful.

The impact pass counts rows of KAS_OK topics only, so a batch whose topics fail compares zeros with zeros.  Topics here start
from a rack-diverse assignment (generator.random_assignment) over brokers 0..N-1 on R racks of equal size, solved against a
broker set perturbed the way the reference's CLI flags do (generator.perturb_brokers: remove / add / replace / as is); ragged
rows, partition sets that differ from the keys and a sparse id space are applied on top of that.  The reference's first fit is
fragile: it wants racks of (nearly) equal size, some 30 brokers or more and free slots under the cap (roomy_P).  assert_exercises() then checks, on
the oracle's result alone, that the batch counts what its test says it counts.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Optional, Sequence

import numpy as np

from kafka_assigner_amd import abi
from kafka_assigner_amd import generator as G
from kafka_assigner_amd.flatten import Scenario, Topic, flatten

IDMAP_CAP = 16384                       # KAS_IDMAP_CAP (kas_plan_math.h): id ranges up to this take the direct table


@dataclass
class T:
    """One topic: P rows of `cw` replicas drawn by G(seed), solved at replication factor `rf`."""
    P: int
    cw: int = 3
    rf: int = 3
    ragged: float = 0.0                 # fraction of rows cut to a random shorter length (cur_len)
    parts: bool = False                 # partitions= differs from the keys: two keys left out, two ids added
    noise: int = 8
    exact: bool = False                 # P as given (else the nearest P below it that leaves first fit the most room)
    balanced: bool = False              # rows of a cyclic assignment in random order, one in `noise` drawn by G: thousands of rows
                                        # still solve (first fit leaves its free slots on the last brokers it visits, and the
                                        # slack never exceeds N - 1 slots, so a late row that wants two brokers is stranded)


def n_in(P: int, parts: bool) -> int:
    """partitions the solve counts (KAS:45): the keys, or what T.parts makes of them"""
    return P                            # (T.parts leaves two keys out and adds two ids)


def slack(P_in: int, rf: int, n_nodes: int) -> int:
    """Replica slots the cap of ceil(P rf / N) per broker (KAS:65-71) leaves free.  The reference's first fit strands a
    partition (KAS_FAIL_UNASSIGNABLE) when few are: the brokers left with room then share racks with the row's holders."""
    return n_nodes * -(-P_in * rf // n_nodes) - P_in * rf


def roomy_P(P: int, rf: int, n_nodes: int, parts: bool = False) -> int:
    """the P' in (P - n_nodes, P] with the largest slack (rows left out of `partitions` keep their replicas: they use slots
    the cap does not count)"""
    return max(range(max(P - n_nodes + 1, 1), P + 1), key=lambda q: (slack(n_in(q, parts), rf, n_nodes), q))


def roomy_N(P: int, rf: int, N: int, delta: int = 0, span: int = 12) -> int:
    """the N' in [N, N + span) for which a broker set of N' + delta brokers has the largest share of free slots"""
    return max(range(N, N + span), key=lambda n: (slack(P, rf, n + delta) / (n + delta), -n))


def sparse(b: int) -> int:
    """39 brokers span more than KAS_IDMAP_CAP ids: the binary search"""
    return b * 1009 + 7


def edge_ids(N: int, span: int) -> Callable[[int], int]:
    """brokers 0..N-2 as they are, broker N-1 at span - 1 (ids beyond follow it): a set 0..N-1 spans exactly `span` ids"""
    return lambda b: b if b < N - 1 else span - 1 + (b - (N - 1))


def scenario(seed: int, N: int, R: int, topics: Sequence[T], remove: Sequence[int] = (), add: int = 0,
             ids: Optional[Callable[[int], int]] = None, rack_aware: bool = True) -> Scenario:
    """Brokers 0..N-1 (rack b mod R) minus `remove` plus `add` new ones; every topic's current assignment is over 0..N-1,
    so replicas on removed brokers are departed.  ids: broker b is known as ids(b), in the broker set and in the rows."""
    bs = G.perturb_brokers(N, R, remove=remove, add=add, rack_aware=rack_aware)
    ids = ids or (lambda b: b)
    brokers = [ids(int(b)) for b in bs.node_id]
    racks = {ids(int(b)): "r%d" % int(r) for b, r in zip(bs.node_id, bs.node_rack)}
    out = []
    for k, t in enumerate(topics):
        rng = np.random.default_rng([seed, k, 0x1A])
        P = t.P if t.exact else roomy_P(t.P, t.rf, len(brokers), t.parts)
        cur = G.random_assignment(seed * 16 + k, P, N, R, t.cw)
        if t.balanced:
            cyc = G.cyclic_assignment(P, N, t.cw)[rng.permutation(P)]
            cur = np.where((np.arange(P) % t.noise == 0)[:, None], cur, cyc)
        rows = {}
        for p in range(P):
            reps = [ids(int(b)) for b in cur[p]]
            if t.cw > t.rf and p % 60:                                  # RF lowered: most rows are rf long already
                reps = reps[:t.rf]
            if t.ragged and p > 0 and rng.random() < t.ragged:         # (row 0 stays whole: cur_width is t.cw)
                reps = reps[:int(rng.integers(0, len(reps)))]
            rows[p] = reps
        parts = None
        if t.parts:
            parts = set(range(P)) - {int(x) for x in rng.choice(P, 2, replace=False)} | {P + 3, P + 7}
        out.append(Topic("t%d-%d" % (seed, k), rows, t.rf, partitions=parts))
    return Scenario(brokers=brokers, racks=racks, topics=out)


def lookup_kind(fb, s: int) -> str:
    """how int32 cells of scenario s find their node (kas_impact_body.h, node_of): 'direct' table or 'bsearch'"""
    n, off = int(fb.scen["n_nodes"][s]), int(fb.scen["node_off"][s])
    if n == 0:
        return "none"
    span = int(fb.node_id[off + n - 1]) - int(fb.node_id[off]) + 1
    return "direct" if 1 <= span <= IDMAP_CAP else "bsearch"


def assert_exercises(fb, ho, want, must_solve: Sequence[int] = (), merge: bool = False, widths=(), lookups=(), ok_share=0.75):
    """A condition on the batch, from the oracle's solve `ho` and the checker's records `want` alone: the test that calls this
    compares counted rows, not zeros.
      - at least `ok_share` of the topics are KAS_OK, and every topic of the scenarios in `must_solve`;
      - inbound, outbound, leaders_before, departed_replicas and leaders_moved are non-zero over the batch;
      - merge: some scenario has two or more OK topics that counted rows;
      - widths: for each (cur_width, out_width) or (cur_width, out_width, rf) an OK topic of that shape with rows exists;
      - lookups: for each of 'direct' / 'bsearch' an OK topic with rows in a scenario of that kind exists."""
    nodes, scen = want
    status = ho.topic_results["status"][:fb.n_topics]
    ok = status == abi.KAS_OK
    assert fb.n_topics > 0 and ok.sum() >= ok_share * fb.n_topics, ("too few topics solve", status.tolist())
    counted = ok & (fb.topics["n_partitions"] > 0)
    owner = np.full(fb.n_topics, -1, dtype=np.int64)
    for s in range(fb.n_scenarios):
        b, c = int(fb.scen["topic_begin"][s]), int(fb.scen["topic_count"][s])
        owner[b:b + c] = s
    for s in must_solve:
        mine = owner == s
        assert mine.any() and ok[mine].all(), ("scenario must solve", s, status[mine].tolist())
        assert int(nodes["replicas_after"][_block(fb, s)].sum()) > 0, ("scenario must count rows", s)
    for f in ("inbound", "outbound", "leaders_before"):
        assert int(nodes[f].sum()) > 0, f
    for f in ("departed_replicas", "leaders_moved"):
        assert int(scen[f].sum()) > 0, f
    if merge:
        assert max(int(counted[owner == s].sum()) for s in range(fb.n_scenarios)) >= 2, "no scenario merges two OK topics"
    for w in widths:
        hit = counted & (fb.topics["cur_width"] == w[0]) & (fb.topics["out_width"] == w[1])
        if len(w) > 2:
            hit &= fb.topics["rf"] == w[2]
        assert hit.any(), ("no OK topic of (cur_width, out_width[, rf])", w)
    kinds = {lookup_kind(fb, int(owner[t])) for t in np.nonzero(counted)[0]}
    for k in lookups:
        assert k in kinds, ("no OK topic looks its nodes up by", k, kinds)


def _block(fb, s):
    base = np.concatenate([[0], np.cumsum(np.clip(fb.scen["n_nodes"], 0, None))]).astype(np.int64)
    return slice(int(base[s]), int(base[s + 1]))


# ---- the batches ----------------------------------------------------------------------------------------------------------
CLUSTERS = ((30, 5), (36, 6), (40, 8), (40, 10), (32, 4), (35, 5))      # (brokers, racks): racks of equal size


def mixed_batch(seed: int, n_scen: int = 4, max_p: int = 600):
    """What the impact tests call a random batch: remove / add / replace / as is, one to three topics per scenario, ragged
    rows, partition sets that are not the keys, lists 2 and 3 wide, replicas on brokers outside the set."""
    rng = np.random.default_rng([seed, 0x1B])
    scs = []
    for s in range(n_scen):
        N, R = CLUSTERS[int(rng.integers(len(CLUSTERS)))]
        act = ("remove", "add", "replace", "as_is")[s % 4]
        remove = sorted(int(b) for b in rng.choice(N, 1 + int(rng.integers(0, 2)), replace=False)) if act in ("remove", "replace") else []
        add = int(rng.integers(1, 4)) if act in ("add", "replace") else 0
        topics = [T(P=int(rng.integers(2 * N, max_p)), cw=int(rng.integers(2, 4)), rf=3, ragged=0.15 if (s + k) % 2 else 0.0,
                    parts=(s + k) % 3 == 0) for k in range(1 + (s + seed) % 3)]
        scs.append(scenario(seed * 100 + s, N, R, topics, remove=remove, add=add))
    return flatten(scs)


def shared_node_range_batch():
    """two scenarios that read one node range (node_off equal): each gets a block of records of its own"""
    a = scenario(5, 30, 5, [T(400)], remove=[4])
    b = scenario(6, 30, 5, [T(400, ragged=0.1)], remove=[4])
    fb = flatten([a, b])
    fb.scen["node_off"][1] = fb.scen["node_off"][0]
    return fb


def widths_4_5_batch(P: int = 300, N: int = 40, R: int = 8, ids=None):
    """(cur_width, rf) = (5,5), (2,4) | (4,4), (5,3), (3,3): the <5> instance, with lists narrower than it on either side"""
    return flatten([scenario(51, N, R, [T(P, 5, 5), T(P - 13, 2, 4, ragged=0.1)], remove=[3, 17], ids=ids),
                    scenario(52, N, R, [T(P, 4, 4, parts=True), T(P + 9, 5, 3), T(P // 2, 3, 3, ragged=0.2)], remove=[8], add=2, ids=ids)])


def widths_6_8_batch(P: int = 300, N: int = 60, R: int = 12, ids=None):
    """(cur_width, rf) = (7,7), (3,6) | (8,8), (8,2): the <8> instance"""
    return flatten([scenario(63, N, R, [T(P, 7, 7), T(P - 13, 3, 6, ragged=0.1)], remove=[3, 17], ids=ids),
                    scenario(64, N, R, [T(P, 8, 8, parts=True), T(P + 9, 8, 2)], remove=[8], add=2, ids=ids)])


def sparse_batch(P: int = 400):
    """every scenario's ids span more than KAS_IDMAP_CAP: sorted ids in the LDS, binary search"""
    return flatten([scenario(71, 40, 8, [T(P), T(P // 2, ragged=0.2)], remove=[5, 30], ids=sparse),
                    scenario(72, 30, 5, [T(P + 17, parts=True)], add=2, ids=sparse)])


def dense_and_sparse_batch(P: int = 400):
    """a dense scenario (direct table) and a sparse one (binary search) in one launch: both use the LDS's lookup region; the
    sparse one has MORE brokers than the dense one's id range has entries"""
    return flatten([scenario(73, 30, 5, [T(P), T(P // 2)], remove=[2]),
                    scenario(74, 40, 8, [T(P + 17, ragged=0.2), T(P // 3)], remove=[5, 30], add=1, ids=sparse),
                    scenario(75, 36, 6, [T(P - 40, parts=True)], add=3)])


def beyond_the_table_batch(P: int = 300, N: int = 30):
    """Sparse ids, the removed broker N-1 above every id of the set: the binary search for its replicas ends one past the
    sorted ids.  On the GPU the LDS there holds whatever the workgroup before left -- its id table, say, with that very broker
    in it -- so only the search's bound keeps such a replica departed (STALE_ID: what a test puts there on the emulator)."""
    return flatten([scenario(78, N, 5, [T(P), T(P // 2)], remove=[N - 1], ids=sparse)])


STALE_ID = sparse(29)


def id_range_edge_batch(P: int = 300, N: int = 30):
    """id ranges of exactly KAS_IDMAP_CAP (the last one on the direct table) and KAS_IDMAP_CAP + 1 (the first one searched)"""
    fb = flatten([scenario(76, N, 5, [T(P)], remove=[2], ids=edge_ids(N, IDMAP_CAP)),
                  scenario(77, N, 5, [T(P)], remove=[2], ids=edge_ids(N, IDMAP_CAP + 1))])
    spans = [int(fb.node_id[int(o) + int(n) - 1]) - int(fb.node_id[int(o)]) + 1 for o, n in zip(fb.scen["node_off"], fb.scen["n_nodes"])]
    assert spans == [IDMAP_CAP, IDMAP_CAP + 1], spans
    return fb


ROW_COUNTS = (1, 511, 512, 513, 1025)   # around ROWS_PER_LANE * KAS_IMPACT_BLOCK = 512 rows, the row loop's stride


def row_counts_batch():
    """one single-topic scenario per row count, each on the cluster size that leaves that many rows the most room"""
    scs = []
    for i, P in enumerate(ROW_COUNTS):
        remove, add = ([i] if i % 2 else []), (1 if i in (2, 3) else 0)
        N = max(range(30, 65, 5), key=lambda n: slack(P, 3, n + add - len(remove)) / n)
        scs.append(scenario(80 + i, N, 5, [T(P, exact=True)], remove=remove, add=add))
    return flatten(scs)


def degenerate_batch():
    """a normal scenario, a scenario without topics (its node records are zeros) and one without brokers (its topic fails;
    no node records, a zero scenario record)"""
    return flatten([scenario(90, 30, 5, [T(300), T(200, ragged=0.2), T(150, parts=True)], remove=[7]),
                    scenario(91, 12, 4, []),
                    Scenario(brokers=[], racks={}, topics=scenario(92, 12, 4, [T(50)]).topics)])


def many_brokers_batch(P: int = 300):
    """7,000 brokers: N x 24 bytes of counters do not fit the LDS next to the id table (the global-scratch path)"""
    N = 7000
    cur = G.random_assignment(11, P, N + 50, 20, 3)
    brokers = list(range(N))
    return flatten([Scenario(brokers, {b: "r%d" % (b % 20) for b in brokers}, [Topic("big", {p: cur[p].tolist() for p in range(P)}, 3)])])


def wide_batch(widths: Sequence[int], P: int, N: int, R: int, seed: int, noise: int = 8):
    """per width one scenario with two removed brokers and rack awareness off and one with one removed broker, thousands of rows"""
    scs = []
    for i, w in enumerate(widths):
        scs.append(scenario(seed + i, N, R, [T(P, w, w, balanced=True, noise=noise)], remove=[3, 17], rack_aware=False))
        scs.append(scenario(seed + 8 + i, N, R, [T(P - 100, w, w, balanced=True, noise=noise)], remove=[5]))
    return flatten(scs)


def big_scenario(P: int, N: int = 60, R: int = 6, seed: int = 0, noise: int = 8):
    """one scenario, one topic of exactly P rows x RF 3: the library cuts it into row ranges of KAS_IMPACT_MIN_ITEM_ROWS = 4096"""
    return flatten([scenario(seed, N, R, [T(P, 3, 3, exact=True, balanced=True, noise=noise)], remove=[1, 13, 40])])


def replan_batches():
    """three batches of one shape (scenario count, topic descriptors, the rows themselves) whose broker sets differ in size:
    what a what-if caller hands one context call after call.  Largest node pool first, so that no buffer has to grow."""
    def one(remove, add):
        return flatten([scenario(30, 40, 8, [T(600, exact=True, balanced=True), T(300, exact=True, ragged=0.1, balanced=True)], remove=remove, add=add),
                        scenario(31, 40, 8, [T(500, exact=True, balanced=True)], remove=remove[:1], add=add)])
    return [one([9], 0), one([9, 20], 0), one([9, 20, 33], 0)]       # (added brokers lower the cap: first fit then strands rows)


def whatif_inputs():
    """(brokers, topics) for whatif.WhatIf: 60 brokers on 6 racks, two topics of uniform RF 3 lists"""
    sc = scenario(40, 60, 6, [T(2990, balanced=True, noise=2, exact=True), T(1190, balanced=True, noise=2, exact=True)])
    return {b: "r%d" % (b % 6) for b in range(60)}, {"orders": dict(sc.topics[0].current), "clicks": dict(sc.topics[1].current)}


# ---- named batches, each built and solved by the oracle once --------------------------------------------------------------
# name -> (builder, what assert_exercises is to find in it)
BATCHES = {
    "mixed7": (lambda: mixed_batch(7), dict(merge=True, widths=[(2, 3), (3, 3)])),
    "mixed8": (lambda: mixed_batch(8), dict(merge=True, widths=[(2, 3), (3, 3)])),
    "mixed21": (lambda: mixed_batch(21, n_scen=3), dict(merge=True)),
    "mixed22": (lambda: mixed_batch(22, n_scen=3), dict(merge=True)),
    "mixed31": (lambda: mixed_batch(31, n_scen=3), dict(merge=True)),
    "mixed42": (lambda: mixed_batch(42, n_scen=6), dict(merge=True, widths=[(2, 3), (3, 3)])),
    "mixed100": (lambda: mixed_batch(100), dict()),
    "mixed101": (lambda: mixed_batch(101), dict()),
    "shared_node_range": (shared_node_range_batch, dict(must_solve=[0, 1])),
    "many_brokers": (many_brokers_batch, dict(must_solve=[0])),
    "widths_4_5": (widths_4_5_batch, dict(must_solve=[0, 1], merge=True, widths=[(5, 5, 5), (4, 4, 4), (2, 4, 4), (5, 5, 3), (3, 3, 3)])),
    "widths_6_8": (widths_6_8_batch, dict(must_solve=[0, 1], merge=True, widths=[(7, 7, 7), (8, 8, 8), (3, 6, 6), (8, 8, 2)])),
    "sparse": (sparse_batch, dict(must_solve=[0, 1], merge=True, lookups=["bsearch"])),
    "dense_and_sparse": (dense_and_sparse_batch, dict(must_solve=[0, 1, 2], merge=True, lookups=["direct", "bsearch"])),
    "id_range_edge": (id_range_edge_batch, dict(must_solve=[0, 1], lookups=["direct", "bsearch"])),
    "beyond_the_table": (beyond_the_table_batch, dict(must_solve=[0], merge=True, lookups=["bsearch"])),
    "row_counts": (row_counts_batch, dict(must_solve=[0, 1, 2, 3, 4])),
    "degenerate": (degenerate_batch, dict(must_solve=[0], merge=True)),
    # the GPU tests' sizes
    "rf_4_5": (lambda: wide_batch((5, 4), 2000, 40, 8, 4), dict(widths=[(5, 5, 5), (4, 4, 4)])),
    "rf_4": (lambda: wide_batch((4,), 2000, 40, 8, 4), dict(widths=[(4, 4, 4)])),
    "rf_7_8": (lambda: wide_batch((7, 8), 1500, 40, 10, 28), dict(widths=[(7, 7, 7), (8, 8, 8)])),
    "rows_4096": (lambda: big_scenario(4096, seed=2, noise=2), dict(must_solve=[0])),
    "rows_4097": (lambda: big_scenario(4097, N=66, seed=2, noise=2), dict(must_solve=[0])),   # (66 brokers leave 57 free slots, 60 only 21)
    "rows_10000": (lambda: big_scenario(10000, seed=2, noise=2), dict(must_solve=[0])),
    "many_brokers_10000": (lambda: many_brokers_batch(10000), dict(must_solve=[0])),
}
_SOLVED = {}


def solved(name: str):
    """(fb, ho, want) of a named batch: the oracle's solve and the checker's records of it, computed once and shared by the
    tests (which leave all three as they are), with the batch's guard already passed"""
    if name not in _SOLVED:
        from impact_ref import impact_ref
        from oracle_lib import oracle_solve
        make, claims = BATCHES[name]
        fb = make()
        ho = oracle_solve(fb)
        want = impact_ref(fb, ho)
        assert_exercises(fb, ho, want, **claims)
        _SOLVED[name] = (fb, ho, want)
    return _SOLVED[name]

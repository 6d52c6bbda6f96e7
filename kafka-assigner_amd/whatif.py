"""What-if planning over ONE cluster snapshot: many broker-set variants, one batch.

The front end SURVEY.md 8(f) N3 describes: the reference's broker-set flags
(--integer_broker_ids / --broker_hosts_to_remove / --disable_rack_awareness,
KafkaAssignmentGenerator.java:137-151, 238-250) decide the solver's `nodes` and rack map; here a
list of such variants is solved against the same current assignment in one launch.  Every topic's
current table is uploaded once and shared by all variants (cur_off of every scenario points at
the same rows), so S variants cost S out tables but one cur table.

    plan = WhatIf(brokers={id: rack or None}, topics={"t": {partition: [replicas]}})
    results = plan.solve([Variant(remove=[5]), Variant(add={9: "c"}), Variant(rack_aware=False)])
    results[0].moved_replicas, results[0].assignment("t")

With impact=True the same call also reduces every variant, on the GPU, to what it does to each broker (include/kas_abi.h,
ABI v6): results[0].broker_impact() -> {broker: {"inbound": ..., ...}}, results[0].max_inbound, ...  rows=False leaves the
variants' rows on the device (kas_solve_host_impact with n_select = 0): only records come back.

best() lets the GPU also compare the variants (kas_solve_host_choose): plan.best(variants, k=3, by=("max_inbound",
"moved_replicas")) returns the three best variants that solve, best first, each with its rows and its per-broker impact;
nothing comes back for the others but their records.

front() returns the variants that no other variant beats on all the named criteria at once (kas_solve_host_front), optionally
among those within hard bounds: plan.front(variants, by=("moved_replicas", "replica_spread"), within={"max_inbound": 200}).

racks=True (with impact=True) adds the rack pass (kas_solve_host_rack_impact): results[0].colocated_after — replicas that share a
rack with another replica of their partition —, .single_rack_rows_after, .new_rack_replicas, ... and results[0].rack_impact() ->
{rack name: {"nodes": ..., "replicas_after": ..., "inbound": ...}}.  The report is against the REAL racks (brokers / Variant.add; a
broker without a rack is a rack of its own, named by its id) whatever rack_aware says, so a rack-unaware variant shows what it
costs.  best() and front() rank and bound by these figures too (kas_solve_host_choose_racks / kas_solve_host_front_racks): name a
rack criterion (abi.RACK_KEY_NAMES: the fields above plus rack_replica_spread and rack_leader_spread) in by= or within=, or pass
racks=True — plan.best(variants, by=("colocated_after", "replica_spread")), plan.front(variants, by=("moved_replicas",
"replica_spread"), within={"single_rack_rows_after": 0}) — and every winner carries the rack figures and rack_impact().

topics=True adds the topic pass (kas_solve_host_topic_impact), with or without impact=True: results[0].topics_moved,
.max_topic_inbound — the most replicas of one topic a single broker must take in —, .max_topic_replica_spread, ... and
results[0].topic_impact() -> {topic name: {"status": ..., "moved_replicas": ..., "max_inbound": ..., "min_replicas_after": ...}}.
best() and front() rank and bound by these figures too (kas_solve_host_choose_topics / kas_solve_host_front_topics): name a topic
criterion (abi.TOPIC_KEY_NAMES) in by= or within=, or pass topics=True — plan.best(variants, by=("max_topic_inbound",
"moved_replicas")), plan.front(variants, by=("moved_replicas", "max_topic_replica_spread"), within={"max_topic_inbound": 40}) — in
any mix with the broker and the rack criteria, and every winner carries the topic figures and topic_impact().

moves=("replicas",) (kinds of abi.MOVE_KINDS: replicas, leader, order) asks for the rows that change instead of every row, compacted
on the GPU (include/kas_abi.h, kas_moves): results[0].moves() -> [(topic, partition, [new replicas], {kinds})] and
results[0].reassignment() -> the Kafka reassignment JSON object of those partitions.  solve(..., moves=...) returns the moves of
every variant and no rows (kas_solve_host_moves); best(..., moves=..., rows=False) those of the winners and no rows at all.

batches={"inbound": 5, "outbound": 0, "max_moves": 0} cuts each variant's replica moves, on the GPU, into the consecutive execution
batches a cluster would be given (include/kas_abi.h, kas_batch_spec: at most 5 moves of a batch bring a replica to the same broker;
0 = no bound): results[0].n_batches, .max_batch_moves, ... and results[0].batches() -> [{"first_move", "n_moves", "topic",
"partition", "replicas", "max_inbound", "max_outbound", "closed_by"}]; with moves=... as well, results[0].reassignment_batches()
-> one Kafka reassignment JSON object per batch.  solve(), best() and front() take it alike.

rounds={"inbound": 5, "outbound": 0} schedules each variant's replica moves, on the GPU, into packed rounds under the same per-broker
caps without keeping list order (include/kas_abi.h, kas_round_spec), in far fewer rounds than consecutive batches take:
results[0].n_rounds, .max_round_moves, ..., results[0].rounds() -> [{"n_moves", "replicas", "first_move", "moves": [indices]}] and,
with moves=... holding "replicas", results[0].reassignment_rounds(max_moves=0) -> one Kafka reassignment JSON object per round (or
per chunk of max_moves partitions of a round).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, Iterable, List, Optional, Sequence

import numpy as np

from . import abi
from .assigner import IllegalStateException, raise_for_status
from .flatten import FlatBatch, java_string_hashcode


@dataclass
class Variant:
    """One what-if: brokers to take out, brokers to add (id -> rack or None), rack awareness."""
    remove: Iterable[int] = ()
    add: Dict[int, Optional[str]] = field(default_factory=dict)
    rack_aware: bool = True                      # False = --disable_rack_awareness (KAG:241)
    label: str = ""


@dataclass
class VariantResult:
    label: str
    status: int                                  # KAS_OK or the first failing topic's status
    fail_topic: Optional[str]
    fail_partition: int
    moved_replicas: int
    moved_partitions: int
    digest: int
    # impact=True (kas_scenario_impact); None without it
    departed_replicas: Optional[int] = None
    leaders_moved: Optional[int] = None
    max_inbound: Optional[int] = None
    max_outbound: Optional[int] = None
    min_replicas_after: Optional[int] = None
    max_replicas_after: Optional[int] = None
    min_leaders_after: Optional[int] = None
    max_leaders_after: Optional[int] = None
    # racks=True (kas_scenario_rack_impact); None without it
    colocated_before: Optional[int] = None
    colocated_after: Optional[int] = None
    rows_colocated_before: Optional[int] = None
    rows_colocated_after: Optional[int] = None
    single_rack_rows_before: Optional[int] = None
    single_rack_rows_after: Optional[int] = None
    new_rack_replicas: Optional[int] = None
    rows_losing_racks: Optional[int] = None
    n_racks: Optional[int] = None
    max_rack_inbound: Optional[int] = None
    max_rack_outbound: Optional[int] = None
    min_rack_replicas_after: Optional[int] = None
    max_rack_replicas_after: Optional[int] = None
    min_rack_leaders_after: Optional[int] = None
    max_rack_leaders_after: Optional[int] = None
    # topics=True (kas_scenario_topic_impact); None without it
    topics_ok: Optional[int] = None
    topics_moved: Optional[int] = None
    topics_leaders_moved: Optional[int] = None
    topics_departed: Optional[int] = None
    max_topic_moved_replicas: Optional[int] = None
    max_topic_moved_partitions: Optional[int] = None
    max_topic_leaders_moved: Optional[int] = None
    max_topic_inbound: Optional[int] = None
    max_topic_outbound: Optional[int] = None
    max_topic_replica_spread: Optional[int] = None
    max_topic_leader_spread: Optional[int] = None
    max_topic_replicas_after: Optional[int] = None
    max_topic_leaders_after: Optional[int] = None
    sum_topic_replica_spread: Optional[int] = None
    sum_topic_leader_spread: Optional[int] = None
    # batches=... (kas_scenario_batches); None without it
    n_batches: Optional[int] = None              # the true count, whatever batch_room
    batch_moves: Optional[int] = None            # replica moves over all batches
    batch_replicas: Optional[int] = None         # replicas brokers receive over all batches
    max_batch_moves: Optional[int] = None
    max_batch_replicas: Optional[int] = None
    closed_by_max_moves: Optional[int] = None    # batches closed for that reason
    closed_by_inbound: Optional[int] = None
    closed_by_outbound: Optional[int] = None
    # rounds=... (kas_scenario_rounds); None without it
    n_rounds: Optional[int] = None               # the true count, whatever round_room
    round_moves: Optional[int] = None            # replica moves over all rounds
    round_replicas: Optional[int] = None         # replicas brokers receive over all rounds
    max_round_moves: Optional[int] = None
    max_round_replicas: Optional[int] = None
    raised_by_inbound: Optional[int] = None      # moves a receiving broker's cap pushed beyond round 0
    raised_by_outbound: Optional[int] = None     # ... that only a giving broker's cap pushed
    rank: Optional[int] = None                   # best(): place among the variants that solve (0 = best); None from solve()
    _plan: "WhatIf" = field(repr=False, default=None)
    _index: int = field(repr=False, default=0)
    _out: np.ndarray = field(repr=False, default=None)
    _nodes: np.ndarray = field(repr=False, default=None)      # this variant's block of kas_node_impact records
    _node_ids: np.ndarray = field(repr=False, default=None)
    _packed_at: Optional[int] = field(repr=False, default=None)   # best(): _out holds this variant's rows packed from here
    _moves: Optional[tuple] = field(repr=False, default=None)     # moves=...: (this variant's kas_move records, its list cells)
    _moves_mask: int = field(repr=False, default=0)               # ... and the kinds that were asked for
    _racks: np.ndarray = field(repr=False, default=None)          # racks=True: this variant's block of kas_rack_impact records
    _rack_names: Optional[list] = field(repr=False, default=None)  # ... and the name of each rack index
    _topics: np.ndarray = field(repr=False, default=None)         # topics=True: this variant's kas_topic_impact records
    _topic_results: np.ndarray = field(repr=False, default=None)  # ... and its kas_topic_result records
    _batches: np.ndarray = field(repr=False, default=None)        # batches=...: this variant's written kas_move_batch records
    _rounds: np.ndarray = field(repr=False, default=None)         # rounds=...: this variant's written kas_move_round records
    _round_of: np.ndarray = field(repr=False, default=None)       # ... and the round of each of its replica moves, as far as written

    def raise_for_status(self):
        """The exception the reference's CLI run would have died with (KAS:183-184 ...)."""
        rf = None
        if self.fail_topic is not None and self._plan is not None:
            rf = self._plan.rfs[self._plan.topic_names.index(self.fail_topic)]
        raise_for_status(self.fail_topic, self.status, self.fail_partition, rf)

    def assignment(self, topic: str) -> Dict[int, List[int]]:
        """partition -> new replica list of `topic` under this variant."""
        if self._out is None:
            raise ValueError("solve(..., rows=False) downloaded no rows: solve with rows=True to read an assignment")
        return self._plan._rows(self._index, topic, self._out, self._packed_at)

    def moves(self, topic: Optional[str] = None, kinds=None) -> list:
        """[(topic, partition, [new replicas], {kinds})]: the partitions that change under this variant, in (topic, partition)
        order, of the kinds asked for with moves=... ({kinds}: every kind that applies to the row).  topic: that topic's only;
        kinds: a subset of the kinds that were asked for."""
        if self._moves is None:
            raise ValueError("no moves: solve(..., moves=(...)) or best(..., moves=(...))")
        mask = self._moves_mask if kinds is None else abi.move_mask(kinds)
        if mask & ~self._moves_mask:
            raise ValueError("kinds that were not asked for with moves=...")
        recs, cells = self._moves
        names = self._plan.topic_names
        out = []
        for r in recs:
            if not int(r["flags"]) & mask or (topic is not None and names[int(r["topic"])] != topic):
                continue
            at = int(r["cell_at"])
            out.append((names[int(r["topic"])], int(r["partition"]), [int(b) for b in cells[at:at + int(r["len"])]],
                        {k for k, bit in abi.MOVE_KINDS.items() if int(r["flags"]) & bit}))
        return out

    def reassignment(self, kinds=None) -> dict:
        """The Kafka reassignment JSON object (version, partitions) holding the partitions of moves(kinds=kinds) only."""
        return {"version": 1, "partitions": [{"topic": t, "partition": p, "replicas": reps} for t, p, reps, _ in self.moves(kinds=kinds)]}

    def batches(self) -> List[dict]:
        """[{first_move, n_moves, topic, partition, replicas, max_inbound, max_outbound, closed_by}]: this variant's execution
        batches (batches=...), in order: consecutive ranges of its replica moves; topic and partition are those of a batch's first
        move, closed_by one of abi.BATCH_CLOSED_BY.  min(n_batches, batch_room) of them."""
        if self._batches is None:
            raise ValueError("no batches: solve(..., batches={...}), best(..., batches={...}) or front(..., batches={...})")
        names = self._plan.topic_names
        out = []
        for r in self._batches:
            d = {f: int(r[f]) for f in abi.MOVE_BATCH_FIELDS}
            d["topic"] = names[d["topic"]]
            d["closed_by"] = abi.BATCH_CLOSED_BY[d["closed_by"]]
            out.append(d)
        return out

    def reassignment_batches(self, kinds=None) -> List[dict]:
        """One Kafka reassignment JSON object per execution batch (batches=... together with moves=...): the partitions of
        moves(kinds=kinds), each in the batch that holds it — a replica move in the batch whose range of the replica move list
        it lies in, any other move (a leader change, a reorder) with the replica move before it, or in the first batch.  The
        objects' partitions, concatenated, are reassignment(kinds)'s.  Raises when n_batches exceeded batch_room."""
        if self._batches is None:
            raise ValueError("no batches: solve(..., batches={...}), best(..., batches={...}) or front(..., batches={...})")
        if self.n_batches > len(self._batches):
            raise ValueError("%d batches, room for %d: ask again with a larger batch_room" % (self.n_batches, len(self._batches)))
        names = self._plan.topic_names
        starts = [(int(r["topic"]), int(r["partition"])) for r in self._batches]       # ascending: the list is in (topic, partition) order
        out = [{"version": 1, "partitions": []} for _ in range(max(len(starts), 1))]
        at = 0
        for t, p, reps, _ in self.moves(kinds=kinds):
            key = (names.index(t), p)
            while at + 1 < len(starts) and starts[at + 1] <= key:
                at += 1
            out[at]["partitions"].append({"topic": t, "partition": p, "replicas": reps})
        return out if starts or out[0]["partitions"] else []

    _NO_ROUNDS = "no rounds: solve(..., rounds={...}), best(..., rounds={...}) or front(..., rounds={...})"

    def _round_members(self) -> List[List[int]]:
        """per round, the list indices of its replica moves, ascending; raises when the room was too small"""
        if self._rounds is None:
            raise ValueError(self._NO_ROUNDS)
        if self.n_rounds > len(self._rounds) or self.round_moves > len(self._round_of):
            raise ValueError("%d rounds of %d moves, room for %d and %d: ask again with a larger round_room"
                             % (self.n_rounds, self.round_moves, len(self._rounds), len(self._round_of)))
        members = [[] for _ in range(self.n_rounds)]
        for i, r in enumerate(self._round_of):
            members[int(r)].append(i)
        return members

    def rounds(self) -> List[dict]:
        """[{n_moves, replicas, first_move, moves}]: this variant's packed rounds (rounds=...): the kas_move_round record and
        `moves`, the indices into its replica move list (moves(kinds=("replicas",))) of the moves the round executes.  Raises
        when n_rounds exceeded round_room."""
        members = self._round_members()
        return [dict(n_moves=int(r["n_moves"]), replicas=int(r["replicas"]), first_move=int(r["first_move"]), moves=m)
                for r, m in zip(self._rounds, members)]

    def reassignment_rounds(self, kinds=None, max_moves: int = 0) -> List[dict]:
        """One Kafka reassignment JSON object per round (rounds=... together with moves=... that holds "replicas"): the partitions
        of moves(kinds=kinds), a replica move in its round, any other move (a leader change, a reorder) in round 0.  max_moves
        > 0: a round of more partitions is split into consecutive objects of at most max_moves (no cap can break by that).  The
        objects' partitions are reassignment(kinds)'s as a set.  Raises when the room was too small."""
        if self._rounds is None:
            raise ValueError(self._NO_ROUNDS)
        if self._moves is None or not self._moves_mask & abi.KAS_MOVE_REPLICAS:
            raise ValueError('reassignment_rounds() needs moves=(...) with "replicas": the rounds index the replica move list')
        if int(max_moves) < 0:
            raise ValueError("max_moves: >= 0 (0 = no bound)")
        self._round_members()
        mask = self._moves_mask if kinds is None else abi.move_mask(kinds)
        per = [[] for _ in range(max(self.n_rounds, 1))]
        i = 0
        for (t, p, reps, _), rec in zip(self.moves(), self._moves[0]):
            flags = int(rec["flags"])
            r = 0
            if flags & abi.KAS_MOVE_REPLICAS:
                r = int(self._round_of[i])
                i += 1
            if flags & mask:
                per[r].append({"topic": t, "partition": p, "replicas": reps})
        out = []
        for parts in per:
            step = int(max_moves) if max_moves else max(len(parts), 1)
            for at in range(0, len(parts), step):
                out.append({"version": 1, "partitions": parts[at:at + step]})
        return out

    def broker_impact(self) -> Dict[int, Dict[str, int]]:
        """broker id -> {replicas_before, replicas_after, leaders_before, leaders_after, inbound, outbound} under this
        variant, over every topic that was solved (solve(..., impact=True))."""
        if self._nodes is None:
            raise ValueError("no impact records: solve with impact=True")
        return {int(b): {f: int(r[f]) for f in abi.NODE_IMPACT_FIELDS} for b, r in zip(self._node_ids, self._nodes)}


    def rack_impact(self) -> Dict[str, Dict[str, int]]:
        """rack name -> {nodes, replicas_before, replicas_after, leaders_before, leaders_after, inbound, outbound} under this
        variant (solve(..., impact=True, racks=True)); a broker without a rack is a rack named by its id."""
        if self._racks is None:
            raise ValueError("no rack records: solve with impact=True, racks=True")
        return {name: {f: int(r[f]) for f in abi.RACK_IMPACT_FIELDS} for name, r in zip(self._rack_names, self._racks)}

    def topic_impact(self) -> Dict[str, Dict[str, int]]:
        """topic name -> {status, moved_replicas, moved_partitions, departed_replicas, leaders_moved, max_inbound, max_outbound,
        min / max_replicas_after, min / max_leaders_after} under this variant (solve(..., topics=True)): the counts over that
        topic's rows only, max and min over every broker of the variant."""
        if self._topics is None:
            raise ValueError("no topic records: solve with topics=True")
        out = {}
        for name, tr, r in zip(self._plan.topic_names, self._topic_results, self._topics):
            rec = {"status": int(tr["status"]), "moved_replicas": int(tr["moved_replicas"]), "moved_partitions": int(tr["moved_partitions"])}
            rec.update({f: int(r[f]) for f in abi.TOPIC_IMPACT_FIELDS})
            out[name] = rec
        return out


class Front(list):
    """What WhatIf.front returns: the members (VariantResult) in member order, and what became of every variant."""
    n_ok = n_eligible = n_front = 0
    classes: List[str] = []


class WhatIf:
    def __init__(self, brokers: Dict[int, Optional[str]], topics: Dict[str, Dict[int, Sequence[int]]],
                 desired_replication_factor: int = -1):
        self.brokers = dict(brokers)
        self.topic_names = list(topics)                                   # KAG:155-157: input order
        self.part_ids, self.widths, self.rfs, tables = [], [], [], []
        for name in self.topic_names:
            cur = topics[name]
            pids = sorted(cur)
            lens = {len(cur[p]) for p in pids}
            rf = desired_replication_factor
            if rf < 0:                                                     # KTA:49-62
                if len(lens) > 1:
                    raise IllegalStateException("Topic " + name + " has partitions with different replication factors")
                rf = lens.pop() if lens else -1
            w = max([len(cur[p]) for p in pids] + [0])
            t = np.full((len(pids), max(w, 1)), -1, dtype=np.int32)
            for i, p in enumerate(pids):
                t[i, :len(cur[p])] = cur[p]
            if any(len(cur[p]) != w for p in pids):
                raise ValueError("what-if tables need uniform replica lists per topic (use flatten() otherwise)")
            self.part_ids.append(np.asarray(pids, dtype=np.int32))
            self.widths.append(w)
            self.rfs.append(rf)
            tables.append(t.reshape(-1))
        self.cur_off = np.concatenate([[0], np.cumsum([t.size for t in tables])[:-1]]).astype(np.int64)
        self.cur = np.concatenate(tables) if tables else np.zeros(1, np.int32)

    # ---- batch construction -----------------------------------------------------------------
    def flat_batch(self, variants: Sequence[Variant]) -> FlatBatch:
        S, T = len(variants), len(self.topic_names)
        scen = np.zeros(S, dtype=abi.SCENARIO_DESC_DTYPE)
        topics = np.zeros(S * T, dtype=abi.TOPIC_DESC_DTYPE)
        node_ids, node_racks, aux = [], [], []
        node_off, out_off, aux_off = 0, 0, 0
        part_off = []
        for pids in self.part_ids:                                         # shared part_id arrays
            part_off.append(aux_off); aux.append(pids); aux_off += pids.size
        for s, v in enumerate(variants):
            live = {b: r for b, r in self.brokers.items() if b not in set(v.remove)}
            live.update(v.add)
            ids = sorted(live)
            index: Dict[str, int] = {}
            racks = []
            for b in ids:                                                  # KAS:82-86
                r = live[b] if (v.rack_aware and live[b] is not None) else str(b)
                racks.append(index.setdefault(r, len(index)))
            scen[s] = (len(ids), s * T, T, 0, node_off, -1)
            node_ids.append(np.asarray(ids, dtype=np.int32)); node_racks.append(np.asarray(racks, dtype=np.int32))
            node_off += len(ids)
            for t, name in enumerate(self.topic_names):
                P, w, rf = self.part_ids[t].size, self.widths[t], self.rfs[t]
                ow = max(w, rf, 1)
                topics[s * T + t] = (java_string_hashcode(name), P, w, rf, ow, 0, int(self.cur_off[t]), out_off,
                                     -1, -1, part_off[t])
                out_off += P * ow
        return FlatBatch(scen=scen, topics=topics,
                         node_id=np.concatenate(node_ids) if S else np.zeros(0, np.int32),
                         node_rack=np.concatenate(node_racks) if S else np.zeros(0, np.int32),
                         cur=self.cur, aux=np.concatenate(aux) if aux else np.zeros(0, np.int32),
                         ctx=np.zeros(0, np.int32), out_len=out_off)

    def report_racks(self, variants: Sequence[Variant]):
        """(table, names): the report rack table of flat_batch(variants) — int32, parallel to its node_rack — built from the REAL
        racks (self.brokers / Variant.add; a None rack -> the broker's id, KAS:82-86) whatever rack_aware says, and per variant
        the rack name of each rack index (indices in order of first appearance over the variant's ascending broker ids)."""
        table, names = [], []
        for v in variants:
            live = {b: r for b, r in self.brokers.items() if b not in set(v.remove)}
            live.update(v.add)
            index: Dict[str, int] = {}
            for b in sorted(live):
                r = live[b] if live[b] is not None else str(b)
                table.append(index.setdefault(r, len(index)))
            names.append(list(index))
        return np.asarray(table, dtype=np.int32), names

    # ---- solve ---------------------------------------------------------------------------------
    def _with_batches(self, fb, results, caps, room: int):
        """the execution batches of `results` (one kas_solve_host_batches call over their variants, which downloads no rows)"""
        if caps is None or not results:
            return results
        from . import native
        _, bl = native.solve_host_batches(fb, caps, select=[r._index for r in results], stride=int(room))
        for j, r in enumerate(results):
            rec = bl.scenarios[j]
            r.n_batches, r.batch_moves, r.batch_replicas = int(rec["n_batches"]), int(rec["n_moves"]), int(rec["replicas"])
            r.max_batch_moves, r.max_batch_replicas = int(rec["max_batch_moves"]), int(rec["max_batch_replicas"])
            r.closed_by_max_moves, r.closed_by_inbound = int(rec["closed_by_max_moves"]), int(rec["closed_by_inbound"])
            r.closed_by_outbound = int(rec["closed_by_outbound"])
            r._batches = bl.of(j)
        return results

    def _with_rounds(self, fb, results, caps, room: int):
        """the packed rounds of `results` (one kas_solve_host_rounds call over their variants, which downloads no rows); the move
        stride is the most moved_partitions of a listed result: every round_of entry comes back"""
        if caps is None or not results:
            return results
        from . import native
        most = max([int(r.moved_partitions) for r in results if r.status == abi.KAS_OK] + [0])
        _, rl = native.solve_host_rounds(fb, caps, select=[r._index for r in results], round_stride=int(room), move_stride=most)
        for j, r in enumerate(results):
            rec = rl.scenarios[j]
            r.n_rounds, r.round_moves, r.round_replicas = int(rec["n_rounds"]), int(rec["n_moves"]), int(rec["replicas"])
            r.max_round_moves, r.max_round_replicas = int(rec["max_round_moves"]), int(rec["max_round_replicas"])
            r.raised_by_inbound, r.raised_by_outbound = int(rec["raised_by_inbound"]), int(rec["raised_by_outbound"])
            r._rounds, r._round_of = rl.of(j), rl.round_of_moves(j)
        return results

    @staticmethod
    def _round_args(rounds, round_room):
        """check rounds= / round_room= before anything is solved"""
        if rounds is None:
            return
        spec = abi.round_spec(rounds)
        if min(spec.cap_inbound, spec.cap_outbound) < 0 or not (spec.cap_inbound or spec.cap_outbound) or spec.policy != abi.KAS_ROUNDS_MONOTONE:
            raise ValueError("rounds: caps are >= 0 (0 = no bound), at least one of inbound, outbound is set, policy is 0")
        if int(round_room) < 0:
            raise ValueError("round_room: room for round records per variant, >= 0")

    @staticmethod
    def _batch_args(batches, batch_room):
        """check batches= / batch_room= before anything is solved"""
        if batches is None:
            return
        spec = abi.batch_spec(batches)
        if min(spec.cap_inbound, spec.cap_outbound, spec.max_moves) < 0 or not (spec.cap_inbound or spec.cap_outbound or spec.max_moves):
            raise ValueError("batches: bounds are >= 0 (0 = no bound) and at least one of inbound, outbound, max_moves is set")
        if int(batch_room) < 0:
            raise ValueError("batch_room: room for batch records per variant, >= 0")

    def solve(self, variants: Sequence[Variant], solve_fn=None, impact: bool = False, rows: bool = True, moves=None,
              racks: bool = False, topics: bool = False, batches=None, batch_room: int = 4096,
              rounds=None, round_room: int = 4096) -> List[VariantResult]:
        """Solve every variant in one batch (default: the HIP path through the C ABI).
        impact=True: also the per-broker impact of every variant, computed on the GPU (kas_solve_host_impact).
        rows=False: no variant's rows come back (kas_solve_host_select / kas_solve_host_impact with n_select = 0) — the
        records and the impact only; assignment() then raises.
        moves=(kinds): the moves of every variant instead of its rows (kas_solve_host_moves: no rows come back whatever `rows`
        says, and the call takes neither impact nor solve_fn); moves() and reassignment() then answer.
        racks=True (needs impact=True): also the rack pass (kas_solve_host_rack_impact) against the real racks (report_racks):
        colocated_after, single_rack_rows_after, ... and rack_impact() then answer.
        topics=True (with or without impact, rows and racks; not with moves or solve_fn): also the topic pass
        (kas_solve_host_topic_impact): topics_moved, max_topic_inbound, max_topic_replica_spread, ... and topic_impact() then
        answer.  Together with racks=True the topic records come from a second host call that downloads no rows.
        batches={"inbound": 5, ...} (abi.batch_spec; not with solve_fn): also every variant's execution batches
        (kas_solve_host_batches): n_batches, max_batch_moves, ... and batches() then answer, and with moves=... as well
        reassignment_batches(); batch_room: batch records kept per variant (n_batches is the true count whatever the room).
        Like the topic records beside racks=True, they come from a second host call that downloads no rows.
        rounds={"inbound": 5, "outbound": 0} (abi.round_spec; not with solve_fn): also every variant's packed rounds
        (kas_solve_host_rounds): n_rounds, max_round_moves, ... and rounds() then answer, and with moves=... holding "replicas"
        reassignment_rounds(); round_room: round records kept per variant.  One more host call that downloads no rows."""
        from . import native
        self._batch_args(batches, batch_room)
        self._round_args(rounds, round_room)
        if batches is not None and solve_fn is not None:
            raise ValueError("batches=... takes the library's own host call (no solve_fn)")
        if rounds is not None and solve_fn is not None:
            raise ValueError("rounds=... takes the library's own host call (no solve_fn)")
        fb = self.flat_batch(variants)
        nodes = scen_imp = ml = rk = rack_names = tp = None
        if topics and (moves is not None or solve_fn is not None):
            raise ValueError("topics=True takes the library's own host call, without moves (no solve_fn)")
        if racks and (not impact or moves is not None):
            raise ValueError("racks=True is a pass behind the impact pass: solve(..., impact=True, racks=True), without moves")
        if moves is not None:
            if solve_fn is not None or impact:
                raise ValueError("moves=... takes the library's own host call, without impact (best() has both)")
            ho, ml = native.solve_host_moves(fb, abi.move_mask(moves))
            rows = False
        elif impact:
            if solve_fn is not None:
                raise ValueError("impact=True takes the library's own host call (no solve_fn)")
            if racks:
                table, rack_names = self.report_racks(variants)
                ho, rk = native.solve_host_rack_impact(fb, report_rack=table, select=None if rows else [])
                nodes, scen_imp = rk.nodes, rk.impact
                if topics:
                    _, tp = native.solve_host_topic_impact(fb, select=[], impact=False)
            elif topics:
                ho, tp = native.solve_host_topic_impact(fb, select=None if rows else [])
                nodes, scen_imp = tp.nodes, tp.impact
            else:
                ho, nodes, scen_imp = native.solve_host_impact(fb, select=None if rows else [])
        elif topics:
            ho, tp = native.solve_host_topic_impact(fb, select=None if rows else [], impact=False)
        elif not rows:
            if solve_fn is not None:
                raise ValueError("rows=False takes the library's own host call (no solve_fn)")
            ho = native.solve_host_select(fb, [])
        else:
            ho = (solve_fn or native.solve_host)(fb)
        self._fb = fb
        base = native.node_blocks(fb)
        res = []
        for s, v in enumerate(variants):
            sr = ho.scenario_results[s]
            ft = int(sr["fail_topic"])
            extra = {}
            if impact:
                extra = {f: int(scen_imp[f][s]) for f in abi.SCENARIO_IMPACT_FIELDS}
                off, n = int(fb.scen["node_off"][s]), int(fb.scen["n_nodes"][s])
                extra.update(_nodes=nodes[base[s]:base[s + 1]], _node_ids=fb.node_id[off:off + n])
            if rk is not None:
                extra.update({f: int(rk.scenarios[f][s]) for f in abi.SCENARIO_RACK_FIELDS})
                extra.update(_racks=rk.of(s), _rack_names=rack_names[s])
            if tp is not None:
                tb, tc = int(fb.scen["topic_begin"][s]), int(fb.scen["topic_count"][s])
                extra.update({f: int(tp.scenarios[f][s]) for f in abi.SCENARIO_TOPIC_FIELDS})
                extra.update(_topics=tp.topics[tb:tb + tc], _topic_results=ho.topic_results[tb:tb + tc])
            if ml is not None:
                extra.update(_moves=ml.of(s), _moves_mask=ml.mask)
            res.append(VariantResult(label=v.label, status=int(sr["status"]),
                                     fail_topic=self.topic_names[ft] if ft >= 0 else None,
                                     fail_partition=int(sr["fail_partition"]),
                                     moved_replicas=int(sr["moved_replicas"]),
                                     moved_partitions=int(sr["moved_partitions"]), digest=int(sr["digest"]),
                                     _plan=self, _index=s, _out=ho.out if rows else None, **extra))
        return self._with_rounds(fb, self._with_batches(fb, res, batches, batch_room), rounds, round_room)

    @staticmethod
    def _criteria(names, racks: bool) -> bool:
        """check criterion names; True when the call takes the rack pass (racks=True, or a rack criterion among the names)"""
        for name in names:
            if name not in abi.KEYS and name not in abi.RACK_KEYS and name not in abi.TOPIC_KEYS:
                raise ValueError("unknown criterion %r (one of %s; rack criteria: %s; topic criteria: %s)" %
                                 (name, ", ".join(abi.KEY_NAMES), ", ".join(abi.RACK_KEY_NAMES), ", ".join(abi.TOPIC_KEY_NAMES)))
        return bool(racks) or any(name in abi.RACK_KEYS for name in names)

    @staticmethod
    def _by_topics(names, topics: bool) -> bool:
        """True when the call takes the topic entries (topics=True, or a topic criterion among the names)"""
        return bool(topics) or any(name in abi.TOPIC_KEYS for name in names)

    def _winner(self, variants, fb, ho, ch, ml, j: int, rows: bool, rk=None, rack_names=None, tp=None) -> VariantResult:
        """chosen[j] of a choice or a front as a VariantResult"""
        s = int(ch.chosen[j])
        sr = ho.scenario_results[s]
        off, n = int(fb.scen["node_off"][s]), int(fb.scen["n_nodes"][s])
        extra = {f: int(ch.scenarios[f][s]) for f in abi.SCENARIO_IMPACT_FIELDS}
        if ml is not None:
            extra.update(_moves=ml.of(j), _moves_mask=ml.mask)
        if rk is not None:
            extra.update({f: int(rk.scenarios[f][s]) for f in abi.SCENARIO_RACK_FIELDS})
            extra.update(_racks=rk.of(s), _rack_names=rack_names[s])
        if tp is not None:
            tb, tc = int(fb.scen["topic_begin"][s]), int(fb.scen["topic_count"][s])
            extra.update({f: int(tp.scenarios[f][s]) for f in abi.SCENARIO_TOPIC_FIELDS})
            extra.update(_topics=tp.topics[tb:tb + tc], _topic_results=ho.topic_results[tb:tb + tc])
        return VariantResult(label=variants[s].label, status=int(sr["status"]), fail_topic=None,
                             fail_partition=int(sr["fail_partition"]), moved_replicas=int(sr["moved_replicas"]),
                             moved_partitions=int(sr["moved_partitions"]), digest=int(sr["digest"]), rank=j,
                             _plan=self, _index=s, _out=ch.rows if rows else None, _packed_at=int(ch.row_off[j]),
                             _nodes=ch.nodes[int(ch.node_off[j]):int(ch.node_off[j + 1])], _node_ids=fb.node_id[off:off + n],
                             **extra)

    def best(self, variants: Sequence[Variant], k: int = 1, by: Sequence[str] = ("moved_replicas", "leaders_moved"), moves=None,
             rows: bool = True, racks: bool = False, topics: bool = False, batches=None, batch_room: int = 4096,
              rounds=None, round_room: int = 4096) -> List[VariantResult]:
        """The k best variants that solve, best first, chosen on the GPU (kas_solve_host_choose): variants are compared by the
        criteria named in `by` (abi.KEY_NAMES; one to four, smaller is better, the earlier variant wins a tie).  Every variant is
        solved and reduced to its records, but rows and per-broker impact come back for the winners only: each result has
        assignment(), broker_impact() and its rank.  Fewer than k results when fewer variants solve.
        moves=(kinds): also each winner's moves (kas_solve_host_choose_moves; moves(), reassignment()); with rows=False no rows
        are fetched and assignment() raises.
        A rack criterion in `by` (abi.RACK_KEY_NAMES), or racks=True, adds the rack pass against the real racks (report_racks)
        and ranks on its records too (kas_solve_host_choose_racks): each winner then also has the rack figures and rack_impact().
        A topic criterion in `by` (abi.TOPIC_KEY_NAMES), or topics=True, adds the topic pass and ranks on its records too
        (kas_solve_host_choose_topics, with the rack pass when a rack criterion is named or racks=True): each winner then also
        has the topic figures and topic_impact().
        batches={"inbound": 5, ...}: also each winner's execution batches (n_batches, ..., batches(), and with moves=...
        reassignment_batches()), fetched with one kas_solve_host_batches call over the chosen: a second host call that downloads
        no rows, as the topic records beside racks=True in solve().
        rounds={"inbound": 5, ...}: also each winner's packed rounds (n_rounds, ..., rounds(), reassignment_rounds()), fetched the
        same way with one kas_solve_host_rounds call over the chosen."""
        from . import native
        self._batch_args(batches, batch_room)
        self._round_args(rounds, round_room)
        by = [by] if isinstance(by, str) else list(by)
        by_racks = self._criteria(by, racks)
        by_topics = self._by_topics(by, topics)
        if not 1 <= len(by) <= abi.KAS_CHOOSE_MAX_KEYS:
            raise ValueError("by: one to four criteria")
        fb = self.flat_batch(variants)
        k = max(0, min(int(k), len(variants)))
        ml = None
        if by_topics:
            if moves is None and not rows:
                raise ValueError("rows=False needs moves=...: a winner without rows and without moves has nothing to act on")
            table, rack_names = self.report_racks(variants) if by_racks else (None, None)
            ho, ch, ml, rk, tp = native.solve_host_choose_topics(fb, by, k, racks=by_racks, report_rack=table, rows=rows,
                                                                 mask=None if moves is None else abi.move_mask(moves))
            self._fb = fb
            return self._with_rounds(fb, self._with_batches(fb, [self._winner(variants, fb, ho, ch, ml, j, rows, rk, rack_names, tp) for j in range(min(k, ch.n_ok))], batches, batch_room), rounds, round_room)
        if by_racks:
            if moves is None and not rows:
                raise ValueError("rows=False needs moves=...: a winner without rows and without moves has nothing to act on")
            table, rack_names = self.report_racks(variants)
            ho, ch, ml, rk = native.solve_host_choose_racks(fb, by, k, report_rack=table, rows=rows,
                                                            mask=None if moves is None else abi.move_mask(moves))
            self._fb = fb
            return self._with_rounds(fb, self._with_batches(fb, [self._winner(variants, fb, ho, ch, ml, j, rows, rk, rack_names) for j in range(min(k, ch.n_ok))], batches, batch_room), rounds, round_room)
        if moves is None:
            if not rows:
                raise ValueError("rows=False needs moves=...: a winner without rows and without moves has nothing to act on")
            ho, ch = native.solve_host_choose(fb, by, k)
        else:
            ho, ch, ml = native.solve_host_choose_moves(fb, by, k, abi.move_mask(moves), rows=rows)
        self._fb = fb
        res = []
        for j in range(min(k, ch.n_ok)):
            s = int(ch.chosen[j])
            sr = ho.scenario_results[s]
            off, n = int(fb.scen["node_off"][s]), int(fb.scen["n_nodes"][s])
            extra = {f: int(ch.scenarios[f][s]) for f in abi.SCENARIO_IMPACT_FIELDS}
            if ml is not None:
                extra.update(_moves=ml.of(j), _moves_mask=ml.mask)
            res.append(VariantResult(label=variants[s].label, status=int(sr["status"]), fail_topic=None,
                                     fail_partition=int(sr["fail_partition"]), moved_replicas=int(sr["moved_replicas"]),
                                     moved_partitions=int(sr["moved_partitions"]), digest=int(sr["digest"]), rank=j,
                                     _plan=self, _index=s, _out=ch.rows if rows else None, _packed_at=int(ch.row_off[j]),
                                     _nodes=ch.nodes[int(ch.node_off[j]):int(ch.node_off[j + 1])], _node_ids=fb.node_id[off:off + n],
                                     **extra))
        return self._with_rounds(fb, self._with_batches(fb, res, batches, batch_room), rounds, round_room)

    def front(self, variants: Sequence[Variant], by: Sequence[str] = ("moved_replicas", "replica_spread"), within=None, k: int = 16,
              moves=None, rows: bool = True, racks: bool = False, topics: bool = False, batches=None, batch_room: int = 4096,
              rounds=None, round_room: int = 4096) -> "Front":
        """The Pareto front of the variants, marked and ranked on the GPU (kas_solve_host_front): every variant that solves,
        respects the hard bounds in `within` ({criterion: limit}, e.g. {"max_inbound": 200}) and is beaten by no other such
        variant on all the criteria in `by` at once (abi.KEY_NAMES; one to four, smaller is better; of variants with identical
        criteria the earliest survives).  Up to k members come back in the order best() would give them, each with
        assignment(), broker_impact(), its rank and — with moves=(kinds) — moves(); rows=False fetches no rows.  The list also
        carries n_ok, n_eligible, n_front (> len when k cut it) and classes: per variant "member", "dominated", "over_limit"
        or "failed".
        A rack criterion in `by` or `within` (abi.RACK_KEY_NAMES), or racks=True, adds the rack pass against the real racks and
        marks and ranks on its records too (kas_solve_host_front_racks): members then also have the rack figures and rack_impact().
        A topic criterion in `by` or `within` (abi.TOPIC_KEY_NAMES), or topics=True, adds the topic pass and marks and ranks on
        its records too (kas_solve_host_front_topics): members then also have the topic figures and topic_impact().
        batches={"inbound": 5, ...}: also each member's execution batches, as in best(): one kas_solve_host_batches call over the
        members, a second host call that downloads no rows.
        rounds={"inbound": 5, ...}: also each member's packed rounds, as in best()."""
        from . import native
        self._batch_args(batches, batch_room)
        self._round_args(rounds, round_room)
        by = [by] if isinstance(by, str) else list(by)
        within = dict(within or {})
        by_racks = self._criteria(by + list(within), racks)
        by_topics = self._by_topics(by + list(within), topics)
        if not 1 <= len(by) <= abi.KAS_CHOOSE_MAX_KEYS:
            raise ValueError("by: one to four criteria")
        if len(within) > abi.KAS_CHOOSE_MAX_KEYS or any(int(v) < 0 for v in within.values()):
            raise ValueError("within: at most four bounds, none negative")
        fb = self.flat_batch(variants)
        k = max(0, min(int(k), len(variants)))
        rk = rack_names = tp = None
        if by_topics:
            table, rack_names = self.report_racks(variants) if by_racks else (None, None)
            ho, ch, ml, rk, tp = native.solve_host_front_topics(fb, abi.topic_front_spec(by, within, k), racks=by_racks, report_rack=table,
                                                                rows=rows, mask=None if moves is None else abi.move_mask(moves))
        elif by_racks:
            table, rack_names = self.report_racks(variants)
            ho, ch, ml, rk = native.solve_host_front_racks(fb, abi.rack_front_spec(by, within, k), report_rack=table, rows=rows,
                                                           mask=None if moves is None else abi.move_mask(moves))
        else:
            ho, ch, ml = native.solve_host_front(fb, abi.front_spec(by, within, k), None if moves is None else abi.move_mask(moves), rows=rows)
        self._fb = fb
        res = Front()
        res.n_ok, res.n_eligible, res.n_front = ch.n_ok, ch.n_eligible, ch.n_front
        res.classes = [abi.FRONT_CLASSES[min(int(r), 0)] for r in ch.rank]
        if by_racks or by_topics:
            res.extend(self._winner(variants, fb, ho, ch, ml, j, rows, rk, rack_names, tp) for j in range(min(k, ch.n_front)))
            return self._with_rounds(fb, self._with_batches(fb, res, batches, batch_room), rounds, round_room)
        for j in range(min(k, ch.n_front)):
            s = int(ch.chosen[j])
            sr = ho.scenario_results[s]
            off, n = int(fb.scen["node_off"][s]), int(fb.scen["n_nodes"][s])
            extra = {f: int(ch.scenarios[f][s]) for f in abi.SCENARIO_IMPACT_FIELDS}
            if ml is not None:
                extra.update(_moves=ml.of(j), _moves_mask=ml.mask)
            res.append(VariantResult(label=variants[s].label, status=int(sr["status"]), fail_topic=None,
                                     fail_partition=int(sr["fail_partition"]), moved_replicas=int(sr["moved_replicas"]),
                                     moved_partitions=int(sr["moved_partitions"]), digest=int(sr["digest"]), rank=j,
                                     _plan=self, _index=s, _out=ch.rows if rows else None, _packed_at=int(ch.row_off[j]),
                                     _nodes=ch.nodes[int(ch.node_off[j]):int(ch.node_off[j + 1])], _node_ids=fb.node_id[off:off + n],
                                     **extra))
        return self._with_rounds(fb, self._with_batches(fb, res, batches, batch_room), rounds, round_room)

    def _rows(self, s: int, topic: str, out: np.ndarray, packed_at: Optional[int] = None) -> Dict[int, List[int]]:
        t = self.topic_names.index(topic)
        td = self._fb.topics[s * len(self.topic_names) + t]
        P, ow, off = int(td["n_partitions"]), int(td["out_width"]), int(td["out_off"])
        if packed_at is not None:                                          # (a scenario's topics are laid out back to back)
            off = packed_at + off - int(self._fb.topics[s * len(self.topic_names)]["out_off"])
        rows = out[off:off + P * ow].reshape(P, ow)
        return {int(p): [int(b) for b in rows[i] if b >= 0] for i, p in enumerate(self.part_ids[t])
                if (rows[i] >= 0).any()}

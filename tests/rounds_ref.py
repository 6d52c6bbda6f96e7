"""Plain-Python restatement of the packed rounds (include/kas_abi.h: kas_round_spec / kas_move_round / kas_scenario_rounds) over a
FlatBatch and the HostOutputs of a solve with every row in place.  The checker of tests/test_rounds_*.py, written from the header's
text, not a product path.

The moves of a scenario, In(i) and Out(i) are those of the batches checker (batches_ref.scenario_moves).  monotone() is the
header's loop, word for word; first_fit() is a true first fit over all rounds (a counter per (round, node)) and lower_bound() is
ceil(max per-node total / cap): what the loop is measured against, neither is a product path.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from batches_ref import scenario_moves
from kafka_assigner_amd import abi

WINDOW = 1024                           # KAS_ROUND_WINDOW (kas_rounds.h): rounds whose counters the kernel holds at a time
ITEM_ROWS = 1024                        # KAS_MOVES_ITEM_ROWS: rows of a tile, and the entries of the kernel's queue


def spec_of(caps) -> SimpleNamespace:
    """(inbound, outbound) from a dict or an abi.RoundSpec"""
    if isinstance(caps, abi.RoundSpec):
        return SimpleNamespace(inbound=caps.cap_inbound, outbound=caps.cap_outbound)
    return SimpleNamespace(inbound=int(caps.get("inbound", 0)), outbound=int(caps.get("outbound", 0)))


def monotone(moves, caps):
    """The header's loop over a move list: (round_of list, raised_by_inbound, raised_by_outbound)"""
    sp = spec_of(caps)
    rin, uin, rout, uout = {}, {}, {}, {}
    round_of = []
    by_in = by_out = 0
    for _, _, In, Out in moves:
        r_in = r_out = 0
        if sp.inbound:
            for b in In:
                r_in = max(r_in, rin.get(b, 0) if uin.get(b, 0) < sp.inbound else rin.get(b, 0) + 1)
        if sp.outbound:
            for b in Out:
                r_out = max(r_out, rout.get(b, 0) if uout.get(b, 0) < sp.outbound else rout.get(b, 0) + 1)
        r = max(r_in, r_out)
        round_of.append(r)
        if r > 0 and r_in == r:
            by_in += 1
        elif r > 0:
            by_out += 1
        if sp.inbound:
            for b in In:
                if rin.get(b, 0) == r:
                    uin[b] = uin.get(b, 0) + 1
                else:
                    rin[b], uin[b] = r, 1
        if sp.outbound:
            for b in Out:
                if rout.get(b, 0) == r:
                    uout[b] = uout.get(b, 0) + 1
                else:
                    rout[b], uout[b] = r, 1
    return round_of, by_in, by_out


def first_fit(moves, caps):
    """True first fit: every move goes into the lowest round in which each of its nodes still has room.  round_of list."""
    sp = spec_of(caps)
    cin, cout = [], []                  # per round: {node: moves}
    round_of = []
    for _, _, In, Out in moves:
        r = 0
        while True:
            if r == len(cin):
                cin.append({})
                cout.append({})
            if (not sp.inbound or all(cin[r].get(b, 0) < sp.inbound for b in In)) and \
               (not sp.outbound or all(cout[r].get(b, 0) < sp.outbound for b in Out)):
                break
            r += 1
        for b in In:
            cin[r][b] = cin[r].get(b, 0) + 1
        for b in Out:
            cout[r][b] = cout[r].get(b, 0) + 1
        round_of.append(r)
    return round_of


def lower_bound(moves, caps) -> int:
    """ceil(max per-node total / cap) over the capped directions; 1 for a list whose moves name no capped node, 0 without moves"""
    sp = spec_of(caps)
    if not moves:
        return 0
    tin, tout = {}, {}
    for _, _, In, Out in moves:
        for b in In:
            tin[b] = tin.get(b, 0) + 1
        for b in Out:
            tout[b] = tout.get(b, 0) + 1
    lb = 1
    if sp.inbound and tin:
        lb = max(lb, -(-max(tin.values()) // sp.inbound))
    if sp.outbound and tout:
        lb = max(lb, -(-max(tout.values()) // sp.outbound))
    return lb


def records(moves, round_of, by_in=0, by_out=0):
    """(scenario record dict, [round record dicts]) of an assignment of rounds to a move list"""
    n = 1 + max(round_of) if round_of else 0
    rounds = [dict(n_moves=0, replicas=0, first_move=-1, reserved=0) for _ in range(n)]
    for i, (r, m) in enumerate(zip(round_of, moves)):
        rec = rounds[r]
        rec["n_moves"] += 1
        rec["replicas"] += len(m[2])
        if rec["first_move"] < 0:
            rec["first_move"] = i
    rec = dict(n_rounds=n, n_moves=len(moves), replicas=sum(len(m[2]) for m in moves),
               max_round_moves=max((r["n_moves"] for r in rounds), default=0),
               max_round_replicas=max((r["replicas"] for r in rounds), default=0),
               raised_by_inbound=by_in, raised_by_outbound=by_out, reserved=0)
    return rec, rounds


def rounds_ref(fb, ho, select, caps, cells16: bool = False, cur16=None):
    """Per listed scenario (None for an empty slot): SimpleNamespace(record, rounds, round_of, moves).  Scenarios listed twice are
    scheduled once."""
    done = {}
    out = []
    for s in [int(x) for x in select]:
        if not 0 <= s < fb.n_scenarios:
            out.append(None)
            continue
        if s not in done:
            mv = scenario_moves(fb, ho, s, cells16, cur16)
            ro, by_in, by_out = monotone(mv, caps)
            rec, rd = records(mv, ro, by_in, by_out)
            done[s] = SimpleNamespace(record=rec, rounds=rd, round_of=ro, moves=mv)
        out.append(done[s])
    return out


def check_caps(moves, round_of, caps, what=""):
    """in every round no node is in In() of more than cap_inbound moves nor in Out() of more than cap_outbound"""
    sp = spec_of(caps)
    cin, cout = {}, {}
    for r, (_, _, In, Out) in zip(round_of, moves):
        for b in In:
            cin[(r, b)] = cin.get((r, b), 0) + 1
        for b in Out:
            cout[(r, b)] = cout.get((r, b), 0) + 1
    assert not sp.inbound or max(cin.values(), default=0) <= sp.inbound, (what, "inbound cap broken")
    assert not sp.outbound or max(cout.values(), default=0) <= sp.outbound, (what, "outbound cap broken")


def check_invariants(want, caps, moved_partitions=None, moved_replicas=None, what=""):
    """The invariants of one scenario's schedule: the caps hold in every round, the counts add up (to the solve's scenario
    record where given), every round below n_rounds holds a move and first_move is its lowest index, and the schedule is no
    better than the lower bound and no worse than one move a round."""
    rec, rd, ro, mv = want.record, want.rounds, want.round_of, want.moves
    check_caps(mv, ro, caps, what)
    assert sum(r["n_moves"] for r in rd) == len(mv) == rec["n_moves"], what
    if moved_partitions is not None:
        assert rec["n_moves"] == int(moved_partitions), (what, rec["n_moves"], moved_partitions)
    if moved_replicas is not None:
        assert rec["replicas"] == int(moved_replicas), (what, rec["replicas"], moved_replicas)
    assert sum(r["replicas"] for r in rd) == rec["replicas"], what
    for k, r in enumerate(rd):
        assert r["n_moves"] >= 1 and ro[r["first_move"]] == k and k not in ro[:r["first_move"]], (what, k, r)
    assert lower_bound(mv, caps) <= rec["n_rounds"] <= len(mv), what
    assert rec["raised_by_inbound"] + rec["raised_by_outbound"] == sum(1 for r in ro if r > 0), what


def assert_same_rounds(want, scen, recs, round_stride: int, round_of, move_stride: int, fill=None, what=""):
    """The arrays a call left (scen: abi.SCENARIO_ROUNDS_DTYPE [n], recs: abi.MOVE_ROUND_DTYPE [n * round_stride], round_of: int32
    [n * move_stride]) against rounds_ref's list; with `fill` (the int32 word the arrays held before), everything at or beyond the
    written prefixes must still hold it."""
    assert len(want) == scen.size, what
    for j, w in enumerate(want):
        rec = w.record if w is not None else {f: 0 for f in abi.SCENARIO_ROUNDS_FIELDS}
        got = {f: int(scen[f][j]) for f in abi.SCENARIO_ROUNDS_FIELDS}
        assert got == rec, (what, "scenario record", j, got, rec)
        n = min(rec["n_rounds"], round_stride)
        for i in range(n):
            g = {f: int(recs[f][j * round_stride + i]) for f in abi.MOVE_ROUND_FIELDS}
            assert g == w.rounds[i], (what, "listed", j, "round", i, g, w.rounds[i])
        m = min(rec["n_moves"], move_stride)
        if m:
            got_of = round_of[j * move_stride:j * move_stride + m]
            assert got_of.tolist() == w.round_of[:m], (what, "listed", j, "round_of")
        if fill is not None:
            fill32 = np.array([fill], np.uint32).view(np.int32)[0]
            if round_stride > n:
                rest = recs[j * round_stride + n:(j + 1) * round_stride].view(np.int32)
                assert (rest == fill32).all(), (what, "round records beyond the written ones were touched", j)
            if move_stride > m:
                rest = round_of[j * move_stride + m:(j + 1) * move_stride]
                assert (rest == fill32).all(), (what, "round_of beyond the written prefix was touched", j)

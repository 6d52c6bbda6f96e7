"""Plain-Python restatement of the execution batches (include/kas_abi.h: kas_batch_spec / kas_move_batch / kas_scenario_batches) over a
FlatBatch and the HostOutputs of a solve with every row in place.  The checker of tests/test_batches_*.py, written from the
header's text, not a product path.

The moves of a scenario are its rows with the KAS_MOVE_REPLICAS flag over its KAS_OK topics, in (topic, row) order (moves_ref's
list under that mask).  In(i) = the nodes named by cells of O not in C, Out(i) = the nodes named by cells of C not in O; a cell that
names no node of the scenario is in neither.  cut() is the header's loop, word for word.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from kafka_assigner_amd import abi
from moves_ref import REPLICAS, topic_rows

END, MAX_MOVES, INBOUND, OUTBOUND = abi.KAS_BATCH_END_OF_LIST, abi.KAS_BATCH_MAX_MOVES, abi.KAS_BATCH_INBOUND, abi.KAS_BATCH_OUTBOUND
GROUP = 256                             # KAS_BATCH_GROUP (kas_batches.h): moves the kernel tries at once
ITEM_ROWS = 1024                        # KAS_MOVES_ITEM_ROWS: rows of a tile


def spec_of(caps) -> SimpleNamespace:
    """(inbound, outbound, max_moves) from a dict or an abi.BatchSpec"""
    if isinstance(caps, abi.BatchSpec):
        return SimpleNamespace(inbound=caps.cap_inbound, outbound=caps.cap_outbound, max_moves=caps.max_moves)
    return SimpleNamespace(inbound=int(caps.get("inbound", 0)), outbound=int(caps.get("outbound", 0)), max_moves=int(caps.get("max_moves", 0)))


def scenario_moves(fb, ho, s: int, cells16: bool = False, cur16=None):
    """[(topic within the scenario, partition, In, Out)] of scenario s: its REPLICAS moves in list order, In / Out as sorted tuples of
    node indices"""
    if cells16 and cur16 is None:
        from kafka_assigner_amd.flatten import to_cells16
        cur16 = to_cells16(fb)
    N, off = max(int(fb.scen["n_nodes"][s]), 0), int(fb.scen["node_off"][s])
    if cells16:
        node = lambda v: int(v) if 0 <= int(v) < N else None          # (KAS_CELL16_NONE is no index)
    else:
        index = {int(b): i for i, b in enumerate(fb.node_id[off:off + N])}
        node = lambda v: index.get(int(v))
    b, c = int(fb.scen["topic_begin"][s]), max(int(fb.scen["topic_count"][s]), 0)
    cur = cur16 if cells16 else fb.cur
    out = []
    for k in range(c):
        t = b + k
        if int(ho.topic_results["status"][t]) != abi.KAS_OK:
            continue
        flags, olen, _, _, O, part = topic_rows(fb, ho, t, cells16, cur16)
        td = fb.topics[t]
        P, cw, co, lo = max(int(td["n_partitions"]), 0), int(td["cur_width"]), int(td["cur_off"]), int(td["cur_len_off"])
        Cc = cur[co:co + P * cw].astype(np.int64).reshape(P, cw)
        clen = np.clip(fb.aux[lo:lo + P].astype(np.int64), 0, cw) if lo >= 0 else np.full(P, cw, dtype=np.int64)
        for p in np.nonzero((flags & REPLICAS) != 0)[0]:
            Cs, Os = [int(v) for v in Cc[p, :clen[p]]], [int(v) for v in O[p, :olen[p]]]
            In = sorted({node(v) for v in Os if v not in Cs} - {None})
            Out = sorted({node(v) for v in Cs if v not in Os} - {None})
            out.append((k, int(part[p]), tuple(In), tuple(Out)))
    return out


def cut(moves, caps):
    """The header's loop over a move list: (scenario record dict, [batch record dicts])"""
    sp = spec_of(caps)
    batches = []
    cur = None
    cin, cout = {}, {}

    def emit(why):
        cur["max_inbound"] = max(cin.values(), default=0)
        cur["max_outbound"] = max(cout.values(), default=0)
        cur["closed_by"] = why
        batches.append(cur)

    for i, (topic, part, In, Out) in enumerate(moves):
        why = 0
        if cur is not None:
            if sp.max_moves and cur["n_moves"] == sp.max_moves:
                why = MAX_MOVES
            elif sp.inbound and any(cin.get(b, 0) == sp.inbound for b in In):
                why = INBOUND
            elif sp.outbound and any(cout.get(b, 0) == sp.outbound for b in Out):
                why = OUTBOUND
        if why:
            emit(why)
            cur, cin, cout = None, {}, {}
        if cur is None:
            cur = dict(first_move=i, n_moves=0, topic=topic, partition=part, replicas=0)
        cur["n_moves"] += 1
        cur["replicas"] += len(In)
        for b in In:
            cin[b] = cin.get(b, 0) + 1
        for b in Out:
            cout[b] = cout.get(b, 0) + 1
    if cur is not None:
        emit(END)
    rec = dict(n_batches=len(batches), n_moves=sum(b["n_moves"] for b in batches), replicas=sum(b["replicas"] for b in batches),
               max_batch_moves=max((b["n_moves"] for b in batches), default=0),
               max_batch_replicas=max((b["replicas"] for b in batches), default=0),
               closed_by_max_moves=sum(b["closed_by"] == MAX_MOVES for b in batches),
               closed_by_inbound=sum(b["closed_by"] == INBOUND for b in batches),
               closed_by_outbound=sum(b["closed_by"] == OUTBOUND for b in batches))
    return rec, batches


def replay(moves, caps, group: int = GROUP):
    """How the kernel's optimistic groups fare on a move list: consecutive groups of `group` moves; a group passes clean iff the loop
    closes no batch at one of its moves (counts only grow within a batch, so a group fits as a whole iff each of its prefixes
    does).  Returns SimpleNamespace(clean, replayed, most_closes): groups of either kind, the most closes inside one group."""
    _, batches = cut(moves, caps)
    closes = np.zeros(max(-(-len(moves) // group), 0), np.int64)
    for b in batches[1:]:                                   # a batch that is not the first begins where the one before was closed
        closes[b["first_move"] // group] += 1
    return SimpleNamespace(clean=int((closes == 0).sum()), replayed=int((closes > 0).sum()), most_closes=int(closes.max()) if closes.size else 0,
                           groups=int(closes.size))


def batches_ref(fb, ho, select, caps, cells16: bool = False, cur16=None):
    """Per listed scenario (None for an empty slot): SimpleNamespace(record, batches, moves).  Scenarios listed twice are cut once."""
    done = {}
    out = []
    for s in [int(x) for x in select]:
        if not 0 <= s < fb.n_scenarios:
            out.append(None)
            continue
        if s not in done:
            mv = scenario_moves(fb, ho, s, cells16, cur16)
            rec, bt = cut(mv, caps)
            done[s] = SimpleNamespace(record=rec, batches=bt, moves=mv)
        out.append(done[s])
    return out


def check_invariants(want, caps, moved_partitions=None, moved_replicas=None, what=""):
    """The invariants of one scenario's cut: the counts add up (to the solve's scenario record where given), every batch is
    within the caps, the first_move values tile the list, (topic, partition) are those of the list's record at first_move."""
    sp = spec_of(caps)
    rec, bt, mv = want.record, want.batches, want.moves
    assert sum(b["n_moves"] for b in bt) == len(mv) == rec["n_moves"], what
    if moved_partitions is not None:
        assert rec["n_moves"] == int(moved_partitions), (what, rec["n_moves"], moved_partitions)
    if moved_replicas is not None:
        assert rec["replicas"] == int(moved_replicas), (what, rec["replicas"], moved_replicas)
    at = 0
    for b in bt:
        assert b["first_move"] == at and b["n_moves"] >= 1, (what, b)
        assert (b["topic"], b["partition"]) == mv[at][:2], (what, b)
        assert not sp.max_moves or b["n_moves"] <= sp.max_moves, (what, b)
        assert not sp.inbound or b["max_inbound"] <= sp.inbound, (what, b)
        assert not sp.outbound or b["max_outbound"] <= sp.outbound, (what, b)
        at += b["n_moves"]
    assert at == len(mv), what


def assert_same_batches(want, scen, recs, stride: int, fill=None, what=""):
    """The arrays a call left (scen: abi.SCENARIO_BATCHES_DTYPE [n], recs: abi.MOVE_BATCH_DTYPE [n * stride]) against batches_ref's
    list; with `fill` (the int32 word the arrays held before), records at or beyond min(n_batches, stride) must still hold it."""
    assert len(want) == scen.size, what
    for j, w in enumerate(want):
        rec = w.record if w is not None else {f: 0 for f in abi.SCENARIO_BATCHES_FIELDS}
        got = {f: int(scen[f][j]) for f in abi.SCENARIO_BATCHES_FIELDS}
        assert got == rec, (what, "scenario record", j, got, rec)
        n = min(rec["n_batches"], stride)
        for i in range(n):
            g = {f: int(recs[f][j * stride + i]) for f in abi.MOVE_BATCH_FIELDS}
            assert g == w.batches[i], (what, "listed", j, "batch", i, g, w.batches[i])
        if fill is not None and stride > n:
            rest = recs[j * stride + n:(j + 1) * stride].view(np.int32)
            assert (rest == fill).all(), (what, "records beyond the written ones were touched", j)

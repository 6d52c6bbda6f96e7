"""NumPy / Python restatement of the topic pass's records (include/kas_abi.h: kas_topic_impact / kas_scenario_topic_impact) over a
FlatBatch and the HostOutputs of a solve with every row in place.  The checker of tests/test_topics_*.py, not a product path;
written from the header's definitions.

For each topic whose status is KAS_OK, in a scenario with nodes, and each row p of it: C = the first clen cells of cur[p]
(clen = cur_len[p], or cur_width), O = the cells of out[p] up to the first pad.  Per node b of the scenario, over THIS topic's
rows: replicas_after = cells of O naming b, leaders_after = rows whose O[0] is b, inbound = cells of O naming b that are not in
C, outbound = cells of C naming b that are not in O.  The topic's record: departed_replicas = cells of C that name no node,
leaders_moved = rows with olen > 0 and (clen == 0 or O[0] != C[0]), and max / min of the four per-node counts over ALL nodes of
the scenario (a node without a cell of the topic counts 0).  Any other topic: zeros.  The scenario's record: sixteen words over
its KAS_OK topics, as the header's table says.
"""
from __future__ import annotations

import numpy as np

from kafka_assigner_amd import abi


def _owner(fb):
    owner = np.full(fb.n_topics, -1, dtype=np.int64)
    for s in range(fb.n_scenarios):
        b, c = int(fb.scen["topic_begin"][s]), int(fb.scen["topic_count"][s])
        owner[b:b + c] = s
    return owner


def _rows(fb, ho, t, cells16, cur16):
    """(C, clen, O) of topic t as Python lists per row: C cut to clen, O cut at the first pad"""
    td = fb.topics[t]
    P, cw, ow = int(td["n_partitions"]), int(td["cur_width"]), int(td["out_width"])
    co, oo, lo = int(td["cur_off"]), int(td["out_off"]), int(td["cur_len_off"])
    cur = cur16 if cells16 else fb.cur
    pad = abi.KAS_CELL16_NONE if cells16 else -1
    C = cur[co:co + P * cw].astype(np.int64).reshape(P, cw)
    O = ho.out[oo:oo + P * ow].astype(np.int64).reshape(P, ow)
    clen = np.clip(fb.aux[lo:lo + P].astype(np.int64), 0, cw) if lo >= 0 else np.full(P, cw, dtype=np.int64)
    rows = []
    for p in range(P):
        c = C[p, :int(clen[p])].tolist()
        o = []
        for v in O[p].tolist():
            if v == pad:
                break
            o.append(v)
        rows.append((c, o))
    return rows


def topic_ref(fb, ho, cells16: bool = False, cur16=None):
    """(topics TOPIC_IMPACT_DTYPE [T], scenarios SCENARIO_TOPIC_IMPACT_DTYPE [S]) for `fb` solved into `ho` (every row in place).
    cells16: ho.out holds uint16 node indices and the cur cells are `cur16` (flatten.to_cells16(fb) by default)."""
    if cells16 and cur16 is None:
        from kafka_assigner_amd.flatten import to_cells16
        cur16 = to_cells16(fb)
    T, S = fb.n_topics, fb.n_scenarios
    topics = np.zeros(T, dtype=abi.TOPIC_IMPACT_DTYPE)
    scen = np.zeros(S, dtype=abi.SCENARIO_TOPIC_IMPACT_DTYPE)
    owner = _owner(fb)
    status = ho.topic_results["status"]
    for t in range(T):
        s = int(owner[t])
        if s < 0 or int(status[t]) != abi.KAS_OK:
            continue
        N, off = max(int(fb.scen["n_nodes"][s]), 0), int(fb.scen["node_off"][s])
        if N == 0:
            continue
        if cells16:
            index = {i: i for i in range(N)}
        else:
            index = {int(b): i for i, b in enumerate(fb.node_id[off:off + N])}
        k = np.zeros((N, 4), dtype=np.int64)          # replicas after, leaders after, inbound, outbound
        departed = moved = 0
        for c, o in _rows(fb, ho, t, cells16, cur16):
            for j, v in enumerate(o):
                n = index.get(v)
                if n is not None:
                    k[n, 0] += 1
                    k[n, 1] += j == 0
                    k[n, 2] += v not in c
            for v in c:
                n = index.get(v)
                if n is None:
                    departed += 1
                else:
                    k[n, 3] += v not in o
            moved += bool(o) and (not c or o[0] != c[0])
        topics[t] = (departed, moved, k[:, 2].max(), k[:, 3].max(), k[:, 0].min(), k[:, 0].max(), k[:, 1].min(), k[:, 1].max())
    tr = ho.topic_results
    for s in range(S):
        mine = [t for t in np.nonzero(owner == s)[0] if int(status[t]) == abi.KAS_OK]
        if not mine:
            continue
        r = topics[mine]
        rs = r["max_replicas_after"].astype(np.int64) - r["min_replicas_after"]
        ls = r["max_leaders_after"].astype(np.int64) - r["min_leaders_after"]
        scen[s] = (len(mine), int((tr["moved_replicas"][mine] > 0).sum()), int((r["leaders_moved"] > 0).sum()),
                   int((r["departed_replicas"] > 0).sum()), int(tr["moved_replicas"][mine].max()), int(tr["moved_partitions"][mine].max()),
                   int(r["leaders_moved"].max()), int(r["max_inbound"].max()), int(r["max_outbound"].max()), int(rs.max()), int(ls.max()),
                   int(r["max_replicas_after"].max()), int(r["max_leaders_after"].max()), int(rs.sum()), int(ls.sum()), 0)
    return topics, scen


def assert_same_topics(want, got, what: str = ""):
    """Field by field equality of two (topics, scenarios) pairs, with the first difference in the message."""
    wt, ws = want
    gt, gs = got
    assert wt.shape == gt.shape and ws.shape == gs.shape, (what, wt.shape, gt.shape, ws.shape, gs.shape)
    for f in abi.TOPIC_IMPACT_FIELDS:
        bad = np.nonzero(wt[f] != gt[f])[0]
        assert bad.size == 0, f"{what}: topic {bad[0]} field {f}: want {wt[f][bad[0]]}, got {gt[f][bad[0]]}"
    for f in abi.SCENARIO_TOPIC_FIELDS + ("reserved",):
        bad = np.nonzero(ws[f] != gs[f])[0]
        assert bad.size == 0, f"{what}: scenario {bad[0]} field {f}: want {ws[f][bad[0]]}, got {gs[f][bad[0]]}"


def check_topic_identities(fb, ho, impact, tp):
    """What ties the topic records to the impact records (`impact`: impact_ref's (nodes, scenarios)) and to topic_results:
      - the sums over a scenario's topics of leaders_moved and of departed_replicas are the scenario impact record's fields;
      - a single-topic scenario's topic record equals its scenario impact record word for word;
      - max_topic_inbound <= the scenario's max_inbound (a broker receives at least what one topic sends it);
      - words 1, 4 and 5 follow from topic_results alone;
      - every word is non-negative and word 15 is 0."""
    _, si = impact
    topics, scen = tp
    owner = _owner(fb)
    status = ho.topic_results["status"]
    for s in range(fb.n_scenarios):
        mine = np.nonzero(owner == s)[0]
        for f in ("leaders_moved", "departed_replicas"):
            assert int(topics[f][mine].sum()) == int(si[f][s]), (s, f)
        if len(mine) == 1:
            for f in abi.TOPIC_IMPACT_FIELDS:
                assert int(topics[f][mine[0]]) == int(si[f][s]), (s, f)
        assert int(scen["max_topic_inbound"][s]) <= int(si["max_inbound"][s]), s
        assert int(scen["max_topic_outbound"][s]) <= int(si["max_outbound"][s]), s
        ok = [t for t in mine if int(status[t]) == abi.KAS_OK]
        mr = ho.topic_results["moved_replicas"][ok] if ok else np.zeros(0, np.int64)
        mp = ho.topic_results["moved_partitions"][ok] if ok else np.zeros(0, np.int64)
        assert int(scen["topics_ok"][s]) == len(ok)
        assert int(scen["topics_moved"][s]) == int((mr > 0).sum())
        assert int(scen["max_topic_moved_replicas"][s]) == (int(mr.max()) if ok else 0)
        assert int(scen["max_topic_moved_partitions"][s]) == (int(mp.max()) if ok else 0)
        for f in abi.SCENARIO_TOPIC_FIELDS:
            assert int(scen[f][s]) >= 0, (s, f)
        assert int(scen["reserved"][s]) == 0

"""NumPy restatement of the impact records (include/kas_abi.h, ABI v6: kas_node_impact / kas_scenario_impact) over a
FlatBatch and the HostOutputs of a solve with every row in place.  The checker of tests/test_impact_*.py, not a product path.

For each scenario, over each of its topics whose status is KAS_OK, and each row p: C = the first clen cells of cur[p]
(clen = cur_len[p], or cur_width), O = the cells of out[p] up to the first pad.  Per node b: replicas_before / _after =
cells of C / O naming b, leaders_before / _after = rows whose C[0] / O[0] is b, inbound = cells of O naming b that are not
in C, outbound = cells of C naming b that are not in O.  Per scenario: departed_replicas = cells of C that name no node,
leaders_moved = rows with olen > 0 and (clen == 0 or O[0] != C[0]), and max / min over the nodes (all 0 without nodes).
"""
from __future__ import annotations

import numpy as np

from kafka_assigner_amd import abi

FIELDS = abi.NODE_IMPACT_FIELDS


def _topic_owner(fb):
    owner = np.full(fb.n_topics, -1, dtype=np.int64)
    for s in range(fb.n_scenarios):
        b, c = int(fb.scen["topic_begin"][s]), int(fb.scen["topic_count"][s])
        owner[b:b + c] = s
    return owner


def impact_ref(fb, ho, cells16: bool = False, cur16=None):
    """(nodes NODE_IMPACT_DTYPE [sum of n_nodes], scenarios SCENARIO_IMPACT_DTYPE [S]) for `fb` solved into `ho` (every row in
    place).  cells16: ho.out holds uint16 node indices and the cur cells are `cur16` (flatten.to_cells16(fb) by default)."""
    if cells16 and cur16 is None:
        from kafka_assigner_amd.flatten import to_cells16
        cur16 = to_cells16(fb)
    S = fb.n_scenarios
    n_nodes = np.clip(fb.scen["n_nodes"], 0, None).astype(np.int64)
    base = np.concatenate([[0], np.cumsum(n_nodes)]).astype(np.int64)
    nodes = np.zeros(int(base[-1]), dtype=abi.NODE_IMPACT_DTYPE)
    scen = np.zeros(S, dtype=abi.SCENARIO_IMPACT_DTYPE)
    counts = [np.zeros((int(n), 6), dtype=np.int64) for n in n_nodes]
    departed = np.zeros(S, dtype=np.int64)
    moved = np.zeros(S, dtype=np.int64)
    owner = _topic_owner(fb)
    for t in range(fb.n_topics):
        s = int(owner[t])
        if s < 0 or int(ho.topic_results["status"][t]) != abi.KAS_OK:
            continue
        td = fb.topics[t]
        P, cw, ow = int(td["n_partitions"]), int(td["cur_width"]), int(td["out_width"])
        if P == 0:
            continue
        N, off = int(n_nodes[s]), int(fb.scen["node_off"][s])
        ids = fb.node_id[off:off + N].astype(np.int64)
        co, oo = int(td["cur_off"]), int(td["out_off"])
        if cells16:
            C = cur16[co:co + P * cw].astype(np.int64).reshape(P, cw)
            C = np.where(C == abi.KAS_CELL16_NONE, -1, C)
            O = ho.out[oo:oo + P * ow].astype(np.int64).reshape(P, ow)
            O = np.where(O == abi.KAS_CELL16_NONE, -1, O)

            def node(v):
                return np.where((v >= 0) & (v < N), v, -1)
        else:
            C = fb.cur[co:co + P * cw].astype(np.int64).reshape(P, cw)
            O = ho.out[oo:oo + P * ow].astype(np.int64).reshape(P, ow)

            def node(v):
                if N == 0:
                    return np.full(v.shape, -1, dtype=np.int64)
                pos = np.searchsorted(ids, v)
                hit = ids[np.minimum(pos, N - 1)] == v
                return np.where(hit & (pos < N), pos, -1)
        lo = int(td["cur_len_off"])
        clen = fb.aux[lo:lo + P].astype(np.int64) if lo >= 0 else np.full(P, cw, dtype=np.int64)
        cmask = np.arange(cw)[None, :] < clen[:, None]
        omask = np.cumprod(O != -1, axis=1).astype(bool)
        olen = omask.sum(axis=1)
        cn, on = node(C), node(O)
        in_o = ((C[:, :, None] == O[:, None, :]) & omask[:, None, :]).any(axis=2)
        in_c = ((O[:, :, None] == C[:, None, :]) & cmask[:, None, :]).any(axis=2)
        k = counts[s]

        def add(f, idx):
            if idx.size:
                k[:, f] += np.bincount(idx, minlength=N)[:N]
        add(0, cn[cmask & (cn >= 0)])
        add(1, on[omask & (on >= 0)])
        if cw:
            add(2, cn[(clen > 0) & (cn[:, 0] >= 0), 0])
        add(3, on[(olen > 0) & (on[:, 0] >= 0), 0])
        add(4, on[omask & (on >= 0) & ~in_c])
        add(5, cn[cmask & (cn >= 0) & ~in_o])
        departed[s] += int((cmask & (cn < 0)).sum())
        first_differs = (clen == 0) if cw == 0 else ((clen == 0) | (O[:, 0] != C[:, 0]))
        moved[s] += int(((olen > 0) & first_differs).sum())
    for s in range(S):
        N = int(n_nodes[s])
        blk = nodes[int(base[s]):int(base[s + 1])]
        for f, name in enumerate(FIELDS):
            blk[name] = counts[s][:, f]
        if N == 0:
            continue
        k = counts[s]
        scen[s] = (departed[s], moved[s], k[:, 4].max(), k[:, 5].max(), k[:, 1].min(), k[:, 1].max(), k[:, 3].min(), k[:, 3].max())
    return nodes, scen


def assert_same_impact(want, got, what: str = ""):
    """Field by field equality of two (nodes, scenarios) pairs, with the first difference in the message."""
    wn, ws = want
    gn, gs = got
    assert wn.shape == gn.shape and ws.shape == gs.shape, (what, wn.shape, gn.shape, ws.shape, gs.shape)
    for f in abi.NODE_IMPACT_FIELDS:
        bad = np.nonzero(wn[f] != gn[f])[0]
        assert bad.size == 0, f"{what}: node record {bad[0]} field {f}: want {wn[f][bad[0]]}, got {gn[f][bad[0]]}"
    for f in abi.SCENARIO_IMPACT_FIELDS:
        bad = np.nonzero(ws[f] != gs[f])[0]
        assert bad.size == 0, f"{what}: scenario {bad[0]} field {f}: want {ws[f][bad[0]]}, got {gs[f][bad[0]]}"


def check_invariants(fb, ho, imp):
    """sum of inbound == moved_replicas per scenario; sum of replicas_after == the cells the scenario emitted (its OK topics)."""
    nodes, scen = imp
    base = np.concatenate([[0], np.cumsum(np.clip(fb.scen["n_nodes"], 0, None))]).astype(np.int64)
    owner = _topic_owner(fb)
    for s in range(fb.n_scenarios):
        blk = nodes[int(base[s]):int(base[s + 1])]
        assert int(blk["inbound"].sum()) == int(ho.scenario_results["moved_replicas"][s]), s
        emitted = 0
        for t in np.nonzero(owner == s)[0]:
            if int(ho.topic_results["status"][t]) != abi.KAS_OK:
                continue
            td = fb.topics[t]
            P, ow, oo = int(td["n_partitions"]), int(td["out_width"]), int(td["out_off"])
            O = ho.out[oo:oo + P * ow].reshape(P, ow).astype(np.int64)
            pad = abi.KAS_CELL16_NONE if ho.out.dtype == np.uint16 else -1
            emitted += int(np.cumprod(O != pad, axis=1).sum())
        assert int(blk["replicas_after"].sum()) == emitted, s
        assert int(blk["leaders_after"].sum()) <= int(blk["replicas_after"].sum())

"""NumPy restatement of the rack records (include/kas_abi.h: kas_rack_impact / kas_scenario_rack_impact) over a FlatBatch and
the HostOutputs of a solve with every row in place.  The checker of tests/test_racks_*.py, not a product path; written from the
header's definitions, not from the kernel.

Rows, C, O, clen and olen are impact_ref's.  rr = report_rack (parallel to fb.node_rack; None: fb.node_rack), R_s = 1 + max rr
over the scenario's nodes (0 without nodes).  A cell that names node i has rack rr[i]; a cell of C that names no node is not
known.  Per row: kB / dB = known cells of C / distinct racks among them, kA / dA = cells of O that name a node / distinct racks
among them.  Per rack: the sums of the node records (impact_ref's) of its nodes, and their number.  Per scenario: the eight row
sums, R_s and the max / min over ALL racks r < R_s (a rack index no node has counts with zeros).
"""
from __future__ import annotations

import numpy as np

from impact_ref import _topic_owner, impact_ref
from kafka_assigner_amd import abi

ROW = abi.SCENARIO_RACK_ROW_FIELDS


def rack_counts(fb, report_rack=None):
    rr = fb.node_rack if report_rack is None else np.asarray(report_rack)
    out = []
    for s in range(fb.n_scenarios):
        off, n = int(fb.scen["node_off"][s]), max(int(fb.scen["n_nodes"][s]), 0)
        out.append(int(rr[off:off + n].max()) + 1 if n else 0)
    return np.asarray(out, dtype=np.int64)


def _distinct(r):
    """per row: racks r[p, :] (-1 = none) -> number of distinct values >= 0"""
    P, W = r.shape
    d = np.zeros(P, dtype=np.int64)
    for j in range(W):
        first = r[:, j] >= 0
        for i in range(j):
            first &= r[:, i] != r[:, j]
        d += first
    return d


def rack_ref(fb, ho, report_rack=None, cells16: bool = False, cur16=None, nodes=None):
    """(racks RACK_IMPACT_DTYPE [sum of R_s], scenarios SCENARIO_RACK_IMPACT_DTYPE [S], rack_off int64 [S + 1]).
    nodes: the node impact records to fold (default: impact_ref's of the same solve)."""
    if cells16 and cur16 is None:
        from kafka_assigner_amd.flatten import to_cells16
        cur16 = to_cells16(fb)
    if nodes is None:
        nodes = impact_ref(fb, ho, cells16=cells16, cur16=cur16)[0]
    rr_all = (fb.node_rack if report_rack is None else np.asarray(report_rack)).astype(np.int64)
    S = fb.n_scenarios
    n_nodes = np.clip(fb.scen["n_nodes"], 0, None).astype(np.int64)
    base = np.concatenate([[0], np.cumsum(n_nodes)]).astype(np.int64)
    R = rack_counts(fb, report_rack)
    rack_off = np.concatenate([[0], np.cumsum(R)]).astype(np.int64)
    racks = np.zeros(int(rack_off[-1]), dtype=abi.RACK_IMPACT_DTYPE)
    scen = np.zeros(S, dtype=abi.SCENARIO_RACK_IMPACT_DTYPE)
    sums = np.zeros((S, len(ROW)), dtype=np.int64)
    owner = _topic_owner(fb)
    for t in range(fb.n_topics):
        s = int(owner[t])
        if s < 0 or int(ho.topic_results["status"][t]) != abi.KAS_OK:
            continue
        td = fb.topics[t]
        P, cw, ow = int(td["n_partitions"]), int(td["cur_width"]), int(td["out_width"])
        N, off = int(n_nodes[s]), int(fb.scen["node_off"][s])
        if P == 0 or N == 0:
            continue
        ids = fb.node_id[off:off + N].astype(np.int64)
        rr = rr_all[off:off + N]
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
                pos = np.searchsorted(ids, v)
                hit = ids[np.minimum(pos, N - 1)] == v
                return np.where(hit & (pos < N), pos, -1)
        lo = int(td["cur_len_off"])
        clen = fb.aux[lo:lo + P].astype(np.int64) if lo >= 0 else np.full(P, cw, dtype=np.int64)
        cmask = np.arange(cw)[None, :] < np.clip(clen, 0, cw)[:, None]
        omask = np.cumprod(O != -1, axis=1).astype(bool)
        cn, on = node(C), node(O)
        rc = np.where(cmask & (cn >= 0), rr[np.clip(cn, 0, N - 1)], -1)       # the rack of every known cell of C
        ro = np.where(omask & (on >= 0), rr[np.clip(on, 0, N - 1)], -1)       # the rack of every cell of O that names a node
        kB, kA = (rc >= 0).sum(axis=1), (ro >= 0).sum(axis=1)
        dB, dA = _distinct(rc), _distinct(ro)
        in_c = ((O[:, :, None] == C[:, None, :]) & cmask[:, None, :]).any(axis=2)
        rack_known = ((ro[:, :, None] == rc[:, None, :]) & (rc >= 0)[:, None, :]).any(axis=2)
        fresh = (ro >= 0) & ~in_c & ~rack_known
        sums[s] += [int((kB - dB).sum()), int((kA - dA).sum()), int((kB > dB).sum()), int((kA > dA).sum()),
                    int(((kB >= 2) & (dB == 1)).sum()), int(((kA >= 2) & (dA == 1)).sum()), int(fresh.sum()), int((dA < dB).sum())]
    for s in range(S):
        N, off, Rs = int(n_nodes[s]), int(fb.scen["node_off"][s]), int(R[s])
        if N == 0:
            continue
        rr = rr_all[off:off + N]
        blk = nodes[int(base[s]):int(base[s + 1])]
        dst = racks[int(rack_off[s]):int(rack_off[s + 1])]
        dst["nodes"] = np.bincount(rr, minlength=Rs)
        for f in abi.NODE_IMPACT_FIELDS:
            dst[f] = np.bincount(rr, weights=blk[f].astype(np.float64), minlength=Rs).astype(np.int64)
        for f, v in zip(ROW, sums[s]):
            scen[f][s] = v
        scen["n_racks"][s] = Rs
        scen["max_rack_inbound"][s] = dst["inbound"].max(); scen["max_rack_outbound"][s] = dst["outbound"].max()
        scen["min_rack_replicas_after"][s] = dst["replicas_after"].min(); scen["max_rack_replicas_after"][s] = dst["replicas_after"].max()
        scen["min_rack_leaders_after"][s] = dst["leaders_after"].min(); scen["max_rack_leaders_after"][s] = dst["leaders_after"].max()
    return racks, scen, rack_off


def assert_same_racks(want, got, what: str = ""):
    """Field by field equality of two (racks, scenarios, rack_off) triples, with the first difference in the message."""
    wr, ws, wo = want
    gr, gs, go = got
    assert np.array_equal(np.asarray(wo), np.asarray(go)), (what, "rack_off", list(wo), list(go))
    assert wr.shape == gr.shape and ws.shape == gs.shape, (what, wr.shape, gr.shape, ws.shape, gs.shape)
    for f in abi.RACK_IMPACT_FIELDS + ("reserved",):
        bad = np.nonzero(wr[f] != gr[f])[0]
        assert bad.size == 0, f"{what}: rack record {bad[0]} field {f}: want {wr[f][bad[0]]}, got {gr[f][bad[0]]}"
    for f in abi.SCENARIO_RACK_FIELDS + ("reserved",):
        bad = np.nonzero(ws[f] != gs[f])[0]
        assert bad.size == 0, f"{what}: scenario {bad[0]} field {f}: want {ws[f][bad[0]]}, got {gs[f][bad[0]]}"


def check_identities(fb, ho, nodes, rk):
    """sum over racks of each field == sum over nodes; sum of inbound == moved_replicas; nodes sum to n_nodes"""
    racks, scen, rack_off = rk
    base = np.concatenate([[0], np.cumsum(np.clip(fb.scen["n_nodes"], 0, None))]).astype(np.int64)
    for s in range(fb.n_scenarios):
        r = racks[int(rack_off[s]):int(rack_off[s + 1])]
        blk = nodes[int(base[s]):int(base[s + 1])]
        for f in abi.NODE_IMPACT_FIELDS:
            assert int(r[f].sum()) == int(blk[f].sum()), (s, f)
        assert int(r["nodes"].sum()) == blk.shape[0], s
        assert int(r["inbound"].sum()) == int(ho.scenario_results["moved_replicas"][s]), s
        assert all(int(scen[f][s]) >= 0 for f in abi.SCENARIO_RACK_FIELDS), s

"""NumPy restatement of a choice (include/kas_abi.h: kas_choose_spec / kas_choice).  The checker of tests/test_choose_*.py, not a
product path.

The key of scenario s is (crit_0(s), ..., crit_{n-1}(s), s), smaller is better; only scenarios with status KAS_OK take part.
np.lexsort orders them, cumsum gives the offsets, and the packed rows and node blocks are slices of an out pool with every row in
place and of impact_ref's node table.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from kafka_assigner_amd import abi


def criterion(sr, si, key) -> np.ndarray:
    """int64 [S]: the criterion `key` (a name of abi.KEY_NAMES or its KAS_KEY_* number) of every scenario"""
    name = abi.KEY_NAMES[key] if not isinstance(key, str) else key
    if name in ("moved_replicas", "moved_partitions"):
        return sr[name].astype(np.int64)
    if name == "replica_spread":
        return si["max_replicas_after"].astype(np.int64) - si["min_replicas_after"]
    if name == "leader_spread":
        return si["max_leaders_after"].astype(np.int64) - si["min_leaders_after"]
    return si[name].astype(np.int64)


@dataclass
class Ranking:
    rank: np.ndarray          # int32 [S]
    chosen: np.ndarray        # int32 [k]
    n_ok: int
    order: np.ndarray         # the OK scenarios, best first


def rank_ref(sr, si, keys, k: int) -> Ranking:
    S = int(sr.shape[0])
    ok = np.nonzero(sr["status"] == abi.KAS_OK)[0]
    crit = [criterion(sr, si, key)[ok] for key in keys]
    order = ok[np.lexsort([ok] + crit[::-1])] if ok.size else ok          # (lexsort: the LAST key is the primary one)
    rank = np.full(S, -1, dtype=np.int32)
    rank[order] = np.arange(order.size, dtype=np.int32)
    chosen = np.full(k, -1, dtype=np.int32)
    m = min(k, order.size)
    chosen[:m] = order[:m]
    return Ranking(rank=rank, chosen=chosen, n_ok=int(order.size), order=order)


def offsets_ref(order, sizes, k: int) -> np.ndarray:
    """int64 [k + 1]: prefix sum of sizes[chosen]; entries past min(k, n_ok) repeat the last offset"""
    m = min(k, int(order.size))
    off = np.zeros(k + 1, dtype=np.int64)
    off[1:m + 1] = np.cumsum(np.asarray(sizes, dtype=np.int64)[order[:m]])
    off[m + 1:] = off[m]
    return off


def packed_cells(fb) -> np.ndarray:
    """int64 [S]: cells of each scenario's rows when packed: its topics' P x out_width"""
    out = np.zeros(fb.n_scenarios, dtype=np.int64)
    for s in range(fb.n_scenarios):
        b, c = int(fb.scen["topic_begin"][s]), int(fb.scen["topic_count"][s])
        t = fb.topics[b:b + c]
        out[s] = int((t["n_partitions"].astype(np.int64) * t["out_width"]).sum())
    return out


def scenario_rows(fb, out, s: int) -> np.ndarray:
    """scenario s's rows as kas_solve_host_select packs them: its topics in descriptor order, P x out_width cells each"""
    b, c = int(fb.scen["topic_begin"][s]), int(fb.scen["topic_count"][s])
    parts = [out[int(td["out_off"]):int(td["out_off"]) + int(td["n_partitions"]) * int(td["out_width"])] for td in fb.topics[b:b + c]]
    return np.concatenate(parts) if parts else out[:0]


@dataclass
class ChoiceRef:
    rank: np.ndarray
    chosen: np.ndarray
    n_ok: int
    row_off: np.ndarray
    node_off: np.ndarray
    rows: np.ndarray
    nodes: np.ndarray


def choose_ref(fb, sr, out, imp, keys, k: int) -> ChoiceRef:
    """The choice of k over `fb` solved into scenario records `sr` and the out pool `out` (every row in place; int32 or uint16
    cells), with imp = (nodes, scenarios) of impact_ref."""
    nodes, si = imp
    S = fb.n_scenarios
    r = rank_ref(sr[:S], si[:S], keys, k)
    n_nodes = np.clip(fb.scen["n_nodes"], 0, None).astype(np.int64)
    base = np.concatenate([[0], np.cumsum(n_nodes)]).astype(np.int64)
    row_off = offsets_ref(r.order, packed_cells(fb), k)
    node_off = offsets_ref(r.order, n_nodes, k)
    m = min(k, r.n_ok)
    rows = [scenario_rows(fb, out, int(s)) for s in r.chosen[:m]]
    blocks = [nodes[int(base[s]):int(base[s + 1])] for s in r.chosen[:m]]
    return ChoiceRef(rank=r.rank, chosen=r.chosen, n_ok=r.n_ok, row_off=row_off, node_off=node_off,
                     rows=np.concatenate(rows) if rows else out[:0], nodes=np.concatenate(blocks) if blocks else nodes[:0])


def assert_same_choice(want: ChoiceRef, got, what: str = ""):
    """`got`: anything with rank, chosen, n_ok, row_off, node_off, rows, nodes (rows / nodes at least as long as the offsets say)"""
    k = int(want.chosen.shape[0])
    assert int(got.n_ok) == want.n_ok, (what, "n_ok", int(got.n_ok), want.n_ok)
    for f in ("rank", "chosen", "row_off", "node_off"):
        w, g = getattr(want, f), np.asarray(getattr(got, f))
        assert w.shape == g.shape, (what, f, w.shape, g.shape)
        bad = np.nonzero(w != g)[0]
        assert bad.size == 0, f"{what}: {f}[{bad[0]}]: want {w[bad[0]]}, got {g[bad[0]]}"
    n, r = int(want.row_off[k]), int(want.node_off[k])
    assert want.rows.shape[0] == n and want.nodes.shape[0] == r
    bad = np.nonzero(want.rows.astype(np.int64) != np.asarray(got.rows[:n]).astype(np.int64))[0]
    assert bad.size == 0, f"{what}: packed row cell {bad[0]}: want {want.rows[bad[0]]}, got {got.rows[bad[0]]}"
    for f in abi.NODE_IMPACT_FIELDS:
        bad = np.nonzero(want.nodes[f] != got.nodes[f][:r])[0]
        assert bad.size == 0, f"{what}: packed node record {bad[0]} field {f}: want {want.nodes[f][bad[0]]}, got {got.nodes[f][bad[0]]}"
    assert (np.asarray(got.nodes["reserved"][:r]) == 0).all(), what

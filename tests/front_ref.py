"""NumPy restatement of the Pareto front (include/kas_abi.h: kas_front_spec).  The checker of tests/test_front_*.py, written from
the header's definition, not a product path.  O(S^2) by broadcasting.

eligible(s): status KAS_OK and every bound holds.  t dominates s: both eligible, key_i(t) <= key_i(s) for every i, and some
key_i(t) < key_i(s) or all equal and t < s.  member: eligible and not dominated.  Members are ordered by (key_0, ..., key_n-1, s).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from choose_ref import criterion, offsets_ref, packed_cells, scenario_rows
from kafka_assigner_amd import abi

NOT_OK, OVER_LIMIT, DOMINATED = abi.KAS_FRONT_NOT_OK, abi.KAS_FRONT_OVER_LIMIT, abi.KAS_FRONT_DOMINATED


@dataclass
class FrontRef:
    classes: np.ndarray       # int32 [S]: 0 for a member, or a class code
    rank: np.ndarray          # int32 [S]: a member's rank, or its class code
    chosen: np.ndarray        # int32 [k]
    counts: np.ndarray        # int32 [4]: n_ok, n_eligible, n_front, 0
    order: np.ndarray         # the members, in member order
    n_ok: int = 0
    row_off: np.ndarray = None
    node_off: np.ndarray = None
    rows: np.ndarray = None
    nodes: np.ndarray = None


def front_ref(sr, si, keys, k: int, within=()) -> FrontRef:
    """within: pairs (criterion, limit), or a dict"""
    S = int(sr.shape[0])
    pairs = list(within.items()) if isinstance(within, dict) else list(within)
    ok = sr["status"] == abi.KAS_OK
    eligible = ok.copy()
    for key, limit in pairs:
        eligible &= criterion(sr, si, key) <= int(limit)
    crit = np.stack([criterion(sr, si, key) for key in keys], axis=1) if S else np.zeros((0, len(keys)), np.int64)
    idx = np.arange(S)
    # dom[t, s]: t dominates s
    le, lt = np.ones((S, S), bool), np.zeros((S, S), bool)
    for i in range(crit.shape[1]):                              # (criterion by criterion: S x S at a time)
        le &= crit[:, None, i] <= crit[None, :, i]
        lt |= crit[:, None, i] < crit[None, :, i]
    dom = eligible[:, None] & eligible[None, :] & le & (lt | (idx[:, None] < idx[None, :]))
    dominated = dom.any(axis=0)
    member = eligible & ~dominated
    # a strict partial order: every dominated scenario is dominated by a member
    assert (dom[member][:, dominated].any(axis=0)).all() if dominated.any() else True
    assert not (dom & dom.T).any() and not dom[idx, idx].any()
    classes = np.where(~ok, NOT_OK, np.where(~eligible, OVER_LIMIT, np.where(dominated, DOMINATED, 0))).astype(np.int32)
    m = np.nonzero(member)[0]
    order = m[np.lexsort([m] + [crit[m, i] for i in range(crit.shape[1])][::-1])] if m.size else m
    rank = classes.copy()
    rank[order] = np.arange(order.size, dtype=np.int32)
    chosen = np.full(k, -1, np.int32)
    n = min(k, order.size)
    chosen[:n] = order[:n]
    counts = np.array([ok.sum(), eligible.sum(), order.size, 0], np.int32)
    return FrontRef(classes=classes, rank=rank, chosen=chosen, counts=counts, order=order, n_ok=int(ok.sum()))


def cut(r: FrontRef, k: int) -> FrontRef:
    """the same front with another k: classes, ranks and counts do not depend on k, chosen is the first k of the member order"""
    chosen = np.full(k, -1, np.int32)
    n = min(k, int(r.order.size))
    chosen[:n] = r.order[:n]
    return FrontRef(classes=r.classes, rank=r.rank, chosen=chosen, counts=r.counts, order=r.order, n_ok=r.n_ok)


def front_choice_ref(fb, sr, out, imp, keys, k: int, within=()) -> FrontRef:
    """front_ref over `fb` solved into `sr` and the out pool `out` (every row in place), with imp = (nodes, scenarios) of
    impact_ref: also the offsets, the packed rows and the node blocks of the first min(k, n_front) members (a ChoiceRef's fields,
    so that choose_ref.assert_same_choice compares it)"""
    nodes, si = imp
    S = fb.n_scenarios
    r = front_ref(sr[:S], si[:S], keys, k, within)
    n_nodes = np.clip(fb.scen["n_nodes"], 0, None).astype(np.int64)
    base = np.concatenate([[0], np.cumsum(n_nodes)]).astype(np.int64)
    r.row_off = offsets_ref(r.order, packed_cells(fb), k)
    r.node_off = offsets_ref(r.order, n_nodes, k)
    m = min(k, int(r.order.size))
    rows = [scenario_rows(fb, out, int(s)) for s in r.chosen[:m]]
    blocks = [nodes[int(base[s]):int(base[s + 1])] for s in r.chosen[:m]]
    r.rows = np.concatenate(rows) if rows else out[:0]
    r.nodes = np.concatenate(blocks) if blocks else nodes[:0]
    return r


def assert_same_front(want: FrontRef, got, what: str = ""):
    """rank, chosen and counts (got.counts: int32 [4]); offsets too when both have them"""
    assert np.array_equal(np.asarray(got.counts), want.counts), (what, "counts", np.asarray(got.counts), want.counts)
    for f in ("rank", "chosen") + (("row_off", "node_off") if want.row_off is not None and getattr(got, "row_off", None) is not None else ()):
        w, g = getattr(want, f), np.asarray(getattr(got, f))
        assert w.shape == g.shape, (what, f, w.shape, g.shape)
        bad = np.nonzero(w != g)[0]
        assert bad.size == 0, f"{what}: {f}[{bad[0]}]: want {w[bad[0]]}, got {g[bad[0]]}"

"""What the winners of a what-if call cost to bring back, as rows and as move lists, at the workload's own shape: 1,000 variants
(variant s takes broker s out) over one snapshot of 100,000 partitions x RF 3 on 1,000 brokers x 20 racks, k = 3.

  python scripts/e2e_moves.py [--log FILE] [--variants S] [--reps N]        # (needs the MI355X)

Three ways, alternated, wall time of the blocking host call and bytes that come back for the winners (their rows or their moves;
the records every way returns — topic and scenario records, scenario impact, rank, chosen, the winners' node blocks — are counted
apart, as `common_bytes`):
  rows            kas_solve_host_choose: the winners' whole assignment (the baseline: the parent commit's entry)
  moves_replicas  kas_solve_host_choose_moves, mask REPLICAS, no rows
  moves_all       kas_solve_host_choose_moves, mask REPLICAS | LEADER | ORDER, no rows
One JSON line on stdout (and appended to --log).
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from kafka_assigner_amd import abi, native  # noqa: E402
from kafka_assigner_amd import generator as G  # noqa: E402
from kafka_assigner_amd.flatten import node_set_batch  # noqa: E402

KEYS = ("moved_replicas", "leaders_moved")


def whatif_batch(S, P=100_000, N=1000, R=20):
    cur = G.random_assignment(11, P, N, R, 3)
    ids = [np.delete(np.arange(N, dtype=np.int32), s % N) for s in range(S)]
    racks = [(i % R).astype(np.int32) for i in ids]
    return node_set_batch(ids, racks, P, 3, 3, shared_cur=True, cur=cur)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", default=None)
    ap.add_argument("--variants", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    ctx = native.DeviceContext(0)
    fb = whatif_batch(a.variants)
    k = 3
    ways = {"rows": lambda: native.solve_host_choose(fb, KEYS, k, ctx=ctx),
            "moves_replicas": lambda: native.solve_host_choose_moves(fb, KEYS, k, ("replicas",), rows=False, ctx=ctx),
            "moves_all": lambda: native.solve_host_choose_moves(fb, KEYS, k, ("replicas", "leader", "order"), rows=False, ctx=ctx)}
    res = {name: f() for name, f in ways.items()}                  # (also the warm-up: plans, buffers)
    ho, ch = res["rows"]
    out = {"leg": "winners_as_rows_or_moves", "variants": fb.n_scenarios, "k": k, "n_ok": ch.n_ok, "chosen": ch.chosen.tolist(),
           "moved_partitions": [int(ho.scenario_results["moved_partitions"][s]) for s in ch.chosen if s >= 0],
           "common_bytes": int(16 * fb.n_topics + 32 * fb.n_scenarios + 32 * fb.n_scenarios + 4 * fb.n_scenarios + 4 * k + 16 * (k + 1) + 4
                               + 32 * ch.nodes.size),
           "rows_bytes": int(ch.rows.nbytes)}
    for name in ("moves_replicas", "moves_all"):
        _, c2, ml = res[name]
        assert np.array_equal(c2.chosen, ch.chosen) and not ml.truncated
        out[name + "_bytes"] = int(ml.moves.nbytes + ml.cells.nbytes + ml.move_off.nbytes + ml.cell_off.nbytes)
        out[name + "_count"] = [int(x) for x in np.diff(ml.move_off)]
    for _ in range(2):                                             # alternated, twice
        for name, f in ways.items():
            t0 = time.perf_counter()
            for _ in range(a.reps):
                f()
            out.setdefault(name + "_ms", []).append(round(1e3 * (time.perf_counter() - t0) / a.reps, 3))
    try:
        out["commit"] = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
    except Exception:
        out["commit"] = None
    line = json.dumps(out)
    print(line, flush=True)
    if a.log:
        with open(a.log, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

"""Figures of the impact pass (ABI v6) on the GPU: prints one JSON line per measurement.

  python scripts/impact_probe.py            # (needs the MI355X)

(a) the pass alone at the headline shape (1000 scenarios x 100k partitions x 1k brokers x 20 racks, RF 3, every scenario its own
    cur table): device time (events around kas_impact_device on the solve's stream) against the solve's
    (kas_plan_kernel_time_us), and GB/s over the 4 P (cur_width + out_width) bytes per topic the pass reads;
(b) bench.py's end_to_end what-if shape (1000 variants over ONE shared cur table), host calls three ways: without impact
    (kas_solve_host_select, one variant's rows), with impact and one variant's rows, with impact and no rows (n_select = 0);
(c) BASELINE configs[4]'s scenario (1M partitions x 5k brokers, RF 5): the pass cut into items and merged.
"""
from __future__ import annotations

import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from kafka_assigner_amd import abi, native  # noqa: E402
from kafka_assigner_amd import generator as G  # noqa: E402
from kafka_assigner_amd.flatten import host_tables, node_set_batch  # noqa: E402


def table_bytes(fb) -> int:
    t = fb.topics
    return int((4 * t["n_partitions"].astype(np.int64) * (t["cur_width"].astype(np.int64) + t["out_width"].astype(np.int64))).sum())


def device_leg(ctx, fb, name, reps=5):
    dev = torch.device("cuda", ctx.device)
    plan = native.Plan(ctx, fb)
    d_cur = torch.from_numpy(fb.cur).to(dev)
    d_out = torch.empty(fb.out_len, dtype=torch.int32, device=dev)
    d_tr = torch.zeros(fb.n_topics * 16, dtype=torch.uint8, device=dev)
    d_sr = torch.zeros(fb.n_scenarios * 32, dtype=torch.uint8, device=dev)
    d_nodes = torch.empty(int(native.node_blocks(fb)[-1]) * 32 + 32, dtype=torch.uint8, device=dev)
    d_scen = torch.empty(fb.n_scenarios * 32, dtype=torch.uint8, device=dev)
    st = torch.cuda.Stream(dev)
    st.wait_stream(torch.cuda.current_stream(dev))
    args = (d_cur.data_ptr(), d_out.data_ptr(), d_tr.data_ptr())
    for _ in range(2):
        plan.solve_device(*args, d_sr.data_ptr(), stream=st.cuda_stream)
        plan.impact_device(*args, d_nodes.data_ptr(), d_scen.data_ptr(), stream=st.cuda_stream)
    st.synchronize()
    plan.kernel_time_us()
    ms = []
    for _ in range(reps):
        plan.solve_device(*args, d_sr.data_ptr(), stream=st.cuda_stream)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        plan.impact_device(*args, d_nodes.data_ptr(), d_scen.data_ptr(), stream=st.cuda_stream)
        e1.record(st)
        st.synchronize()
        ms.append(e0.elapsed_time(e1))
    solve_us, _ = plan.kernel_time_us()
    plan.close()
    imp_ms = float(np.median(ms))
    nbytes = table_bytes(fb)
    print(json.dumps({"leg": name, "impact_ms": round(imp_ms, 4), "impact_ms_min": round(min(ms), 4),
                      "solve_ms": round(solve_us / 1e3, 4), "impact_over_solve": round(imp_ms * 1e3 / solve_us, 3),
                      "table_bytes": nbytes, "GB_per_s": round(nbytes / imp_ms / 1e6, 1)}), flush=True)


def whatif_leg(ctx, S=1000, P=100_000, N=1000, R=20, n=6):
    cur = G.random_assignment(11, P, N, R, 3)
    ids, racks = [], []
    for s in range(S):
        _, bs = G.scenario_action(29, s, N, R, actions=G.BENCH_ACTIONS)
        ids.append(bs.node_id); racks.append(bs.node_rack)
    fb = node_set_batch(ids, racks, P, 3, 3, shared_cur=True, cur=cur)
    sel = [S // 2]
    ways = {"no_impact_one_row_set": lambda: native.solve_host_select(fb, sel, ctx),
            "impact_one_row_set": lambda: native.solve_host_impact(fb, select=sel, ctx=ctx),
            "impact_no_rows": lambda: native.solve_host_impact(fb, select=[], ctx=ctx)}
    for f in ways.values():
        f()
    out = {"leg": "whatif_end_to_end_shape", "variants": S, "partitions": P, "brokers": N}
    for _ in range(2):                                     # alternated, twice
        for k, f in ways.items():
            t0 = time.perf_counter()
            for _ in range(n):
                f()
            out.setdefault(k + "_ms", []).append(round(1e3 * (time.perf_counter() - t0) / n, 3))
    print(json.dumps(out), flush=True)


def main():
    ctx = native.DeviceContext(0)
    S, P, N, R = 1000, 100_000, 1000, 20
    cur = G.torch_random_assignment(torch.Generator(device="cuda").manual_seed(7), S, P, N, R, 3, torch.device("cuda", 0)).cpu().numpy()
    sets = [G.scenario_action(7, s, N, R, actions=G.BENCH_ACTIONS)[1] for s in range(S)]
    fb = node_set_batch([b.node_id for b in sets], [b.node_rack for b in sets], P, 3, 3, cur=cur)
    device_leg(ctx, fb, "headline_device_pass")
    del fb, cur
    whatif_leg(ctx)
    cur5 = G.random_assignment(77, 1_000_000, 5000, 25, 5)
    bs = G.perturb_brokers(5000, 25, remove=list(range(0, 100, 5)), add=30)
    device_leg(ctx, node_set_batch([bs.node_id], [bs.node_rack], 1_000_000, 5, 5, cur=cur5), "configs4_scenario_device_pass")


if __name__ == "__main__":
    main()

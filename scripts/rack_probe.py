"""Figures of the rack pass (kas_rack_impact_device, kas_solve_host_rack_impact) on the GPU: prints one JSON line per measurement.

  python scripts/rack_probe.py            # (needs the MI355X)

At the headline what-if shape (1000 variants x 100k partitions x RF 3, ~1k brokers, 20 racks, one shared cur table):
(a) device time of the rack pass (row kernel + reduce kernel, events around kas_rack_impact_device) beside the impact pass's and
    the solve's, in the same run;
(b) wall time of kas_solve_host_rack_impact (n_select = 0, nodes = NULL) beside kas_solve_host_impact (n_select = 0), alternated,
    medians of five.
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

from kafka_assigner_amd import native  # noqa: E402
from kafka_assigner_amd import generator as G  # noqa: E402
from kafka_assigner_amd.flatten import node_set_batch  # noqa: E402


def whatif_batch(S=1000, P=100_000, N=1000, R=20):
    cur = G.random_assignment(11, P, N, R, 3)
    ids, racks = [], []
    for s in range(S):
        _, bs = G.scenario_action(29, s, N, R, actions=G.BENCH_ACTIONS)
        ids.append(bs.node_id); racks.append(bs.node_rack)
    return node_set_batch(ids, racks, P, 3, 3, shared_cur=True, cur=cur)


def device_leg(ctx, fb, reps=5):
    dev = torch.device("cuda", ctx.device)
    plan = native.Plan(ctx, fb)
    d_cur = torch.from_numpy(fb.cur).to(dev)
    d_out = torch.empty(fb.out_len, dtype=torch.int32, device=dev)
    d_tr = torch.zeros(fb.n_topics * 16, dtype=torch.uint8, device=dev)
    d_sr = torch.zeros(fb.n_scenarios * 32, dtype=torch.uint8, device=dev)
    d_nodes = torch.empty(int(native.node_blocks(fb)[-1]) * 32 + 32, dtype=torch.uint8, device=dev)
    d_scen = torch.empty(fb.n_scenarios * 32, dtype=torch.uint8, device=dev)
    cap = int(native.rack_counts(fb).sum())
    d_racks = torch.empty(cap * 32 + 32, dtype=torch.uint8, device=dev)
    d_rscen = torch.empty(fb.n_scenarios * 64, dtype=torch.uint8, device=dev)
    st = torch.cuda.Stream(dev)
    st.wait_stream(torch.cuda.current_stream(dev))
    args = (d_cur.data_ptr(), d_out.data_ptr(), d_tr.data_ptr())
    solve = lambda: plan.solve_device(*args, d_sr.data_ptr(), stream=st.cuda_stream)
    impact = lambda: plan.impact_device(*args, d_nodes.data_ptr(), d_scen.data_ptr(), stream=st.cuda_stream)
    racks = lambda: plan.rack_impact_device(*args, d_nodes.data_ptr(), d_scen.data_ptr(), d_racks.data_ptr(), cap, d_rscen.data_ptr(),
                                            stream=st.cuda_stream)
    for _ in range(2):
        solve(); impact(); racks()
    st.synchronize()
    plan.kernel_time_us()
    imp_ms, rack_ms = [], []
    for _ in range(reps):
        solve()
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record(st); impact(); e[1].record(st); racks(); e[2].record(st)
        st.synchronize()
        imp_ms.append(e[0].elapsed_time(e[1])); rack_ms.append(e[1].elapsed_time(e[2]))
    solve_us, _ = plan.kernel_time_us()
    plan.close()
    print(json.dumps({"leg": "headline_whatif_device_passes", "solve_ms": round(solve_us / 1e3, 4),
                      "impact_ms": round(float(np.median(imp_ms)), 4), "impact_ms_all": [round(v, 4) for v in imp_ms],
                      "rack_pass_ms": round(float(np.median(rack_ms)), 4), "rack_pass_ms_all": [round(v, 4) for v in rack_ms]}), flush=True)


def host_leg(ctx, fb, n=5):
    cap = int(native.rack_counts(fb).sum())
    ways = {"impact_no_rows": lambda: native.solve_host_impact(fb, select=[], ctx=ctx),
            "rack_impact_no_rows_no_nodes": lambda: native.solve_host_rack_impact(fb, select=[], nodes=False, racks_cap=cap, ctx=ctx)}
    for f in ways.values():
        f()
    out = {"leg": "headline_whatif_host_calls"}
    for _ in range(n):                                     # alternated
        for k, f in ways.items():
            t0 = time.perf_counter()
            f()
            out.setdefault(k + "_ms_all", []).append(round(1e3 * (time.perf_counter() - t0), 3))
    for k in ways:
        out[k + "_ms"] = float(np.median(out[k + "_ms_all"]))
    print(json.dumps(out), flush=True)


def main():
    ctx = native.DeviceContext(0)
    fb = whatif_batch()
    device_leg(ctx, fb)
    host_leg(ctx, fb)


if __name__ == "__main__":
    main()

"""Figures of the rank and gather kernels (kas_rank_device / kas_choose_device / kas_solve_host_choose) on the GPU: prints one
line per measurement, each with the figure it stands next to.

  python scripts/choose_probe.py            # (needs the MI355X)

(a) the headline what-if shape (1000 variants x 100k partitions x 1k brokers x 20 racks, RF 3, one shared cur table), device
    tables: the solve (kas_plan_kernel_time_us), the impact pass, rank + gather for k = 1 and k = 16, the rank kernel alone —
    events on the solve's stream;
(b) the rank kernel alone on synthetic records at S = 1,000, 8,000 and 64,000;
(c) the what-if host call at the headline shape, wall time, three ways, alternated: kas_solve_host_impact with n_select = 0,
    kas_solve_host_choose with k = 1, and the two calls the latter replaces (n_select = 0, then kas_solve_host_select of the
    winner).
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
from kafka_assigner_amd.flatten import node_set_batch  # noqa: E402

KEYS = ("moved_replicas", "leaders_moved")
LOG = os.path.join(ROOT, "profiles", "choose_probe.log")


def emit(record):
    """one line on stdout and in profiles/choose_probe.log"""
    line = json.dumps(record)
    print(line, flush=True)
    with open(LOG, "a") as f:
        f.write(line + "\n")


def whatif_batch(S=1000, P=100_000, N=1000, R=20):
    cur = G.random_assignment(11, P, N, R, 3)
    ids, racks = [], []
    for s in range(S):
        _, bs = G.scenario_action(29, s, N, R, actions=G.BENCH_ACTIONS)
        ids.append(bs.node_id); racks.append(bs.node_rack)
    return node_set_batch(ids, racks, P, 3, 3, shared_cur=True, cur=cur)


def timed(st, fn, reps=5):
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st); fn(); e1.record(st)
        st.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(min(ms))


def device_leg(ctx, fb):
    dev = torch.device("cuda", ctx.device)
    S = fb.n_scenarios
    plan = native.Plan(ctx, fb)
    d_cur = torch.from_numpy(fb.cur).to(dev)
    d_out = torch.empty(fb.out_len, dtype=torch.int32, device=dev)
    d_tr = torch.zeros(fb.n_topics * 16, dtype=torch.uint8, device=dev)
    d_sr = torch.zeros(S * 32, dtype=torch.uint8, device=dev)
    n_nodes = int(native.node_blocks(fb)[-1])
    d_nodes = torch.empty(n_nodes * 32 + 32, dtype=torch.uint8, device=dev)
    d_scen = torch.empty(S * 32, dtype=torch.uint8, device=dev)
    st = torch.cuda.Stream(dev)
    st.wait_stream(torch.cuda.current_stream(dev))
    args = (d_cur.data_ptr(), d_out.data_ptr(), d_tr.data_ptr())
    solve = lambda: plan.solve_device(*args, d_sr.data_ptr(), stream=st.cuda_stream)
    impact = lambda: plan.impact_device(*args, d_nodes.data_ptr(), d_scen.data_ptr(), stream=st.cuda_stream)
    for _ in range(2):
        solve(); impact()
    st.synchronize()
    plan.kernel_time_us()
    for _ in range(3):
        solve()
    st.synchronize()
    solve_us, _ = plan.kernel_time_us()
    imp_ms, _ = timed(st, impact)
    out = {"leg": "headline_whatif_device", "scenarios": S, "solve_ms": round(solve_us / 1e3, 4), "impact_ms": round(imp_ms, 4)}
    cells = native.packed_cells(fb)
    d_rank = torch.empty(S, dtype=torch.int32, device=dev)
    d_nok = torch.empty(1, dtype=torch.int32, device=dev)
    for k in (1, 16):
        rows_cap = int(np.sort(cells)[::-1][:k].sum())
        nodes_cap = int(np.sort(fb.scen["n_nodes"].astype(np.int64))[::-1][:k].sum())
        d_chosen = torch.empty(k, dtype=torch.int32, device=dev)
        d_ro, d_no = torch.empty(k + 1, dtype=torch.int64, device=dev), torch.empty(k + 1, dtype=torch.int64, device=dev)
        d_rows = torch.empty(rows_cap, dtype=torch.int32, device=dev)
        d_cn = torch.empty(nodes_cap * 32, dtype=torch.uint8, device=dev)
        choose = lambda: plan.choose_device(KEYS, k, d_out.data_ptr(), d_sr.data_ptr(), d_nodes.data_ptr(), d_scen.data_ptr(),
                                            d_rank.data_ptr(), d_chosen.data_ptr(), d_ro.data_ptr(), d_no.data_ptr(), d_nok.data_ptr(),
                                            d_rows.data_ptr(), rows_cap, d_cn.data_ptr(), nodes_cap, stream=st.cuda_stream)
        choose(); st.synchronize()
        med, low = timed(st, choose)
        out["rank_and_gather_k%d_ms" % k] = round(med, 4)
        out["rank_and_gather_k%d_ms_min" % k] = round(low, 4)
        out["gathered_bytes_k%d" % k] = 4 * rows_cap + 32 * nodes_cap
    d_chosen = torch.empty(1, dtype=torch.int32, device=dev)
    rank = lambda: native.rank_device(d_sr.data_ptr(), d_scen.data_ptr(), S, KEYS, 1, d_rank.data_ptr(), d_chosen.data_ptr(),
                                      d_nok.data_ptr(), stream=st.cuda_stream, ctx=ctx)
    rank(); st.synchronize()
    med, low = timed(st, rank)
    out["rank_alone_ms"], out["rank_alone_ms_min"] = round(med, 4), round(low, 4)
    out["gather_k1_ms"] = round(out["rank_and_gather_k1_ms"] - med, 4)
    out["gather_k16_ms"] = round(out["rank_and_gather_k16_ms"] - med, 4)
    out["parent"] = "solve and impact pass exist in the parent (DESIGN 10: 2.67 / 0.81 ms with a cur table per scenario); rank and gather do not"
    emit(out)
    plan.close()


def rank_leg(ctx, S):
    dev = torch.device("cuda", ctx.device)
    rng = np.random.default_rng(S)
    sr = np.zeros(S, abi.SCENARIO_RESULT_DTYPE)
    si = np.zeros(S, abi.SCENARIO_IMPACT_DTYPE)
    sr["status"] = (rng.integers(0, 8, S) == 0) * abi.KAS_FAIL_UNASSIGNABLE
    sr["moved_replicas"] = rng.integers(0, 5000, S)
    si["leaders_moved"] = rng.integers(0, 2000, S)
    d_sr = torch.from_numpy(sr.view(np.uint8)).to(dev)
    d_si = torch.from_numpy(si.view(np.uint8)).to(dev)
    d_rank = torch.empty(S, dtype=torch.int32, device=dev)
    d_chosen = torch.empty(16, dtype=torch.int32, device=dev)
    d_nok = torch.empty(1, dtype=torch.int32, device=dev)
    st = torch.cuda.Stream(dev)
    st.wait_stream(torch.cuda.current_stream(dev))
    rank = lambda: native.rank_device(d_sr.data_ptr(), d_si.data_ptr(), S, KEYS, 16, d_rank.data_ptr(), d_chosen.data_ptr(),
                                      d_nok.data_ptr(), stream=st.cuda_stream, ctx=ctx)
    rank(); st.synchronize()
    med, low = timed(st, rank)
    emit({"leg": "rank_kernel_synthetic", "scenarios": S, "compares": S * S, "rank_ms": round(med, 4), "rank_ms_min": round(low, 4),
          "workgroups": (S + 256) // 256, "parent": "none: the parent sorts on the CPU after downloading every record"})


def host_leg(ctx, fb, n=6):
    def two_calls():
        ho, _, scen = native.solve_host_impact(fb, select=[], ctx=ctx)
        sr = ho.scenario_results[:fb.n_scenarios]
        ok = np.nonzero(sr["status"] == 0)[0]
        best = int(ok[np.lexsort([ok, scen["leaders_moved"][ok], sr["moved_replicas"][ok]])[0]])
        native.solve_host_select(fb, [best], ctx)
        return best
    ways = {"impact_no_rows": lambda: native.solve_host_impact(fb, select=[], ctx=ctx),
            "choose_k1": lambda: native.solve_host_choose(fb, KEYS, 1, ctx=ctx),
            "two_calls_impact_then_select": two_calls}
    best = two_calls()
    _, ch = native.solve_host_choose(fb, KEYS, 1, ctx=ctx)
    assert int(ch.chosen[0]) == best, (int(ch.chosen[0]), best)
    for f in ways.values():
        f()
    out = {"leg": "whatif_host_call_headline_shape", "variants": fb.n_scenarios, "winner": best,
           "parent": "impact_no_rows and the two-call pattern are the parent's entries (DESIGN 10: 5.0 ms with impact and no rows); choose_k1 is new"}
    for _ in range(2):                                     # alternated, twice
        for k, f in ways.items():
            t0 = time.perf_counter()
            for _ in range(n):
                f()
            out.setdefault(k + "_ms", []).append(round(1e3 * (time.perf_counter() - t0) / n, 3))
    emit(out)


def main():
    open(LOG, "w").close()
    ctx = native.DeviceContext(0)
    fb = whatif_batch()
    device_leg(ctx, fb)
    for S in (1000, 8000, 64000):
        rank_leg(ctx, S)
    host_leg(ctx, fb)


if __name__ == "__main__":
    main()

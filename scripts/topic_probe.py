"""Figures of the topic pass (kas_topic_impact_device, kas_solve_host_topic_impact) on the GPU: prints one JSON line per measurement.

  python scripts/topic_probe.py [headline] [many_topics] [host]      # (needs the MI355X; no argument: the three legs one after
                                                                     #  the other, each in a process and under a time limit of its own)

headline     the headline what-if shape (1000 variants x 100k partitions x RF 3, ~1k brokers, one topic each, one shared cur
             table): device time of the topic pass (events around kas_topic_impact_device) beside the impact pass's and the
             solve's in the same run, medians of five.
many_topics  the same rows as 200 topics x 500 rows per variant (200,000 topic descriptors).  First fit strands rows in topics
             this small, and a topic that is not KAS_OK streams nothing, so behind the solve the leg sets every status to KAS_OK
             and takes cur's rows, shifted by one partition, for out: every item then zeroes its histogram, streams its 500
             rows and reduces.  A second figure with every status set to a failure is the same launch without the rows: what
             zeroing and reducing an N-entry histogram per item costs.
host         wall time of kas_solve_host_topic_impact (n_select = 0) with and without host_impact beside kas_solve_host_impact
             (n_select = 0), alternated, medians of five; with KAS_HIP_LIB set to another build of the library (the parent
             commit's), only kas_solve_host_impact is timed.
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


def whatif_batch(S=1000, P=100_000, N=1000, R=20):
    cur = G.random_assignment(11, P, N, R, 3)
    ids, racks = [], []
    for s in range(S):
        _, bs = G.scenario_action(29, s, N, R, actions=G.BENCH_ACTIONS)
        ids.append(bs.node_id); racks.append(bs.node_rack)
    return node_set_batch(ids, racks, P, 3, 3, shared_cur=True, cur=cur)


def many_topics(fb, per=500):
    """the batch with every scenario's one topic of P rows described as P / per topics of `per` rows over the same cells"""
    S, P = fb.n_scenarios, int(fb.topics["n_partitions"][0])
    K = P // per
    topics = np.repeat(fb.topics, K)
    k = np.tile(np.arange(K, dtype=np.int64), S)
    topics["n_partitions"] = per
    topics["cur_off"] += k * per * 3
    topics["out_off"] += k * per * 3
    topics["name_hash"] = (3644 + k).astype(topics["name_hash"].dtype)
    scen = fb.scen.copy()
    scen["topic_begin"] = np.arange(S) * K
    scen["topic_count"] = K
    return type(fb)(scen=scen, topics=topics, node_id=fb.node_id, node_rack=fb.node_rack, cur=fb.cur, aux=fb.aux, ctx=fb.ctx, out_len=fb.out_len)


class Device:
    def __init__(self, ctx, fb):
        self.dev = dev = torch.device("cuda", ctx.device)
        self.fb = fb
        self.plan = native.Plan(ctx, fb)
        self.d_cur = torch.from_numpy(fb.cur).to(dev)
        self.d_out = torch.empty(fb.out_len, dtype=torch.int32, device=dev)
        self.d_tr = torch.zeros(fb.n_topics * 4, dtype=torch.int32, device=dev)
        self.d_sr = torch.zeros(fb.n_scenarios * 32, dtype=torch.uint8, device=dev)
        self.d_nodes = torch.empty(int(native.node_blocks(fb)[-1]) * 32 + 32, dtype=torch.uint8, device=dev)
        self.d_scen = torch.empty(fb.n_scenarios * 32, dtype=torch.uint8, device=dev)
        self.d_topics = torch.empty(fb.n_topics * 32, dtype=torch.uint8, device=dev)
        self.d_tscen = torch.empty(fb.n_scenarios * 64, dtype=torch.uint8, device=dev)
        self.st = torch.cuda.Stream(dev)
        self.st.wait_stream(torch.cuda.current_stream(dev))
        self.args = (self.d_cur.data_ptr(), self.d_out.data_ptr(), self.d_tr.data_ptr())

    def solve(self):
        self.plan.solve_device(*self.args, self.d_sr.data_ptr(), stream=self.st.cuda_stream)

    def impact(self):
        self.plan.impact_device(*self.args, self.d_nodes.data_ptr(), self.d_scen.data_ptr(), stream=self.st.cuda_stream)

    def topics(self):
        self.plan.topic_impact_device(*self.args, self.d_topics.data_ptr(), self.d_tscen.data_ptr(), stream=self.st.cuda_stream)

    def timed(self, fn, reps=5):
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(self.st); fn(); b.record(self.st)
            self.st.synchronize()
            ms.append(a.elapsed_time(b))
        return round(float(np.median(ms)), 4), [round(v, 4) for v in ms]


def headline_leg(ctx, fb):
    d = Device(ctx, fb)
    for _ in range(2):
        d.solve(); d.impact(); d.topics()
    d.st.synchronize()
    d.plan.kernel_time_us()
    d.solve()
    imp, imp_all = d.timed(d.impact)
    top, top_all = d.timed(d.topics)
    solve_us, _ = d.plan.kernel_time_us()
    scen = d.d_tscen.cpu().numpy().view(abi.SCENARIO_TOPIC_IMPACT_DTYPE)
    d.plan.close()
    print(json.dumps({"leg": "headline_whatif_device_passes", "solve_ms": round(solve_us / 1e3, 4), "impact_ms": imp, "impact_ms_all": imp_all,
                      "topic_pass_ms": top, "topic_pass_ms_all": top_all, "scenarios_ok": int(scen["topics_ok"].sum()),
                      "max_topic_inbound": int(scen["max_topic_inbound"].max())}), flush=True)


def many_topics_leg(ctx, fb):
    mt = many_topics(fb)
    d = Device(ctx, mt)
    d.solve()
    d.st.synchronize()
    solve_us, _ = d.plan.kernel_time_us()
    ok = int((d.d_tr.view(-1, 4)[:, 0] == abi.KAS_OK).sum())
    with torch.cuda.stream(d.st):                              # every topic OK, out = cur shifted by one partition
        d.d_tr.view(-1, 4)[:, 0] = abi.KAS_OK
        d.d_out.view(mt.n_scenarios, -1)[:] = torch.roll(d.d_cur.view(-1, 3), 1, 0).reshape(1, -1)
    for _ in range(2):
        d.topics()
    full, full_all = d.timed(d.topics)
    scen = d.d_tscen.cpu().numpy().view(abi.SCENARIO_TOPIC_IMPACT_DTYPE)
    with torch.cuda.stream(d.st):                              # no topic OK: the items zero and reduce, and stream nothing
        d.d_tr.view(-1, 4)[:, 0] = abi.KAS_FAIL_UNASSIGNABLE
    d.topics()
    bare, bare_all = d.timed(d.topics)
    d.plan.close()
    print(json.dumps({"leg": "many_topics_device_pass", "topics": mt.n_topics, "rows_per_topic": 500, "solve_ms": round(solve_us / 1e3, 4),
                      "topics_ok_after_the_solve": ok, "topic_pass_ms": full, "topic_pass_ms_all": full_all,
                      "topic_pass_without_rows_ms": bare, "topic_pass_without_rows_ms_all": bare_all,
                      "share_without_rows": round(bare / full, 3), "topics_counted": int(scen["topics_ok"].sum())}), flush=True)


def host_leg(ctx, fb, n=5):
    ways = {"impact_no_rows": lambda: native.solve_host_impact(fb, select=[], ctx=ctx)}
    if "KAS_HIP_LIB" not in os.environ:
        ways["topic_impact_no_rows_no_nodes"] = lambda: native.solve_host_topic_impact(fb, select=[], nodes=False, ctx=ctx)
        ways["topic_impact_no_rows_no_impact"] = lambda: native.solve_host_topic_impact(fb, select=[], impact=False, ctx=ctx)
    for f in ways.values():
        f()
    out = {"leg": "headline_whatif_host_calls", "lib": os.environ.get("KAS_HIP_LIB", "this tree's")}
    for _ in range(n):                                     # alternated
        for k, f in ways.items():
            t0 = time.perf_counter()
            f()
            out.setdefault(k + "_ms_all", []).append(round(1e3 * (time.perf_counter() - t0), 3))
    for k in ways:
        out[k + "_ms"] = float(np.median(out[k + "_ms_all"]))
    print(json.dumps(out), flush=True)


LEG_SECONDS = {"headline": 240, "many_topics": 300, "host": 240}


def main():
    legs = sys.argv[1:]
    if not legs:
        # every leg in a fresh child process under a time limit of its own; a leg that fails or runs out of time ends the run
        import subprocess
        for leg, limit in LEG_SECONDS.items():
            try:
                rc = subprocess.run([sys.executable, os.path.abspath(__file__), leg], timeout=limit).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:
                print(json.dumps({"leg": leg, "failed": rc}), flush=True)
                sys.exit(rc)
        return
    ctx = native.DeviceContext(0)
    fb = whatif_batch()
    if "headline" in legs:
        headline_leg(ctx, fb)
    if "many_topics" in legs:
        many_topics_leg(ctx, fb)
    if "host" in legs:
        host_leg(ctx, fb)


if __name__ == "__main__":
    main()

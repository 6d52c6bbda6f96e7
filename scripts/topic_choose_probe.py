"""Figures of ranking and fronting by topic criteria (the *_topics entries) on the GPU: one JSON line per measurement, on stdout and in
profiles/topic_choose_probe.log.  Medians of five with min and max, every pair alternated, all in one run.

  python scripts/topic_choose_probe.py [--parent-tree PATH]          # (needs the MI355X)

(a) the rank kernel, and the mark and front rank kernels, alone on synthetic records at S = 1,000 and 8,000: with broker keys (the
    instances that were always there), with rack keys (the instances that read the scenario rack records) and with topic keys (the
    instances that read the scenario topic records too; once with a rack key beside them), alternated;
(b) the what-if host call at the headline shape (1000 variants x 100k partitions x ~1k brokers x 20 racks, RF 3, one shared cur
    table), wall time: kas_solve_host_choose_topics with k = 1 by (max_topic_inbound, moved_replicas) and host_racks == NULL against
    the way to the same result without it — kas_solve_host_topic_impact with n_select = 0 and no node records, a CPU sort,
    kas_solve_host_select of the winner — alternated;
(c) kas_solve_host_choose with k = 1 at the same shape, this tree against the parent commit's (--parent-tree: a checkout of the
    parent with its library built, which its own binding loads; each in a child process of its own, alternated);
(d) bench.py --gpus 1 --steps 20 --warmup 5, alternated with the parent's in the same way.
Without --parent-tree, (c) and (d) measure this tree alone.
"""
from __future__ import annotations

import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = ROOT
if "--root" in sys.argv:                                    # a child measuring another checkout: its package, its library
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
sys.path.insert(0, ROOT)

LOG = os.path.join(HERE, "profiles", "topic_choose_probe.log")
BROKER_KEYS = ("moved_replicas", "leaders_moved")
RACK_KEYS = ("colocated_after", "rack_replica_spread")
TOPIC_KEYS = ("max_topic_inbound", "sum_topic_replica_spread")
MIXED_KEYS = ("max_topic_inbound", "rack_replica_spread")
HOST_KEYS = ("max_topic_inbound", "moved_replicas")


def emit(record):
    line = json.dumps(record)
    print(line, flush=True)
    with open(LOG, "a") as f:
        f.write(line + "\n")


def whatif_batch(S=1000, P=100_000, N=1000, R=20):
    from kafka_assigner_amd import generator as G
    from kafka_assigner_amd.flatten import node_set_batch
    cur = G.random_assignment(11, P, N, R, 3)
    ids, racks = [], []
    for s in range(S):
        _, bs = G.scenario_action(29, s, N, R, actions=G.BENCH_ACTIONS)
        ids.append(bs.node_id); racks.append(bs.node_rack)
    return node_set_batch(ids, racks, P, 3, 3, shared_cur=True, cur=cur)


def summary(ms):
    return {"median": round(float(np.median(ms)), 4), "min": round(float(min(ms)), 4), "max": round(float(max(ms)), 4),
            "all": [round(float(v), 4) for v in ms]}


# ---- (a) the kernels alone ------------------------------------------------------------------------------------------------
def kernel_leg(ctx, S, reps=5):
    import torch
    from kafka_assigner_amd import abi, native
    dev = torch.device("cuda", ctx.device)
    rng = np.random.default_rng(S)
    sr = np.zeros(S, abi.SCENARIO_RESULT_DTYPE)
    si = np.zeros(S, abi.SCENARIO_IMPACT_DTYPE)
    srk = np.zeros(S, abi.SCENARIO_RACK_IMPACT_DTYPE)
    stp = np.zeros(S, abi.SCENARIO_TOPIC_IMPACT_DTYPE)
    sr["status"] = (rng.integers(0, 8, S) == 0) * abi.KAS_FAIL_UNASSIGNABLE
    sr["moved_replicas"] = rng.integers(0, 5000, S)
    si["leaders_moved"] = rng.integers(0, 2000, S)
    srk["colocated_after"] = rng.integers(0, 400, S) * (rng.integers(0, 6, S) == 0)
    srk["max_rack_replicas_after"] = rng.integers(2000, 2600, S)
    srk["min_rack_replicas_after"] = rng.integers(1400, 2000, S)
    stp["max_topic_inbound"] = rng.integers(0, 60, S)
    stp["sum_topic_replica_spread"] = rng.integers(0, 300, S)
    up = lambda a: torch.from_numpy(a.view(np.uint8)).to(dev)
    d_sr, d_si, d_srk, d_stp = up(sr), up(si), up(srk), up(stp)
    d_rank = torch.empty(S, dtype=torch.int32, device=dev)
    d_chosen = torch.empty(16, dtype=torch.int32, device=dev)
    d_counts = torch.empty(4, dtype=torch.int32, device=dev)
    d_cls = torch.empty(S, dtype=torch.int32, device=dev)
    st = torch.cuda.Stream(dev)
    st.wait_stream(torch.cuda.current_stream(dev))
    out = (d_rank.data_ptr(), d_chosen.data_ptr(), d_counts.data_ptr())
    rec_ptrs = (d_sr.data_ptr(), d_si.data_ptr())
    kw = dict(stream=st.cuda_stream, ctx=ctx)
    ways = {
        "rank_broker_keys": lambda: native.rank_device(*rec_ptrs, S, BROKER_KEYS, 16, *out, **kw),
        "rank_rack_keys": lambda: native.rank_device_racks(*rec_ptrs, d_srk.data_ptr(), S, RACK_KEYS, 16, *out, **kw),
        "rank_topic_keys": lambda: native.rank_device_topics(*rec_ptrs, 0, d_stp.data_ptr(), S, TOPIC_KEYS, 16, *out, **kw),
        "rank_topic_and_rack_keys": lambda: native.rank_device_topics(*rec_ptrs, d_srk.data_ptr(), d_stp.data_ptr(), S, MIXED_KEYS, 16, *out, **kw),
        "mark_and_front_rank_broker_keys": lambda: native.front_rank_device(*rec_ptrs, S, abi.front_spec(BROKER_KEYS, None, 16), *out,
                                                                            d_cls.data_ptr(), **kw),
        "mark_and_front_rank_rack_keys": lambda: native.front_rank_device_racks(*rec_ptrs, d_srk.data_ptr(), S, abi.rack_front_spec(RACK_KEYS, None, 16),
                                                                                *out, d_cls.data_ptr(), **kw),
        "mark_and_front_rank_topic_keys": lambda: native.front_rank_device_topics(*rec_ptrs, 0, d_stp.data_ptr(), S,
                                                                                  abi.topic_front_spec(TOPIC_KEYS, None, 16), *out, d_cls.data_ptr(), **kw),
    }
    for f in ways.values():
        f()
    st.synchronize()
    ms = {k: [] for k in ways}
    for _ in range(reps):                                   # alternated
        for k, f in ways.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st); f(); e1.record(st)
            st.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    rec = {"leg": "a_kernels_alone", "scenarios": S, "workgroups": (S + 256) // 256, "unit": "ms, events around the launches"}
    rec.update({k: summary(v) for k, v in ms.items()})
    emit(rec)


# ---- (b) the host call against the two-call pattern -----------------------------------------------------------------------
def host_leg(ctx, fb, reps=5):
    from kafka_assigner_amd import native

    def two_calls():
        ho, tp = native.solve_host_topic_impact(fb, select=[], nodes=False, ctx=ctx)
        sr = ho.scenario_results[:fb.n_scenarios]
        ok = np.nonzero(sr["status"] == 0)[0]
        best = int(ok[np.lexsort([ok, sr["moved_replicas"][ok], tp.scenarios["max_topic_inbound"][ok]])[0]])
        native.solve_host_select(fb, [best], ctx)
        return best

    def one_call():
        _, ch, _, _, _ = native.solve_host_choose_topics(fb, HOST_KEYS, 1, ctx=ctx)
        return int(ch.chosen[0])
    ways = {"choose_topics_k1": one_call, "two_calls_topic_impact_sort_select": two_calls,
            "topic_impact_no_rows_no_nodes": lambda: native.solve_host_topic_impact(fb, select=[], nodes=False, ctx=ctx)}
    assert one_call() == two_calls()
    for f in ways.values():
        f()
    ms = {k: [] for k in ways}
    for _ in range(reps):                                   # alternated
        for k, f in ways.items():
            t0 = time.perf_counter()
            f()
            ms[k].append(1e3 * (time.perf_counter() - t0))
    rec = {"leg": "b_whatif_host_call_headline_shape", "variants": fb.n_scenarios, "unit": "ms, wall"}
    rec.update({k: summary(v) for k, v in ms.items()})
    a, b = ms["choose_topics_k1"], ms["two_calls_topic_impact_sort_select"]
    rec["margin_ms"] = round(float(np.median(b) - np.median(a)), 4)
    rec["spread_ms"] = round(float(max(max(a) - min(a), max(b) - min(b))), 4)
    emit(rec)


# ---- (c), (d): this library against the parent's, each in a child process ----------------------------------------------------
def child_choose():
    """(c)'s child: five kas_solve_host_choose calls (k = 1) at the headline shape behind two warm-up calls; prints their wall times"""
    from kafka_assigner_amd import native
    ctx = native.DeviceContext(0)
    fb = whatif_batch()
    for _ in range(2):
        native.solve_host_choose(fb, BROKER_KEYS, 1, ctx=ctx)
    ms = []
    for _ in range(5):
        t0 = time.perf_counter()
        native.solve_host_choose(fb, BROKER_KEYS, 1, ctx=ctx)
        ms.append(1e3 * (time.perf_counter() - t0))
    print("CHILD " + json.dumps(ms), flush=True)


def run_child(args, root, timeout):
    env = dict(os.environ)
    env.pop("KAS_HIP_LIB", None)
    done = subprocess.run([sys.executable] + args, env=env, cwd=root, capture_output=True, text=True, timeout=timeout)
    if done.returncode != 0:
        raise RuntimeError("child %s failed (%d): %s" % (args, done.returncode, done.stderr[-2000:]))
    print("child done: %s in %s" % (os.path.basename(args[0]), root), flush=True)
    return done.stdout


def ab_legs(parent_tree):
    libs = {"this": HERE}
    if parent_tree:
        libs["parent"] = os.path.abspath(parent_tree)
    choose = {k: [] for k in libs}
    for _ in range(2):                                      # alternated, twice
        for k, lib in libs.items():
            line = [l for l in run_child([os.path.abspath(__file__), "--child-choose", "--root", lib], lib, 600).splitlines() if l.startswith("CHILD ")][-1]
            choose[k].append(json.loads(line[6:]))
    rec = {"leg": "c_solve_host_choose_k1_headline_shape", "unit": "ms, wall; five calls per process, two processes per library, alternated"}
    for k, runs in choose.items():
        flat = [v for r in runs for v in r]
        rec[k] = {"median": round(float(np.median(flat)), 4), "min": round(min(flat), 4), "max": round(max(flat), 4),
                  "medians_per_process": [round(float(np.median(r)), 4) for r in runs]}
    emit(rec)
    bench = {k: [] for k in libs}
    for _ in range(2):                                      # alternated, twice
        for k, lib in libs.items():
            out = run_child([os.path.join(lib, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"], lib, 900)
            bench[k].append(json.loads([l for l in out.splitlines() if l.startswith("{")][-1]))
    rec = {"leg": "d_bench_gpus1_steps20_warmup5", "unit": "bench.py's own result lines, two runs per library, alternated"}
    for k, runs in bench.items():
        key = next((n for n in ("scenarios_per_s", "value", "throughput") if n in runs[0]), None)
        rec[k] = {"runs": runs if key is None else [r[key] for r in runs], "metric": key}
        if key is not None:
            rec[k]["median"] = float(np.median([r[key] for r in runs]))
    emit(rec)


def main():
    if "--child-choose" in sys.argv:
        return child_choose()
    parent_tree = sys.argv[sys.argv.index("--parent-tree") + 1] if "--parent-tree" in sys.argv else None
    open(LOG, "w").close()
    from kafka_assigner_amd import native
    ctx = native.DeviceContext(0)
    for S in (1000, 8000):
        kernel_leg(ctx, S)
    host_leg(ctx, whatif_batch())
    ab_legs(parent_tree)


if __name__ == "__main__":
    main()

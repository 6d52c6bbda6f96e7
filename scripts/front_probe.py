"""Figures of the Pareto front kernels (kas_front_rank_device / kas_solve_host_front) on the GPU: prints one line per measurement,
each with the figure it stands next to.  Medians of five after a warm-up, the sides alternated in one process.

  python scripts/front_probe.py [kernels] [host]        # (needs the MI355X; no argument: both legs)

kernels  mark + front rank (kas_front_rank_device) against the rank kernel (kas_rank_device, unchanged code: the yardstick) on
         the same synthetic records at S = 1,000 and 8,000, events on one stream.  The two new kernels' own times come from a
         kernel trace of this leg (rocprofv3 --kernel-trace --stats -- python scripts/front_probe.py kernels).
         KAS_FRONT_AB_LIB=path of a second build of the library (e.g. -DKAS_FRONT_MARK_UNROLL=1): the same call through it,
         alternated with the first — the A/B of the mark loop's unrolling.
host     kas_solve_host_front (k = 3) at the headline what-if shape (1,000 variants x 100k partitions x 1k brokers, one shared
         cur) against kas_solve_host_choose (k = 3) and against the two calls it replaces: kas_solve_host_impact with
         n_select = 0, the front on the CPU (NumPy, O(S^2) by broadcasting: its own time is reported apart, in
         two_calls_parts_ms = impact call, CPU front, select call), kas_solve_host_select of its first three members.  Wall time.
"""
from __future__ import annotations

import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from kafka_assigner_amd import abi, native  # noqa: E402
from choose_probe import whatif_batch  # noqa: E402

KEYS = ("moved_replicas", "leader_spread", "replica_spread")
LOG = os.path.join(ROOT, "profiles", "front_probe.log")


def emit(record):
    line = json.dumps(record)
    print(line, flush=True)
    with open(LOG, "a") as f:
        f.write(line + "\n")


def alternated(st, sides, reps=5):
    """{name: median ms} of the callables in `sides`, each timed by events on `st`, alternated, after one warm-up each"""
    for fn in sides.values():
        fn()
    st.synchronize()
    ms = {n: [] for n in sides}
    for _ in range(reps):
        for n, fn in sides.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st); fn(); e1.record(st)
            st.synchronize()
            ms[n].append(e0.elapsed_time(e1))
    return {n: round(float(np.median(v)), 4) for n, v in ms.items()}


def second_library(path):
    """kas_front_rank_device of another build of the library, on a context of its own"""
    L = C.CDLL(path)
    L.kas_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.kas_front_rank_device.restype = C.c_int
    L.kas_front_rank_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(abi.FrontSpec)] + [C.c_void_p] * 5
    h = C.c_void_p()
    assert L.kas_ctx_create(0, C.byref(h)) == 0
    return L, h


def kernels_leg(ctx, S, other):
    dev = torch.device("cuda", ctx.device)
    rng = np.random.default_rng(S)
    sr = np.zeros(S, abi.SCENARIO_RESULT_DTYPE)
    si = np.zeros(S, abi.SCENARIO_IMPACT_DTYPE)
    sr["status"] = (rng.integers(0, 8, S) == 0) * abi.KAS_FAIL_UNASSIGNABLE
    sr["moved_replicas"] = rng.integers(0, 5000, S)
    si["max_leaders_after"] = rng.integers(0, 64, S)
    si["max_replicas_after"] = rng.integers(0, 64, S)
    d_sr = torch.from_numpy(sr.view(np.uint8)).to(dev)
    d_si = torch.from_numpy(si.view(np.uint8)).to(dev)
    d_rank = torch.empty(S, dtype=torch.int32, device=dev)
    d_chosen = torch.empty(16, dtype=torch.int32, device=dev)
    d_counts = torch.empty(4, dtype=torch.int32, device=dev)
    d_cls = torch.empty(S, dtype=torch.int32, device=dev)
    st = torch.cuda.Stream(dev)
    st.wait_stream(torch.cuda.current_stream(dev))
    spec = abi.front_spec(KEYS, {"max_inbound": 10**9}, 16)
    sides = {"rank_ms": lambda: native.rank_device(d_sr.data_ptr(), d_si.data_ptr(), S, KEYS, 16, d_rank.data_ptr(), d_chosen.data_ptr(),
                                                   d_counts.data_ptr(), stream=st.cuda_stream, ctx=ctx),
             "mark_and_front_rank_ms": lambda: native.front_rank_device(d_sr.data_ptr(), d_si.data_ptr(), S, spec, d_rank.data_ptr(), d_chosen.data_ptr(),
                                                                        d_counts.data_ptr(), d_cls.data_ptr(), stream=st.cuda_stream, ctx=ctx)}
    if other:
        L, h = other
        sides["mark_and_front_rank_other_build_ms"] = lambda: L.kas_front_rank_device(
            h, d_sr.data_ptr(), d_si.data_ptr(), S, C.byref(spec), d_rank.data_ptr(), d_chosen.data_ptr(), d_counts.data_ptr(), d_cls.data_ptr(),
            C.c_void_p(st.cuda_stream))
    out = {"leg": "front_kernels_synthetic", "scenarios": S, "compares": S * S}
    out.update(alternated(st, sides))
    counts = d_counts.cpu().numpy()
    out.update(n_ok=int(counts[0]), n_eligible=int(counts[1]), n_front=int(counts[2]),
               parent="rank_ms is the parent's kernel, unchanged (profiles/choose_probe.log: 0.138 / 1.04 ms); the other two do not exist there")
    emit(out)


def cpu_front(sr, scen, k):
    ok = np.nonzero(sr["status"] == 0)[0]
    c = np.stack([sr["moved_replicas"][ok], scen["max_leaders_after"][ok] - scen["min_leaders_after"][ok],
                  scen["max_replicas_after"][ok] - scen["min_replicas_after"][ok]], axis=1).astype(np.int64)
    le = (c[:, None, :] <= c[None, :, :]).all(axis=2)
    lt = (c[:, None, :] < c[None, :, :]).any(axis=2)
    dom = le & (lt | (np.arange(ok.size)[:, None] < np.arange(ok.size)[None, :]))
    m = np.nonzero(~dom.any(axis=0))[0]
    m = m[np.lexsort([m, c[m, 2], c[m, 1], c[m, 0]])]
    return [int(s) for s in ok[m][:k]]


def host_leg(ctx, fb, n=5):
    parts = []                                              # (impact call, CPU front, select call) ms of every two_calls()

    def two_calls():
        t0 = time.perf_counter()
        ho, _, scen = native.solve_host_impact(fb, select=[], ctx=ctx)
        t1 = time.perf_counter()
        members = cpu_front(ho.scenario_results[:fb.n_scenarios], scen, 3)
        t2 = time.perf_counter()
        native.solve_host_select(fb, members, ctx)
        parts.append((1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * (time.perf_counter() - t2)))
        return members
    spec = abi.front_spec(KEYS, None, 3)
    ways = {"choose_k3": lambda: native.solve_host_choose(fb, KEYS, 3, ctx=ctx),
            "front_k3": lambda: native.solve_host_front(fb, spec, ctx=ctx),
            "two_calls_impact_cpu_front_select": two_calls}
    members = two_calls()
    _, fr, _ = native.solve_host_front(fb, spec, ctx=ctx)
    assert [int(s) for s in fr.chosen[:min(3, fr.n_front)]] == members, (fr.chosen, members)
    for f in ways.values():
        f()
    ms = {k: [] for k in ways}
    for _ in range(n):                                      # alternated
        for k, f in ways.items():
            t0 = time.perf_counter()
            f()
            ms[k].append(1e3 * (time.perf_counter() - t0))
    out = {"leg": "whatif_host_call_headline_shape", "variants": fb.n_scenarios, "n_front": fr.n_front, "members": members,
           "parent": "choose_k3 and the two-call pattern are the parent's entries (DESIGN 10.1: 3.83 / 7.46 ms with k = 1); front_k3 is new"}
    out.update({k + "_ms": round(float(np.median(v)), 3) for k, v in ms.items()})
    out["two_calls_parts_ms"] = [round(float(v), 3) for v in np.median(np.asarray(parts[-n:]), axis=0)]
    emit(out)


def main():
    legs = [a for a in sys.argv[1:] if a in ("kernels", "host")] or ["kernels", "host"]
    if len(legs) == 2:
        open(LOG, "w").close()
    ctx = native.DeviceContext(0)
    if "kernels" in legs:
        other = second_library(os.environ["KAS_FRONT_AB_LIB"]) if os.environ.get("KAS_FRONT_AB_LIB") else None
        for S in (1000, 8000):
            kernels_leg(ctx, S, other)
    if "host" in legs:
        host_leg(ctx, whatif_batch())


if __name__ == "__main__":
    main()

"""Figures of the batches pass (kas_batches_device) on the GPU: prints one JSON line per measurement.

  python scripts/batches_probe.py [headline]      # (needs the MI355X; no argument: the leg in a process and under a time limit of its own)

headline  the headline what-if shape (1000 variants x 100k partitions x RF 3, ~1k brokers, one topic each, one shared cur table).
          Device time (events around the device entry on one stream, median of five with min - max) of the pass over all 1,000
          variants, counts only, at cap_inbound 5, at cap_inbound 1 (the replay-heavy case) and at max_moves 100; of the pass over
          three variants with records; beside them, for comparison only, the solve, the moves pass (REPLICAS mask) over the same
          lists, and the reference loop (tests/batches_ref.py, plain Python) over one variant's downloaded rows.  The variant the
          reference loop cuts is also compared with the device's record of it.
"""
from __future__ import annotations

import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

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


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def headline_leg(ctx, fb):
    dev = torch.device("cuda", ctx.device)
    S = fb.n_scenarios
    plan = native.Plan(ctx, fb)
    d_cur = torch.from_numpy(fb.cur).to(dev)
    d_out = torch.empty(fb.out_len, dtype=torch.int32, device=dev)
    d_tr = torch.zeros(fb.n_topics * 4, dtype=torch.int32, device=dev)
    d_sr = torch.zeros(S * 32, dtype=torch.uint8, device=dev)
    st = torch.cuda.Stream(dev)
    st.wait_stream(torch.cuda.current_stream(dev))
    args = (d_cur.data_ptr(), d_out.data_ptr(), d_tr.data_ptr())

    def timed(fn, reps=5):
        fn()
        st.synchronize()
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(st); fn(); b.record(st)
            st.synchronize()
            ms.append(a.elapsed_time(b))
        return stats(ms)

    for _ in range(2):
        plan.solve_device(*args, d_sr.data_ptr(), stream=st.cuda_stream)
    st.synchronize()
    plan.kernel_time_us()
    plan.solve_device(*args, d_sr.data_ptr(), stream=st.cuda_stream)
    st.synchronize()
    solve_us, _ = plan.kernel_time_us()
    sr = d_sr.cpu().numpy().view(abi.SCENARIO_RESULT_DTYPE)
    ok = np.nonzero(sr["status"] == abi.KAS_OK)[0]
    print(json.dumps({"leg": "solve", "solve_ms": round(solve_us / 1e3, 4), "variants_ok": int(ok.size),
                      "moved_partitions_median": int(np.median(sr["moved_partitions"][ok])) if ok.size else 0,
                      "moved_partitions_max": int(sr["moved_partitions"].max())}), flush=True)
    d_all = torch.arange(S, dtype=torch.int32, device=dev)
    three = [int(s) for s in ok[:3]] if ok.size >= 3 else [0, 1, 2]
    d_three = torch.tensor(three, dtype=torch.int32, device=dev)
    d_scen = torch.zeros(S * 8, dtype=torch.int32, device=dev)
    stride = 4096
    d_recs = torch.zeros(3 * stride * 8, dtype=torch.int32, device=dev)

    def batches(caps, sel, n, recs=0, room=0):
        return lambda: plan.batches_device(caps, sel.data_ptr(), n, *args, d_scen.data_ptr(), recs, room, stream=st.cuda_stream)

    seen = {}
    for name, caps in (("cap_inbound_5", {"inbound": 5}), ("cap_inbound_1", {"inbound": 1}), ("max_moves_100", {"max_moves": 100})):
        t = timed(batches(caps, d_all, S))
        scen = d_scen.cpu().numpy().view(abi.SCENARIO_BATCHES_DTYPE)
        seen[name] = scen.copy()
        print(json.dumps(dict({"leg": "batches_all_variants_counts_only", "caps": name, "n_batches_median": int(np.median(scen["n_batches"][ok])) if ok.size else 0,
                               "n_batches_max": int(scen["n_batches"].max()), "moves": int(scen["n_moves"].sum())}, **t)), flush=True)
    t = timed(batches({"inbound": 5}, d_three, 3, d_recs.data_ptr(), stride))
    print(json.dumps(dict({"leg": "batches_three_variants_with_records", "caps": "cap_inbound_5", "stride": stride}, **t)), flush=True)
    # the moves pass over the same lists (REPLICAS mask), for comparison: offsets only, then with the records of the three
    d_moff = torch.zeros(S + 1, dtype=torch.int64, device=dev)
    d_coff = torch.zeros(S + 1, dtype=torch.int64, device=dev)
    t = timed(lambda: plan.moves_device(1, d_all.data_ptr(), S, *args, d_moff.data_ptr(), d_coff.data_ptr(), 0, 0, 0, 0, stream=st.cuda_stream))
    print(json.dumps(dict({"leg": "moves_pass_all_variants_offsets_only", "moves": int(d_moff.cpu()[-1])}, **t)), flush=True)
    room = native.moves_room(fb, three)
    d_moves = torch.zeros(room[0] * 16, dtype=torch.uint8, device=dev)
    d_cells = torch.zeros(room[1], dtype=torch.int32, device=dev)
    t = timed(lambda: plan.moves_device(1, d_three.data_ptr(), 3, *args, d_moff.data_ptr(), d_coff.data_ptr(), d_moves.data_ptr(), room[0],
                                        d_cells.data_ptr(), room[1], stream=st.cuda_stream))
    print(json.dumps(dict({"leg": "moves_pass_three_variants_with_records"}, **t)), flush=True)
    # the reference loop over one variant's downloaded rows (plain Python: the checker of the tests), and its record against the device's
    from types import SimpleNamespace
    from batches_ref import cut, scenario_moves
    s = three[0]
    td = fb.topics[int(fb.scen["topic_begin"][s])].copy()
    lo, cells = int(td["out_off"]), int(td["n_partitions"]) * int(td["out_width"])
    t0 = time.perf_counter()
    out = d_out[lo:lo + cells].cpu().numpy()
    download_ms = 1e3 * (time.perf_counter() - t0)
    td["out_off"] = 0
    scen1 = fb.scen[s:s + 1].copy()
    scen1["topic_begin"] = 0
    fb1 = type(fb)(scen=scen1, topics=np.array([td]), node_id=fb.node_id, node_rack=fb.node_rack, cur=fb.cur, aux=fb.aux, ctx=fb.ctx, out_len=cells)
    ho1 = SimpleNamespace(out=out, topic_results=np.zeros(1, abi.TOPIC_RESULT_DTYPE))
    ho1.topic_results["status"][0] = abi.KAS_OK
    t0 = time.perf_counter()
    mv = scenario_moves(fb1, ho1, 0)
    list_ms = 1e3 * (time.perf_counter() - t0)
    loops = {}
    for name, caps in (("cap_inbound_5", {"inbound": 5}), ("cap_inbound_1", {"inbound": 1}), ("max_moves_100", {"max_moves": 100})):
        t0 = time.perf_counter()
        rec, _ = cut(mv, caps)
        loops[name] = round(1e3 * (time.perf_counter() - t0), 3)
        got = {f: int(seen[name][f][s]) for f in abi.SCENARIO_BATCHES_FIELDS}
        assert got == rec, (name, got, rec)
    print(json.dumps({"leg": "reference_loop_one_variant_python", "variant": s, "moves": len(mv), "download_rows_ms": round(download_ms, 3),
                      "build_move_list_ms": round(list_ms, 3), "loop_ms": loops, "device_record_equal": True}), flush=True)
    plan.close()


LEG_SECONDS = {"headline": 420}


def main():
    legs = sys.argv[1:]
    if not legs:
        # the leg in a fresh child process under a time limit of its own; a leg that fails or runs out of time ends the run
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


if __name__ == "__main__":
    main()

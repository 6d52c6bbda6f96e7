"""Figures of the rounds pass (kas_rounds_device) on the GPU beside the batches pass over the same lists: prints one JSON line
per measurement.

  python scripts/rounds_probe.py [headline]      # (needs the MI355X; no argument: the leg in a process and under a time limit of its own)

headline  the headline what-if shape of scripts/batches_probe.py (1000 variants x 100k partitions x RF 3, ~1k brokers, one shared
          cur table).  Device time (events around the device entry on one stream, median of five with min - max) of the rounds
          pass and of the batches pass, ALTERNATED in one run, over all 1,000 variants counts only and over three variants with
          records, at cap_inbound 5 and 1.  Then the quality of the schedule over the variants that solve: n_rounds against
          n_batches (both from the device) and against the lower bound ceil(max_inbound / cap) (max_inbound from the impact
          pass), and, over the three variants' downloaded rows, against a true first fit (tests/rounds_ref.py, plain Python),
          whose monotone loop is also compared with the device's records.
"""
from __future__ import annotations

import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import torch  # noqa: E402

from batches_probe import stats, whatif_batch  # noqa: E402
from kafka_assigner_amd import abi, native  # noqa: E402


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

    def one(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st); fn(); b.record(st)
        st.synchronize()
        return a.elapsed_time(b)

    def alternated(fns, reps=5):
        """every function once untimed, then `reps` rounds in which each runs once, in turn"""
        for fn in fns:
            fn()
        st.synchronize()
        ms = [[] for _ in fns]
        for _ in range(reps):
            for k, fn in enumerate(fns):
                ms[k].append(one(fn))
        return [stats(m) for m in ms]

    for _ in range(3):
        plan.solve_device(*args, d_sr.data_ptr(), stream=st.cuda_stream)
    st.synchronize()
    n_nodes = int(native.node_blocks(fb)[-1])
    d_nodes = torch.zeros(max(n_nodes, 1) * 32, dtype=torch.uint8, device=dev)
    d_imp = torch.zeros(S * 32, dtype=torch.uint8, device=dev)
    plan.impact_device(*args, d_nodes.data_ptr(), d_imp.data_ptr(), stream=st.cuda_stream)
    st.synchronize()
    sr = d_sr.cpu().numpy().view(abi.SCENARIO_RESULT_DTYPE)
    imp = d_imp.cpu().numpy().view(abi.SCENARIO_IMPACT_DTYPE)
    ok = np.nonzero(sr["status"] == abi.KAS_OK)[0]
    print(json.dumps({"leg": "solve", "variants_ok": int(ok.size), "moved_partitions_median": int(np.median(sr["moved_partitions"][ok])),
                      "moved_partitions_max": int(sr["moved_partitions"].max()), "max_inbound_median": int(np.median(imp["max_inbound"][ok])),
                      "max_inbound_max": int(imp["max_inbound"][ok].max())}), flush=True)
    d_all = torch.arange(S, dtype=torch.int32, device=dev)
    three = [int(s) for s in ok[:3]]
    d_three = torch.tensor(three, dtype=torch.int32, device=dev)
    d_rscen = torch.zeros(S * 8, dtype=torch.int32, device=dev)
    d_bscen = torch.zeros(S * 8, dtype=torch.int32, device=dev)
    room = 4096
    most = int(sr["moved_partitions"][three].max())
    d_rrecs = torch.zeros(3 * room * 4, dtype=torch.int32, device=dev)
    d_rof = torch.zeros(3 * most, dtype=torch.int32, device=dev)
    d_brecs = torch.zeros(3 * room * 8, dtype=torch.int32, device=dev)

    def rounds(caps, sel, n, records):
        return lambda: plan.rounds_device(caps, sel.data_ptr(), n, *args, d_rscen.data_ptr(), d_rrecs.data_ptr() if records else 0,
                                          room if records else 0, d_rof.data_ptr() if records else 0, most if records else 0, stream=st.cuda_stream)

    def batches(caps, sel, n, records):
        return lambda: plan.batches_device(caps, sel.data_ptr(), n, *args, d_bscen.data_ptr(), d_brecs.data_ptr() if records else 0,
                                           room if records else 0, stream=st.cuda_stream)

    seen = {}
    for cap in (5, 1):
        caps = {"inbound": cap}
        tr, tb = alternated([rounds(caps, d_all, S, False), batches(caps, d_all, S, False)])
        rs = d_rscen.cpu().numpy().view(abi.SCENARIO_ROUNDS_DTYPE).copy()
        bs = d_bscen.cpu().numpy().view(abi.SCENARIO_BATCHES_DTYPE).copy()
        seen[cap] = rs
        assert (rs["n_moves"][ok] == sr["moved_partitions"][ok]).all() and (bs["n_moves"][ok] == rs["n_moves"][ok]).all()
        print(json.dumps(dict({"leg": "rounds_all_variants_counts_only", "cap_inbound": cap, "moves": int(rs["n_moves"].sum())}, **tr)), flush=True)
        print(json.dumps(dict({"leg": "batches_all_variants_counts_only", "cap_inbound": cap}, **tb)), flush=True)
        lb = np.maximum(-(-imp["max_inbound"][ok].astype(np.int64) // cap), (rs["n_moves"][ok] > 0).astype(np.int64))
        nr, nb = rs["n_rounds"][ok].astype(np.int64), bs["n_batches"][ok].astype(np.int64)
        assert (nr >= lb).all()
        moving = nr > 0
        print(json.dumps({"leg": "quality_all_variants", "cap_inbound": cap, "variants": int(ok.size), "n_rounds_median": float(np.median(nr)),
                          "n_batches_median": float(np.median(nb)), "lower_bound_median": float(np.median(lb)),
                          "rounds_fewer_than_batches": int((nr[moving] < nb[moving]).sum()), "variants_with_moves": int(moving.sum()),
                          "at_lower_bound": int((nr == lb).sum()), "batches_over_rounds_median": round(float(np.median(nb[moving] / nr[moving])), 3),
                          "rounds_over_bound_worst": round(float((nr[moving] / lb[moving]).max()), 3), "n_rounds_max": int(nr.max())}), flush=True)
        tr, tb = alternated([rounds(caps, d_three, 3, True), batches(caps, d_three, 3, True)])
        print(json.dumps(dict({"leg": "rounds_three_variants_with_records", "cap_inbound": cap, "round_stride": room, "move_stride": most}, **tr)), flush=True)
        print(json.dumps(dict({"leg": "batches_three_variants_with_records", "cap_inbound": cap, "stride": room}, **tb)), flush=True)
    # the three variants on the CPU: the header's loop against the device's records, and a true first fit
    from batches_ref import scenario_moves
    from rounds_ref import first_fit, lower_bound, monotone, records
    for s in three:
        td = fb.topics[int(fb.scen["topic_begin"][s])].copy()
        lo, cells = int(td["out_off"]), int(td["n_partitions"]) * int(td["out_width"])
        out = d_out[lo:lo + cells].cpu().numpy()
        td["out_off"] = 0
        scen1 = fb.scen[s:s + 1].copy()
        scen1["topic_begin"] = 0
        fb1 = type(fb)(scen=scen1, topics=np.array([td]), node_id=fb.node_id, node_rack=fb.node_rack, cur=fb.cur, aux=fb.aux, ctx=fb.ctx, out_len=cells)
        ho1 = SimpleNamespace(out=out, topic_results=np.zeros(1, abi.TOPIC_RESULT_DTYPE))
        ho1.topic_results["status"][0] = abi.KAS_OK
        mv = scenario_moves(fb1, ho1, 0)
        for cap in (5, 1):
            caps = {"inbound": cap}
            t0 = time.perf_counter()
            ro, by_in, by_out = monotone(mv, caps)
            loop_ms = 1e3 * (time.perf_counter() - t0)
            rec, _ = records(mv, ro, by_in, by_out)
            got = {f: int(seen[cap][f][s]) for f in abi.SCENARIO_ROUNDS_FIELDS}
            assert got == rec, (s, cap, got, rec)
            ff = first_fit(mv, caps)
            print(json.dumps({"leg": "reference_one_variant_python", "variant": s, "cap_inbound": cap, "moves": len(mv), "n_rounds": rec["n_rounds"],
                              "first_fit_rounds": 1 + max(ff) if ff else 0, "lower_bound": lower_bound(mv, caps), "loop_ms": round(loop_ms, 3),
                              "device_record_equal": True}), flush=True)
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

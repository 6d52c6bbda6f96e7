"""Round 7 on the MI355X (-m gpu): the batches of tests/test_sorted_rows_emu.py — 512 scenarios, 40 and 1,100 brokers — through
native.Plan / solve_device as the plan chooses (the slim fill, kas_p4_kernel, tiles of 64 rows on dword mid rows: the headline's
kernels), with first fit beside the order kernel and with double tiles.  Every record against the flat-array CPU baseline, the
lists of 16 scenarios against the oracle (the digests in the records cover the lists of the others)."""
import functools

import numpy as np
import pytest

import sorted_rows_cases as cases
from kafka_assigner_amd import abi, native
from oracle_lib import cpu_fast_solve, oracle_solve

pytestmark = pytest.mark.gpu

LISTS_OF = (0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 12, 13, 300, 301, 511)     # the scenarios made by hand among them
TOPIC_FIELDS = ("status", "fail_partition", "moved_replicas", "moved_partitions")
SCENARIO_FIELDS = ("status", "fail_topic", "fail_partition", "moved_replicas", "moved_partitions", "digest")


@functools.lru_cache(maxsize=None)
def _case(name):
    """(batch, the CPU baseline's outputs, the oracle's): computed once, shared, never written to"""
    fb = cases.batch_40() if name == "40 brokers" else cases.batch_wide(1100)
    return fb, cpu_fast_solve(fb, threads=0), oracle_solve(fb, threads=0)


@pytest.mark.parametrize("flags", [0, abi.KAS_PLAN_P4_WITH_ORDER, abi.KAS_PLAN_RELAX_TILES_128],
                         ids=["the plan's choice", "first fit beside the order kernel", "double tiles"])
@pytest.mark.parametrize("name", ["40 brokers", "1100 brokers"])
def test_hip_sorted_rows(name, flags):
    import torch
    fb, fast, want = _case(name)
    ctx = native.default_context()
    plan = native.Plan(ctx, fb)
    plan.set_flags(flags)
    what = plan.describe()
    assert "dword mid rows" in what, what
    if flags == 0:
        assert "kas_fill_slim_kernel<3>" in what and "kas_p4_kernel<3>" in what and "tiles of 64 rows" in what, what
    elif flags == abi.KAS_PLAN_P4_WITH_ORDER:
        assert "kas_p4_order_kernel<3>" in what, what
    else:
        assert "tiles of 128 rows" in what, what
    dev = torch.device("cuda", ctx.device)
    d_cur = torch.from_numpy(fb.cur).to(dev)
    d_out = torch.full((fb.out_len,), -7, dtype=torch.int32, device=dev)
    d_tr = torch.zeros(fb.n_topics * abi.TOPIC_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_sr = torch.zeros(fb.n_scenarios * abi.SCENARIO_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    plan.solve_device(d_cur.data_ptr(), d_out.data_ptr(), d_tr.data_ptr(), d_sr.data_ptr(),
                      stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    plan.close()
    tr = d_tr.cpu().numpy().view(abi.TOPIC_RESULT_DTYPE)
    sr = d_sr.cpu().numpy().view(abi.SCENARIO_RESULT_DTYPE)
    out = d_out.cpu().numpy()
    for f in TOPIC_FIELDS:
        np.testing.assert_array_equal(tr[f], fast.topic_results[f][:fb.n_topics], err_msg=f"{name}, flags {flags:#x}: topic_results.{f}")
    for f in SCENARIO_FIELDS:
        np.testing.assert_array_equal(sr[f], fast.scenario_results[f][:fb.n_scenarios], err_msg=f"{name}, flags {flags:#x}: scenario_results.{f}")
    for s in LISTS_OF:
        tb, tc = int(fb.scen[s]["topic_begin"]), int(fb.scen[s]["topic_count"])
        for t in range(tb, tb + tc):
            td = fb.topics[t]
            lo = int(td["out_off"]); hi = lo + int(td["n_partitions"]) * int(td["out_width"])
            np.testing.assert_array_equal(out[lo:hi], want.out[lo:hi], err_msg=f"{name}, flags {flags:#x}: lists of scenario {s}, topic {t}")

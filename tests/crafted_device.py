"""The device side of the crafted cases (tests/crafted_cases.py) for tests/test_batches_crafted_gpu.py and
tests/test_rounds_crafted_gpu.py.  Test infrastructure.

kas_batches_device and kas_rounds_device read whatever cur / out / topic_results pointers they are handed; all they ask of the plan
is that it has solved once.  So a case's plan solves once into scratch tables nobody reads again, and the passes then run over the
out pool and the topic results the case wrote itself, in buffers of their own, on one non-default stream.  Every output array is
full of FILL before a call and carries one guard record behind it; every call is made twice and must give the same bytes.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from kafka_assigner_amd import abi, native

FILL = 0x5A5A5A5A


def device_tables(ctx, case, cells16):
    """Plan + uploads + the one solve; raises native.KasError where the plan refuses the case's shape.  Close with .plan.close()."""
    import torch
    fb, ho, cur16 = case.tables(cells16)
    plan = native.Plan(ctx, fb, cells16=cells16)
    try:
        dev = torch.device("cuda", ctx.device)
        cdt = torch.int16 if cells16 else torch.int32
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).to(dev)
        d = SimpleNamespace(plan=plan, dev=dev)
        d.cur = up(cur16.view(np.int16) if cells16 else fb.cur)
        d.aux_t = up(fb.aux) if fb.aux.size else None
        d.aux = d.aux_t.data_ptr() if d.aux_t is not None else 0
        # the scratch tables of the one solve the passes ask the plan for
        d.s_out = torch.full((max(fb.out_len, 1),), -2, dtype=cdt, device=dev)
        d.s_tr = torch.zeros(max(fb.n_topics, 1) * abi.TOPIC_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d.s_sr = torch.zeros(max(fb.n_scenarios, 1) * abi.SCENARIO_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        # the crafted tables
        d.out = up(ho.out.view(np.int16) if cells16 else ho.out)
        d.tr = up(np.frombuffer(ho.topic_results.tobytes(), np.uint8))
        d.stream = torch.cuda.Stream(dev)
        d.stream.wait_stream(torch.cuda.current_stream(dev))
        plan.solve_device(d.cur.data_ptr(), d.s_out.data_ptr(), d.s_tr.data_ptr(), d.s_sr.data_ptr(), aux=d.aux, stream=d.stream.cuda_stream)
        return d
    except BaseException:
        plan.close()
        raise


def _filled(d, words):
    import torch
    return torch.full((words,), FILL, dtype=torch.int32, device=d.dev)


def _twice(d, make, launch, what):
    """two calls into fresh arrays; -> the first call's arrays on the host, after holding the second's to the same bytes"""
    import torch
    runs = []
    for _ in range(2):
        arrays = make()
        d.stream.wait_stream(torch.cuda.current_stream(d.dev))            # (the fills run on the current stream)
        launch(*arrays)
        runs.append(arrays)
    d.stream.synchronize()
    first, second = [[a.cpu().numpy() for a in arrays] for arrays in runs]
    for a, b in zip(first, second):
        assert a.tobytes() == b.tobytes(), (what, "a second call gave other bytes")
    return first


def run_batches(d, caps, select, stride, what=""):
    """kas_batches_device / 16 over the crafted tables -> (scenario records, batch records); guards and both calls' bytes held"""
    import torch
    n = len(select)
    sel = torch.tensor(list(select), dtype=torch.int32, device=d.dev)

    def launch(scen, recs):
        d.plan.batches_device(caps, sel.data_ptr(), n, d.cur.data_ptr(), d.out.data_ptr(), d.tr.data_ptr(), scen.data_ptr(),
                              recs.data_ptr() if stride else 0, stride, aux=d.aux, stream=d.stream.cuda_stream)
    scen, recs = _twice(d, lambda: (_filled(d, (n + 1) * 8), _filled(d, (n * stride + 1) * 8)), launch, what)
    fill = np.int32(FILL)
    assert (scen[8 * n:] == fill).all() and (recs[8 * n * stride:] == fill).all(), (what, "written behind the arrays")
    return scen[:8 * n].view(abi.SCENARIO_BATCHES_DTYPE), recs[:8 * n * stride].view(abi.MOVE_BATCH_DTYPE)


def run_rounds(d, caps, select, rs, ms, what=""):
    """kas_rounds_device / 16 over the crafted tables -> (scenario records, round records, round_of); guards and both calls' bytes held"""
    import torch
    n = len(select)
    sel = torch.tensor(list(select), dtype=torch.int32, device=d.dev)

    def launch(scen, recs, rof):
        d.plan.rounds_device(caps, sel.data_ptr(), n, d.cur.data_ptr(), d.out.data_ptr(), d.tr.data_ptr(), scen.data_ptr(),
                             recs.data_ptr() if rs else 0, rs, rof.data_ptr() if ms else 0, ms, aux=d.aux, stream=d.stream.cuda_stream)
    scen, recs, rof = _twice(d, lambda: (_filled(d, (n + 1) * 8), _filled(d, (n * rs + 1) * 4), _filled(d, n * ms + 1)), launch, what)
    fill = np.int32(FILL)
    assert (scen[8 * n:] == fill).all() and (recs[4 * n * rs:] == fill).all() and (rof[n * ms:] == fill).all(), (what, "written behind the arrays")
    return scen[:8 * n].view(abi.SCENARIO_ROUNDS_DTYPE), recs[:4 * n * rs].view(abi.MOVE_ROUND_DTYPE), rof[:n * ms]


def assert_plan_refuses(ctx, case, cells16, text, what=""):
    """the library plans no launch for this shape: the passes cannot see it (the emulator runs the case all the same)"""
    import pytest
    fb, _, _ = case.tables(cells16)
    with pytest.raises(native.KasError) as e:
        native.Plan(ctx, fb, cells16=cells16).close()
    assert e.value.code == abi.KAS_E_UNSUPPORTED and text in e.value.detail, (what, e.value.code, e.value.detail)

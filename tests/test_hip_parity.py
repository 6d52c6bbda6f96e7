"""The parity tests proper: the HIP path, called through the C ABI on a real MI355X, must be
bit-identical to the oracle — statuses, failing partition ids, every partition -> broker list,
movement counts, digests and Context counters.  (-m gpu; the driver runs these on the GPU box.)"""
import numpy as np
import pytest
from hypothesis import HealthCheck, given, seed, settings

from kafka_assigner_amd import abi, native
from kafka_assigner_amd import generator as G
from kafka_assigner_amd.flatten import Scenario, Topic, flatten, uniform_batch
from oracle_lib import oracle_solve
from parity_util import assert_same_outputs
from test_emu_parity import _batch, _multi_topic_scenarios
from test_oracle_vs_literal import scenarios

pytestmark = pytest.mark.gpu
TICKET_ORDER = abi.KAS_PLAN_TICKET_ORDER      # the ticket form of P5 where the relaxation form would run
TILES_64 = abi.KAS_PLAN_RELAX_TILES_64        # relaxation form over tiles of 64 rows / double tiles whatever the batch size
TILES_128 = abi.KAS_PLAN_RELAX_TILES_128      # (by itself: double tiles for batches of fewer than 512 scenarios)


def test_device_is_gfx950_and_library_loaded():
    import torch
    assert torch.cuda.is_available()
    assert "gfx950" in torch.cuda.get_device_properties(0).gcnArchName
    assert native.load().kas_device_count() >= 1
    native.default_context()


@seed(20260921)
@settings(max_examples=150, deadline=None, suppress_health_check=[HealthCheck.too_slow])
@given(scenarios())
def test_hip_equals_oracle_small_odd_inputs(sc):
    brokers, racks, topics = sc
    fb = flatten([Scenario(brokers=brokers, racks=racks, want_context=True,
                           topics=[Topic(n, c, rf, parts) for n, c, rf, parts in topics])])
    assert_same_outputs(fb, oracle_solve(fb), native.solve_host(fb), "hip")


@seed(20260922)
@settings(max_examples=150, deadline=None, suppress_health_check=[HealthCheck.too_slow])
@given(scenarios())
def test_hip_equals_oracle_small_odd_inputs_without_context_io(sc):
    """No Context in or out: lists up to 3 wide take the relaxation form of P5 (KAS_PLAN_TICKET_ORDER: the ticket form)."""
    brokers, racks, topics = sc
    fb = flatten([Scenario(brokers=brokers, racks=racks, want_context=False,
                           topics=[Topic(n, c, rf, parts) for n, c, rf, parts in topics])])
    want = oracle_solve(fb)
    assert_same_outputs(fb, want, native.solve_host(fb), "hip (no ctx)")
    assert_same_outputs(fb, want, native.solve_host_with_flags(fb, TICKET_ORDER), "hip (no ctx), ticket form")
    assert_same_outputs(fb, want, native.solve_host_with_flags(fb, TILES_64), "hip (no ctx), relaxation form, tiles of 64 rows")


@pytest.mark.parametrize("P,N,R,RF,actions", [
    (1000, 40, 8, 3, G.ACTIONS),
    (3000, 100, 10, 3, ("remove1",)),
    (2048, 64, 8, 2, ("add_k",)),
    (777, 40, 10, 5, G.ACTIONS),
    (640, 24, 8, 4, ("replace1", "remove1")),
    (8000, 80, 8, 3, ("replace1", "add_k")),  # many P4 windows in flight on all waves; zero-slack strandings
])
def test_hip_equals_oracle_seeded_batches(P, N, R, RF, actions):
    fb = _batch(1234, 6, P, N, R, RF, actions)
    want = oracle_solve(fb)
    assert_same_outputs(fb, want, native.solve_host(fb), "hip")
    assert_same_outputs(fb, want, native.solve_host_with_flags(fb, TICKET_ORDER), "hip ticket form")
    assert_same_outputs(fb, want, native.solve_host_with_flags(fb, TILES_64), "hip relaxation form, tiles of 64 rows")
    assert_same_outputs(fb, want, native.solve_host_with_flags(fb, TILES_128), "hip relaxation form, double tiles")
    assert_same_outputs(fb, want, native.solve_host_with_flags(fb, abi.KAS_PLAN_NO_RTN_QUOTA), "hip fill, quota drawn without the atomic-with-return")
    assert_same_outputs(fb, want, native.solve_host_with_flags(fb, abi.KAS_PLAN_NO_INDEX_ROWS), "hip fill, cur read by both row scans (no index rows)")
    assert_same_outputs(fb, want, native.solve_host_with_flags(fb, abi.KAS_PLAN_NO_INDEX_ROWS | abi.KAS_PLAN_SPLIT_P4 | TILES_64), "hip no index rows, kas_p4_kernel, tiles of 64 rows")
    assert_same_outputs(fb, want, native.solve_host_with_flags(fb, abi.KAS_PLAN_INDEX_ROWS), "hip fill, index rows (cur read once)")
    assert_same_outputs(fb, want, native.solve_host_with_flags(fb, abi.KAS_PLAN_INDEX_ROWS | abi.KAS_PLAN_SPLIT_P4 | TILES_64), "hip index rows, kas_p4_kernel, tiles of 64 rows")
    assert_same_outputs(fb, want, native.solve_host_with_flags(fb, abi.KAS_PLAN_INDEX_ROWS | abi.KAS_PLAN_FILL_WITH_P4), "hip index rows, first fit inside the fill workgroup")
    assert_same_outputs(fb, want, native.solve_host_with_flags(fb, abi.KAS_PLAN_FILL_WITH_P4), "hip first fit inside the fill workgroup (no kas_p4_kernel)")
    assert_same_outputs(fb, want, native.solve_host_with_flags(fb, abi.KAS_PLAN_SPLIT_P4), "hip first fit in kas_p4_kernel (what batches of >= 512 scenarios take)")
    assert_same_outputs(fb, want, native.solve_host_with_flags(fb, abi.KAS_PLAN_SPLIT_P4 | TILES_64), "hip kas_p4_kernel + tiles of 64 rows: the headline's kernels")
    assert_same_outputs(fb, want, native.solve_host_with_flags(fb, abi.KAS_PLAN_FULL_FILL | abi.KAS_PLAN_SPLIT_P4 | TILES_64), "hip the headline's kernels without the slim fill kernel in front")
    assert_same_outputs(fb, want, native.solve_host_with_flags(fb, abi.KAS_PLAN_FULL_FILL), "hip no slim fill kernel, the plan's choice otherwise")
    assert_same_outputs(fb, want, native.solve_host_with_flags(fb, abi.KAS_PLAN_P4_WITH_ORDER), "hip first fit as a wavefront of the order kernel's workgroup (kas_p4_order_kernel where it applies)")
    assert_same_outputs(fb, want, native.solve_host_with_flags(fb, abi.KAS_PLAN_P4_WITH_ORDER | TILES_64), "hip kas_p4_order_kernel, tiles of 64 rows")
    assert_same_outputs(fb, want, native.solve_host_with_flags(fb, abi.KAS_PLAN_P4_WITH_ORDER | TILES_128 | abi.KAS_PLAN_INDEX_ROWS), "hip kas_p4_order_kernel, double tiles, index rows")
    # the general multi-sweep sticky fill must agree with the rack-diverse histogram/quota form,
    # the tile-round preference ordering with the ticket form, at every workgroup width
    assert_same_outputs(fb, want, native.solve_host_with_flags(fb, 1), "hip generic fill")
    assert_same_outputs(fb, want, native.solve_host_with_flags(fb, 2), "hip round order")
    assert_same_outputs(fb, want, native.solve_host_with_flags(fb, 4), "hip 4 x uint16 counter rows")
    assert_same_outputs(fb, want, native.solve_host_with_flags(fb, 8), "hip chunk-count pass instead of per-chunk histograms")
    for nw, g in ((1, 1), (2, 2), (4, 4), (2, 1)):
        assert_same_outputs(fb, want, native.solve_host_with_flags(fb, (nw << 8) | (g << 12)),
                            f"hip {nw} waves, {g} scenarios per wave")
    assert_same_outputs(fb, want, native.solve_host_with_flags(fb, 3 | (1 << 8)), "hip generic+round, 1 wave")


def test_hip_dword_mid_rows_where_they_apply():
    """KAS_FLAG_MID32 (round 6; tests/test_emu_parity.py has the emulator's run of the same batches): between the fill and the order
    kernel a row is ONE dword — its holders sorted, 11 bits each — on int32 cells, lists 3 wide, at most 2,047 brokers, the
    relaxation form; every place first fit runs in, scenarios handed back to the full fill kernel, topics narrower than the batch,
    failures, node indices around 1,024 and up to 2,046.  Lists equal to the oracle's on either layout."""
    from test_emu_parity import dword_mid_row_cases
    ctx = native.default_context()
    for what, fb, flag_words in dword_mid_row_cases():
        want = oracle_solve(fb)
        for flags in flag_words:
            assert_same_outputs(fb, want, native.solve_host_with_flags(fb, flags), f"hip dword mid rows: {what}, plan flags {flags:#x}")
        plan = native.Plan(ctx, fb)
        fits = int(fb.scen["n_nodes"].max()) <= 2047
        assert ("dword mid rows" in plan.describe()) == fits, plan.describe()
        plan.set_flags(abi.KAS_PLAN_NO_MID32)
        assert "dword mid rows" not in plan.describe(), plan.describe()
        plan.close()


def test_hip_relaxation_steps_of_1_2_and_4_tiles_at_their_edges():
    """The emulator's batch of tests/test_emu_parity.py (topics of one, two and four tiles of rows less one, exactly and plus one, a
    narrower topic, a topic whose every row is an orphan) under the same plan flag words: steps of 64, 128 and 256 rows, the order
    kernel of its own and beside first fit in one workgroup, the sampled verification, int32 and 16-bit cells — the kernel each
    word names, and the lists against the oracle."""
    from kafka_assigner_amd.flatten import index_form
    from test_emu_parity import relax_step_edge_cases
    ctx = native.default_context()
    fb, flag_words = relax_step_edge_cases()
    want = oracle_solve(fb)
    assert (want.topic_results["status"] == abi.KAS_OK).all()
    # (as the emulator does for a word that names no place for first fit: kas_p4_kernel, so that the order kernel of its own runs
    # too — by itself a batch this small takes kas_p4_order_kernel under every word)
    own_p4 = lambda flags: flags if flags & abi.KAS_PLAN_P4_WITH_ORDER else flags | abi.KAS_PLAN_SPLIT_P4
    for flags in map(own_p4, flag_words):
        plan = native.Plan(ctx, fb)
        plan.set_flags(flags)
        what = plan.describe()
        plan.close()
        rows = 64 << (((flags >> 17) & 3) - 1)
        assert "tiles of %d rows" % rows in what, (hex(flags), what)
        assert ("kas_p4_order_kernel<3>" in what) == ((flags & abi.KAS_PLAN_P4_WITH_ORDER) == abi.KAS_PLAN_P4_WITH_ORDER), (hex(flags), what)
        assert ("sampled verification" in what) == (flags >> 24 != 0) and ("dword mid rows" in what) == (not flags & abi.KAS_PLAN_NO_MID32), (hex(flags), what)
        got = native.solve_host_with_flags(fb, flags, ctx)
        assert_same_outputs(fb, want, got, f"hip relaxation steps at their edges, plan flags {flags:#x}")
        assert (got.scenario_results["status"] == abi.KAS_OK).all(), hex(flags)
    want16 = oracle_solve(index_form(fb))
    want16.out = np.where(want16.out < 0, 0xFFFF, want16.out).astype(np.uint16)
    for flags in map(own_p4, (TILES_64, TILES_128)):
        got16 = native.solve_device16_with_flags(fb, flags, ctx)
        assert "[16-bit cells]" in got16.describe and "tiles of %d rows" % (64 if flags & TILES_128 == 0 else 128) in got16.describe, got16.describe
        assert_same_outputs(fb, want16, got16, f"hip relaxation steps at their edges, 16-bit cells, plan flags {flags:#x}")


def test_hip_rack_awareness_disabled_cyclic_and_sparse_ids():
    fb = _batch(99, 4, 1500, 50, 10, 3, G.ACTIONS, rack_aware=False)
    assert_same_outputs(fb, oracle_solve(fb), native.solve_host(fb), "hip norack")
    fb = _batch(7, 4, 1200, 60, 6, 3, ("add_k", "remove1"), cyclic=True)
    assert_same_outputs(fb, oracle_solve(fb), native.solve_host(fb), "hip cyclic")
    cur = G.random_assignment(5, 500, 20, 5, 3).astype(np.int64) * 100003 + 7
    ids = (np.arange(20, dtype=np.int64) * 100003 + 7).astype(np.int32)[None, :]
    racks = (np.arange(20) % 5).astype(np.int32)[None, :]
    fb = uniform_batch(cur.astype(np.int32)[None], ids[:, :19], racks[:, :19], 3)
    assert_same_outputs(fb, oracle_solve(fb), native.solve_host(fb), "hip sparse")


def test_config2_single_scenario_10k_partitions_decommission_one():
    """BASELINE.json config 2: 10k partitions x 100 brokers x 10 racks, RF 3, remove 1 broker."""
    for seed_ in (0, 1, 2, 3):
        cur = G.random_assignment(seed_, 10000, 100, 10, 3)
        bs = G.perturb_brokers(100, 10, remove=[seed_ % 100])
        fb = uniform_batch(cur[None], bs.node_id[None], bs.node_rack[None], 3)
        assert_same_outputs(fb, oracle_solve(fb), native.solve_host(fb), f"C2 seed {seed_}")


def test_config3_shape_full_size_scenarios():
    """BASELINE.json config 3 shape (100k partitions x 1k brokers x 20 racks, RF 3): a handful
    of full-size scenarios list-compared against the oracle, every action kind."""
    fb = _batch(2024, 8, 100000, 1000, 20, 3, G.ACTIONS)
    want = oracle_solve(fb)
    got = native.solve_host(fb)
    assert_same_outputs(fb, want, got, "C3")
    assert_same_outputs(fb, want, native.solve_host_with_flags(fb, TILES_64), "C3 relaxation form over tiles of 64 rows (what a batch of 1000 takes)")
    assert_same_outputs(fb, want, native.solve_host_with_flags(fb, TICKET_ORDER), "C3 ticket form")
    assert_same_outputs(fb, want, native.solve_host_with_flags(fb, abi.KAS_PLAN_NO_RTN_QUOTA), "C3 quota drawn without the atomic-with-return")
    assert_same_outputs(fb, want, native.solve_host_with_flags(fb, abi.KAS_PLAN_NO_INDEX_ROWS), "C3 cur read by both row scans (no index rows)")
    assert_same_outputs(fb, want, native.solve_host_with_flags(fb, abi.KAS_PLAN_INDEX_ROWS), "C3 index rows (cur read once)")
    assert_same_outputs(fb, want, native.solve_host_with_flags(fb, abi.KAS_PLAN_P4_WITH_ORDER), "C3 first fit as a wavefront of the order kernel's workgroup")
    assert_same_outputs(fb, want, native.solve_host_with_flags(fb, abi.KAS_PLAN_P4_WITH_ORDER | TILES_64), "C3 kas_p4_order_kernel, tiles of 64 rows")
    assert_same_outputs(fb, want, native.solve_host_with_flags(fb, abi.KAS_PLAN_SPLIT_P4 | TILES_64), "C3 kas_p4_kernel + tiles of 64 rows (the headline's kernels)")
    assert_same_outputs(fb, want, native.solve_host_with_flags(fb, 1), "C3 generic fill")
    assert_same_outputs(fb, want, native.solve_host_with_flags(fb, 2), "C3 round order")
    assert_same_outputs(fb, want, native.solve_host_with_flags(fb, 4), "C3 4 x uint16 counter rows")
    assert_same_outputs(fb, want, native.solve_host_with_flags(fb, 8), "C3 chunk-count pass instead of per-chunk histograms")
    for nw, g in ((1, 1), (2, 2), (4, 1)):     # 4 scenarios per wave do not fit 16-bit LDS offsets at N = 1000
        assert_same_outputs(fb, want, native.solve_host_with_flags(fb, (nw << 8) | (g << 12)),
                            f"C3 {nw} waves, {g} scenarios per wave")
    assert (want.scenario_results["status"] == abi.KAS_OK).sum() >= 4


def test_config5_shape_rf5_rack_on_and_off_scaled():
    """BASELINE.json config 5 shape scaled to one GPU test: RF 5, 40 racks, mixed add+remove
    broker set, rack awareness on and off (--disable_rack_awareness)."""
    P, N, R, RF = 200000, 1000, 40, 5
    cur = G.random_assignment(7, P, N, R, RF)
    for rack_aware in (True, False):
        bs = G.perturb_brokers(N, R, remove=list(range(0, N, 50)), add=40, rack_aware=rack_aware)
        fb = uniform_batch(cur[None], bs.node_id[None], bs.node_rack[None], RF)
        assert_same_outputs(fb, oracle_solve(fb), native.solve_host(fb), f"C5 rack_aware={rack_aware}")


def test_wide_lists_relaxation_form_on_the_gpu():
    """Round 6: the relaxation form for lists 4 and 5 wide (kas_order_relax_wide.h), KAS_PLAN_RELAX_TILES(1) at these widths — built
    and measured because VERDICT r5 asked for a measurement instead of DESIGN's estimate (it is slower than the wide ticket form at
    configs[4]: profiles/r06_ab_config5_relaxation_form.log), so it is opt-in; exact all the same."""
    P, N, R = 200000, 1000, 40
    for RF in (5, 4):
        cur = G.random_assignment(7, P, N, R, RF)
        sets = [G.perturb_brokers(N, R, remove=list(range(k, N, 50)), add=40, rack_aware=(k % 2 == 0)) for k in range(4)]
        fb = uniform_batch(np.stack([cur] * 4), np.stack([b.node_id for b in sets]), np.stack([b.node_rack for b in sets]), RF)
        want = oracle_solve(fb, threads=0)
        assert (want.scenario_results["status"] == abi.KAS_OK).any()
        plan = native.Plan(native.default_context(), fb)
        plan.set_flags(TILES_64)
        assert f"kas_order_relax_wide_kernel<{RF}>[tiles of 64 rows, ids in LDS]" in plan.describe(), plan.describe()
        plan.set_flags(0)
        assert f"kas_order_wide_kernel<{RF}>" in plan.describe(), plan.describe()
        plan.close()
        assert_same_outputs(fb, want, native.solve_host_with_flags(fb, TILES_64), f"hip relaxation form, lists {RF} wide")
        assert_same_outputs(fb, want, native.solve_host_with_flags(fb, TILES_64 | abi.KAS_PLAN_FILL_WITH_P4), f"hip relaxation form, lists {RF} wide, first fit inside the fill workgroup")
    fb = _multi_topic_scenarios(91, 4, 3, 900, 60, 12, 5)
    assert_same_outputs(fb, oracle_solve(fb), native.solve_host_with_flags(fb, TILES_64), "hip relaxation form, lists 5 wide, topics of one scenario sharing the counters")


def test_config4_exact_action_add_brokers_1000_to_1049_full_size():
    """BASELINE.json configs[3]'s exact action at full size: 100k partitions x 1k brokers x 20
    racks, RF 3, add brokers 1000-1049 (rack id mod 20) -> N = 1050, cap 286; 64 scenarios with
    their own G(seed+s) tables — one GPU's slice of the 64k — every list compared."""
    fb = _batch(4004, 64, 100000, 1000, 20, 3, ("add50",))
    assert (fb.scen["n_nodes"] == 1050).all()
    want = oracle_solve(fb, threads=0)
    assert (want.scenario_results["status"] == abi.KAS_OK).all()
    assert (want.scenario_results["moved_replicas"] > 10000).all()      # 14k-16k orphans each
    assert_same_outputs(fb, want, native.solve_host(fb), "C4 add 50")
    assert_same_outputs(fb, want, native.solve_host_with_flags(fb, TILES_64), "C4 add 50, tiles of 64 rows")


def test_config5_full_size_1m_partitions_5k_brokers_rf5_rack_on_and_off():
    """BASELINE.json configs[4] at its stated size: 1M partitions x 5k brokers x 40 racks, RF 5,
    remove every 50th broker + add 5000-5199, rack map as generated and empty
    (--disable_rack_awareness): N = 5100, cap 981, ~219k moved replicas.  Every list compared."""
    P, N, R, RF = 1000000, 5000, 40, 5
    cur = G.random_assignment(7, P, N, R, RF)
    for rack_aware in (True, False):
        bs = G.perturb_brokers(N, R, remove=list(range(0, N, 50)), add=200, rack_aware=rack_aware)
        assert bs.node_id.shape[0] == 5100
        fb = uniform_batch(cur[None], bs.node_id[None], bs.node_rack[None], RF)
        want = oracle_solve(fb)
        assert want.scenario_results["status"][0] == abi.KAS_OK
        assert want.scenario_results["moved_replicas"][0] > 200000
        assert_same_outputs(fb, want, native.solve_host(fb), f"C5 full size rack_aware={rack_aware}")


def test_one_plan_orders_its_solves_across_streams():
    """A plan owns the scratch of one solve (include/kas_abi.h): solves of one plan enqueued on
    different streams must not overlap.  Alternate two streams without any host synchronisation in
    between and compare every result."""
    import torch
    fb = _batch(515, 24, 20000, 200, 10, 3, G.ACTIONS)
    want = oracle_solve(fb, threads=0)
    ctx = native.default_context()
    plan = native.Plan(ctx, fb)
    assert "kas_fill_kernel<3,4>[quota, chunk histograms" in plan.describe() and "kas_order_relax_kernel<3>" in plan.describe()
    assert "kas_p4_kernel" not in plan.describe()                                   # 24 scenarios: first fit inside the fill workgroup
    dev = torch.device("cuda", ctx.device)
    d_cur = torch.from_numpy(fb.cur).to(dev)
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    outs = []
    for i in range(6):
        d_out = torch.full((fb.out_len,), -7, dtype=torch.int32, device=dev)
        d_tr = torch.zeros(fb.n_topics * 16, dtype=torch.uint8, device=dev)
        d_sr = torch.zeros(fb.n_scenarios * 32, dtype=torch.uint8, device=dev)
        streams[i % 2].wait_stream(torch.cuda.current_stream(dev))
        plan.solve_device(d_cur.data_ptr(), d_out.data_ptr(), d_tr.data_ptr(), d_sr.data_ptr(),
                          stream=streams[i % 2].cuda_stream)
        outs.append((d_out, d_sr))
    torch.cuda.synchronize(dev)
    for d_out, d_sr in outs:
        np.testing.assert_array_equal(d_out.cpu().numpy(), want.out[:fb.out_len])
        sr = d_sr.cpu().numpy().view(abi.SCENARIO_RESULT_DTYPE)
        np.testing.assert_array_equal(sr["digest"], want.scenario_results["digest"])
    plan.set_flags(2)
    assert "kas_order_round_kernel<3>" in plan.describe()
    plan.set_flags(TICKET_ORDER)
    assert "kas_order_ticket_kernel<3,2,true>" in plan.describe()
    plan.set_flags(0)
    assert "kas_order_relax_kernel<3>[tiles of 128 rows" in plan.describe()      # 24 scenarios: a latency-bound launch
    plan.set_flags(TILES_64)
    assert "kas_order_relax_kernel<3>[tiles of 64 rows" in plan.describe()
    plan.set_flags(abi.KAS_PLAN_SPLIT_P4)
    assert "+ kas_p4_kernel<3> grid=24x64" in plan.describe()                       # a launch of its own, one wavefront per scenario
    plan.set_flags(abi.KAS_PLAN_FILL_WITH_P4)
    assert "kas_p4_kernel" not in plan.describe()
    plan.close()


def test_host_path_reuses_buffers_and_plans_across_calls():
    """kas_solve_host on one context: the device buffers only grow, the plan of a batch that comes
    again byte for byte is reused, and a batch of a known shape with OTHER broker sets (what a what-if
    caller sends on every call) rebuilds such a plan in place over the scratch it owns — no device
    allocation either way (include/kas_abi.h).  Results stay the oracle's on every call."""
    ctx = native.DeviceContext(0)
    fb = _batch(91, 5, 4000, 80, 8, 3, G.ACTIONS)
    want = oracle_solve(fb)
    for _ in range(3):
        assert_same_outputs(fb, want, native.solve_host(fb, ctx), "host path, same batch")
    calls, hits, allocs = ctx.host_stats()
    assert (calls, hits) == (3, 2) and allocs > 0
    big = _batch(92, 9, 9000, 120, 12, 3, G.ACTIONS)
    assert_same_outputs(big, oracle_solve(big), native.solve_host(big, ctx), "host path, bigger batch")
    calls2, hits2, allocs2 = ctx.host_stats()
    assert hits2 == 2 and allocs2 > allocs                   # new shape: new plan, buffers grown
    assert_same_outputs(fb, want, native.solve_host(fb, ctx), "host path, first batch again")
    assert ctx.host_stats() == (5, 3, allocs2)               # cached plan hit; nothing had to grow
    # same shape (scenario count, topic descriptors), other broker sets: rebuilt in place
    for seed_ in (191, 192, 193):
        other = _batch(seed_, 5, 4000, 80, 8, 3, ("remove1",))
        other.cur = fb.cur; other.topics = fb.topics
        if other.node_id.size > fb.node_id.size:
            continue                                         # (a larger node pool may grow a buffer: not this test's point)
        assert_same_outputs(other, oracle_solve(other), native.solve_host(other, ctx), "host path, other broker sets")
        assert ctx.host_stats()[1:] == (3, allocs2)          # a miss, and yet no allocation
    fb5 = _batch(93, 3, 2000, 60, 12, 5, G.ACTIONS)          # other width class: a new plan
    assert_same_outputs(fb5, oracle_solve(fb5), native.solve_host(fb5, ctx), "host path, RF 5")
    assert ctx.host_stats()[2] > allocs2
    ctx.close()


def test_host_path_what_if_select_returns_every_record_and_the_selected_rows():
    """kas_solve_host_select (KAG:131-187: many broker sets over one snapshot, ONE assignment printed):
    records of every variant, rows of the selected ones only, packed in selection order; n_select = 0
    needs no out buffer at all."""
    P, N, R, RF, S = 30000, 300, 10, 3, 40
    fb = _batch(41, S, P, N, R, RF, G.BENCH_ACTIONS)
    fb.cur = G.random_assignment(41, P, N, R, RF).reshape(-1).copy()     # one shared table ...
    fb.topics["cur_off"] = 0                                             # ... read by every variant
    want = oracle_solve(fb, threads=0)
    ctx = native.DeviceContext(0)
    cells = P * RF
    for select in ([7], [39, 0, 12], []):
        got = native.solve_host_select(fb, select, ctx)
        for f in ("status", "fail_topic", "fail_partition", "moved_replicas", "moved_partitions", "digest"):
            np.testing.assert_array_equal(got.scenario_results[f][:S], want.scenario_results[f][:S])
        for f in ("status", "fail_partition", "moved_replicas", "moved_partitions"):
            np.testing.assert_array_equal(got.topic_results[f][:S], want.topic_results[f][:S])
        for k, s_ in enumerate(select):
            np.testing.assert_array_equal(got.out[k * cells:(k + 1) * cells], want.out[s_ * cells:(s_ + 1) * cells])
    with pytest.raises(native.KasError):
        native.solve_host_select(fb, [S], ctx)
    ctx.close()


def test_host_path_cuts_large_tables_into_overlapping_scenario_ranges_and_takes_pinned_memory():
    """Tables of 48 MB and more laid out scenario by scenario are moved and solved as up to three
    scenario ranges (upload / solve / download overlapping, each on streams of its own); the result must not depend
    on it, nor on whether the caller's pools are pageable or pinned (kas_host_alloc)."""
    from kafka_assigner_amd.flatten import host_tables
    import ctypes as C
    fb = _batch(2025, 44, 100000, 1000, 20, 3, G.BENCH_ACTIONS)          # 52.8 MB in, 52.8 MB out
    want = oracle_solve(fb, threads=0)
    ctx = native.DeviceContext(0)
    assert_same_outputs(fb, want, native.solve_host(fb, ctx), "host path, split into ranges (pageable)")
    calls, hits, allocs = ctx.host_stats()
    assert_same_outputs(fb, want, native.solve_host(fb, ctx), "host path, split into ranges, again")
    assert ctx.host_stats() == (calls + 1, hits + 3, allocs)             # three ranges, three cached plans, nothing grown
    pin_cur, pin_out = native.PinnedArray(fb.cur.size), native.PinnedArray(fb.out_len)
    pin_cur.array[:] = fb.cur
    pin_out.array[:] = -9
    t, ho = host_tables(fb)
    t.cur = pin_cur.array.ctypes.data; t.out = pin_out.array.ctypes.data
    native._check(native.load().kas_solve_host(ctx._h, C.byref(native.batch_desc(fb)), C.byref(t)))
    ho.out = pin_out.array.copy()
    assert_same_outputs(fb, want, ho, "host path, pinned pools")
    pin_cur.close(); pin_out.close()
    ctx.close()


def test_host_path_sharded_over_two_contexts_and_the_slice_helper():
    """kas_solve_host_sharded: contiguous scenario ranges (kas_shard_range) on several contexts, one
    host thread each — here two contexts on the one device of the test box, multi-topic scenarios with
    and without a Context, an odd scenario count.  Same results as one call; and kas_shard_range agrees
    with sharding.shard_range."""
    from kafka_assigner_amd import sharding
    for total, world in ((0, 3), (7, 3), (8, 8), (1000, 8), (5, 8)):
        for r in range(world):
            assert native.shard_range(total, r, world) == tuple(sharding.shard_range(total, r, world))
    fb = _multi_topic_scenarios(55, 7, 3, 3000, 60, 12, 3)
    fb.scen["ctx_width"][::2] = 8                                         # every other scenario hands a Context in
    off = 0
    for s in range(fb.n_scenarios):
        if fb.scen["ctx_width"][s]:
            fb.scen["ctx_off"][s] = off
            off += 8 * int(fb.scen["n_nodes"][s])
    fb.ctx = np.random.default_rng(3).integers(0, 50, size=off).astype(np.int32)
    want = oracle_solve(fb)
    a, b = native.DeviceContext(0), native.DeviceContext(0)
    got = native.solve_host_sharded(fb, [a, b])
    assert_same_outputs(fb, want, got, "sharded over two contexts")
    assert a.host_stats()[0] == 1 and b.host_stats()[0] == 1
    a.close(); b.close()


def test_host_path_sharded_over_eight_contexts_ragged_and_overlapping_extents():
    """The node's shape without the node: eight contexts (on the one device of the test box), 13 scenarios — shards of
    2, 2, 2, 2, 2, 1, 1, 1 — and, second, a batch whose `out` pool is NOT laid out in scenario order (scenario s writes
    behind scenario s + 1): the shards' download extents overlap, and the call must solve it on one context instead of
    letting one shard's download overwrite another's rows."""
    ctxs = [native.DeviceContext(0) for _ in range(8)]
    fb = _batch(808, 13, 4000, 60, 6, 3, G.ACTIONS)
    want = oracle_solve(fb)
    got = native.solve_host_sharded(fb, ctxs)
    assert_same_outputs(fb, want, got, "sharded over eight contexts, 13 scenarios")
    assert sorted(c.host_stats()[0] for c in ctxs) == [1] * 8
    # out regions in reverse scenario order
    fb2 = _batch(809, 6, 3000, 50, 5, 3, G.ACTIONS)
    P, W = 3000, 3
    fb2.topics["out_off"] = ((fb2.n_scenarios - 1 - np.arange(fb2.n_scenarios)) * P * W).astype(np.int64)
    want2 = oracle_solve(fb2)
    got2 = native.solve_host_sharded(fb2, ctxs)
    assert_same_outputs(fb2, want2, got2, "sharded call, out pool not in scenario order")
    calls = sorted(c.host_stats()[0] for c in ctxs)
    assert calls == [1] * 7 + [2], calls                                  # one context took the whole second batch
    for c in ctxs:
        c.close()


@pytest.mark.parametrize("P,N,R,RF,kernel", [(30000, 300, 10, 3, "kas_order_ticket_kernel<3,2,false>"),
                                             (9000, 120, 12, 5, "kas_order_wide_kernel<5>"),
                                             (5000, 80, 8, 2, "kas_order_ticket_kernel<2,2,false>")])
def test_ticket_forms_take_a_context_in_and_hand_it_back(P, N, R, RF, kernel):
    """KAS:59-62 / KTA:19-23: the reference hands its Context to EVERY call.  With one the plan keeps the
    ticket kernels (count fields seeded from the counters, written back at the end); scenarios whose
    counters do not fit the fields are flagged on the device and solved by the round form behind them."""
    from test_emu_parity import _random_counters, _with_context
    fb = _with_context(_batch(606 + RF, 6, P, N, R, RF, G.BENCH_ACTIONS), _random_counters(7, 90))
    plan = native.Plan(native.default_context(), fb)
    if RF <= 3:
        # round 4: by itself the plan takes the relaxation form with a Context too; the ticket form when asked
        assert f"kas_order_relax_kernel<{RF}>" in plan.describe() and "Context in/out" in plan.describe(), plan.describe()
        plan.set_flags(TICKET_ORDER)
    assert kernel in plan.describe() and "Context in/out" in plan.describe(), plan.describe()
    plan.close()
    want = oracle_solve(fb, threads=0)
    got = native.solve_host_with_flags(fb, TICKET_ORDER) if RF <= 3 else native.solve_host(fb)
    assert_same_outputs(fb, want, got, "hip ticket form with a Context")
    assert (got.ctx != fb.ctx).any()
    assert_same_outputs(fb, want, native.solve_host_with_flags(fb, 2), "hip round form with the same Context")
    if RF <= 3:
        for flags, what in ((0, "by batch size"), (TILES_64, "tiles of 64 rows"), (TILES_128, "double tiles")):
            got = native.solve_host_with_flags(fb, flags) if flags else native.solve_host(fb)
            assert_same_outputs(fb, want, got, f"hip relaxation form with a Context, {what}")
            np.testing.assert_array_equal(got.ctx.reshape(-1, 8)[:, RF:], fb.ctx.reshape(-1, 8)[:, RF:])

    def big(s, n):
        v = np.random.default_rng(s).integers(0, 200, size=(n, 8))
        if s in (1, 4): v[n // 3, s % RF] = 65535 if RF <= 3 else 1020
        if s == 2: v[0, 0] = -1
        return v
    fb = _with_context(_batch(707 + RF, 6, P, N, R, RF, G.BENCH_ACTIONS), big)
    want = oracle_solve(fb, threads=0)
    assert_same_outputs(fb, want, native.solve_host(fb), "hip, three scenarios flagged for the round form")
    if RF <= 3:
        assert_same_outputs(fb, want, native.solve_host_with_flags(fb, TICKET_ORDER), "hip ticket form, three scenarios flagged for the round form")

        def big12(s, n):                                                 # the relaxation form's 16-bit fields
            v = np.random.default_rng(s).integers(0, 200, size=(n, 8))
            if s in (0, 3): v[n // 3, s % 2] = 65535 - 20                # + the rows to come: over
            if s == 1: v[n // 4, 0] = 4095; v[n // 4 + 1, 1] = 30000     # (inside the fields: stays in the relaxation form)
            if s == 5: v[7, 2] = 1 << 29                                 # column 2 is no field: stays in the relaxation form
            return v
        fb = _with_context(_batch(808 + RF, 6, P, N, R, RF, G.BENCH_ACTIONS), big12)
        assert_same_outputs(fb, oracle_solve(fb, threads=0), native.solve_host(fb), "hip relaxation form, two scenarios flagged for the round form")


def test_wide_lists_a_broker_holding_1023_rows_or_more_keeps_the_wide_ticket_form_and_its_counts_are_checked():
    """Round 3: lists 4-5 wide and a broker that may hold 1,023 .. 2,039 rows of the scenario used
    to drop to the one-wavefront round form.  The wide form now runs and checks its count fields when the last row
    has retired; a scenario whose counts outgrew them (here: every row of a broker at list position 0) is filled and
    ordered again behind it."""
    from test_emu_parity import _wide_batch_whose_counts_outgrow_the_fields
    fb = _batch(31, 1, 4600, 20, 10, 5, ("add_k",), rack_aware=False)      # 1,046 rows per broker, <= 360 per position
    plan = native.Plan(native.default_context(), fb)
    assert "kas_order_wide_kernel<5>" in plan.describe() and "count fields checked" in plan.describe(), plan.describe()
    plan.close()
    assert_same_outputs(fb, oracle_solve(fb), native.solve_host(fb), "hip wide form, 1046 rows per broker")
    fb, P, W = _wide_batch_whose_counts_outgrow_the_fields()
    want = oracle_solve(fb)
    assert np.bincount(want.out[:P * W].reshape(P, W)[:, 0]).max() >= 1024
    for rep in range(3):
        assert_same_outputs(fb, want, native.solve_host(fb), "hip wide form, count[.][0] beyond 1023 (solved again)")
    # the same at a size where the node tables matter: 1.1M partitions would be BASELINE configs[4] with cap 1,100;
    # scaled to 1/10 of the brokers
    fb = _batch(11, 1, 110000, 500, 40, 5, ("c5",))
    plan = native.Plan(native.default_context(), fb)
    assert "kas_order_wide_kernel<5>" in plan.describe() and "count fields checked" in plan.describe(), plan.describe()
    plan.close()
    assert_same_outputs(fb, oracle_solve(fb), native.solve_host(fb), "hip wide form, 110k x 500 x RF 5 (cap 1100)")


@pytest.mark.parametrize("N,P", [(9000, 40000), (12000, 60000)])
def test_lists_3_wide_beyond_8191_brokers_take_the_relaxation_form(N, P):
    """Round 4: the relaxation form keeps 4 B of LDS per broker and has no 16-bit LDS offsets, so lists <= 3 wide
    without a Context are served up to where the fill kernel's LDS ends (13,492 brokers); rounds 1-3 refused these
    shapes (KAS_E_UNSUPPORTED).  KAS_PLAN_TICKET_ORDER changes nothing there: no ticket form applies."""
    fb = _batch(4243, 3, P, N, 25, 3, ("add_k", "mixed", "remove_k"))
    plan = native.Plan(native.default_context(), fb)
    assert "kas_order_relax_kernel<3>" in plan.describe(), plan.describe()
    plan.set_flags(TICKET_ORDER)
    assert "kas_order_relax_kernel<3>" in plan.describe(), plan.describe()
    plan.close()
    want = oracle_solve(fb, threads=0)
    assert (want.scenario_results["status"] == abi.KAS_OK).any()
    assert_same_outputs(fb, want, native.solve_host(fb), f"hip relaxation form, {N} brokers")
    assert_same_outputs(fb, want, native.solve_host_with_flags(fb, 1), f"hip general fill + relaxation form, {N} brokers")


@pytest.mark.parametrize("N,P", [(5000, 200000), (7400, 60000)])
def test_lists_3_wide_keep_the_ticket_form_up_to_8191_brokers(N, P):
    """Round 3: one scenario per solver wavefront is limited by where its counter rows end (8 B per broker below
    64 KiB): 5,000 brokers x RF 3 used to take the one-wavefront round form (4,680 was the limit), and from 6,800
    brokers on nothing served the shape."""
    fb = _batch(4242, 4, P, N, 25, 3, ("add_k", "mixed"))
    plan = native.Plan(native.default_context(), fb)
    assert "kas_order_relax_kernel<3>" in plan.describe(), plan.describe()
    plan.set_flags(TICKET_ORDER)
    assert "kas_order_ticket_kernel<3,1," in plan.describe(), plan.describe()
    plan.close()
    want = oracle_solve(fb, threads=0)
    assert (want.scenario_results["status"] == abi.KAS_OK).all()
    assert_same_outputs(fb, want, native.solve_host(fb), f"hip relaxation form, {N} brokers")
    assert_same_outputs(fb, want, native.solve_host_with_flags(fb, TICKET_ORDER), f"hip ticket form, {N} brokers")
    if N == 5000:
        assert_same_outputs(fb, want, native.solve_host_with_flags(fb, 2), "hip round form, 5000 brokers")


def test_1_1m_partitions_5k_brokers_rf5_keeps_the_wide_ticket_form():
    """The shape VERDICT round 2 named (1.1M x 5k, RF 5: a broker holds up to 1,079 rows — beyond the 10-bit bound of
    the wide form's count fields, which sent it to the one-wavefront round form, seconds per scenario): at full size,
    every list compared."""
    P, N, R, RF = 1100000, 5000, 40, 5
    cur = G.random_assignment(9, P, N, R, RF)
    bs = G.perturb_brokers(N, R, remove=list(range(0, N, 50)), add=200, rack_aware=True)
    fb = uniform_batch(cur[None], bs.node_id[None], bs.node_rack[None], RF)
    plan = native.Plan(native.default_context(), fb)
    assert "kas_order_wide_kernel<5>" in plan.describe() and "count fields checked" in plan.describe(), plan.describe()
    plan.close()
    want = oracle_solve(fb)
    assert want.scenario_results["status"][0] == abi.KAS_OK
    assert np.bincount(want.out.reshape(-1)).max() >= 1023
    import time
    got = native.solve_host(fb)                                       # (first call: plan, buffers)
    t0 = time.perf_counter()
    got = native.solve_host(fb)
    dt = time.perf_counter() - t0
    assert_same_outputs(fb, want, got, "1.1M x 5k x RF 5")
    assert dt < 1.0, f"1.1M x 5k x RF 5 took {dt:.3f} s through the host path: not the wide form?"


def test_topic_without_rows_next_to_full_width_topics():
    """A topic with zero partitions whose widths match the kernel's width class (the fast fill's
    full-row loads must not touch a table that has no rows), at the very end of the cur pool."""
    cur = G.cyclic_assignment(300, 12, 3)                # balanced and rack-diverse: topic a succeeds
    sc = Scenario(brokers=list(range(12)), racks={b: "r%d" % (b % 4) for b in range(12)},
                  topics=[Topic("a", {p: cur[p].tolist() for p in range(300)}, 3),
                          Topic("empty", {}, 3)])
    fb = flatten([sc])
    fb.topics["cur_width"][1] = 3; fb.topics["out_width"][1] = 3        # same width class, no rows
    assert_same_outputs(fb, oracle_solve(fb), native.solve_host(fb), "empty topic last")


def test_multi_topic_scenarios_without_context_io_use_cross_topic_tickets():
    """Three topics per scenario sharing one Context that is neither handed in nor out (one
    PRINT_REASSIGNMENT run, KAG:172-184): the ticket form carries the tickets across topics."""
    fb = _multi_topic_scenarios(77, 6, 3, 5000, 120, 12, 3)
    want = oracle_solve(fb)
    assert (want.topic_results["status"] == abi.KAS_OK).sum() >= 6
    assert_same_outputs(fb, want, native.solve_host(fb), "hip multi-topic, relaxation form")
    assert_same_outputs(fb, want, native.solve_host_with_flags(fb, TICKET_ORDER), "hip multi-topic tickets")
    assert_same_outputs(fb, want, native.solve_host_with_flags(fb, TILES_64), "hip multi-topic, relaxation form over tiles of 64 rows")
    assert_same_outputs(fb, want, native.solve_host_with_flags(fb, 2), "hip multi-topic rounds")
    assert_same_outputs(fb, want, native.solve_host_with_flags(fb, 2 << 12), "hip multi-topic, 2 scenarios per wave")


def test_config5_full_broker_count_rf5():
    """BASELINE.json configs[4] at its full broker count (5k brokers x 40 racks, RF 5, remove every
    50th broker + add 200), 200k partitions: general sticky fill (no LDS for the histogram at this
    size) + round form of P5, list-compared with the oracle, rack awareness on and off."""
    P, N, R, RF = 200000, 5000, 40, 5
    cur = G.random_assignment(7, P, N, R, RF)
    for rack_aware in (True, False):
        bs = G.perturb_brokers(N, R, remove=list(range(0, N, 50)), add=200, rack_aware=rack_aware)
        fb = uniform_batch(cur[None], bs.node_id[None], bs.node_rack[None], RF)
        assert_same_outputs(fb, oracle_solve(fb), native.solve_host(fb), f"C5 N=5100 rack_aware={rack_aware}")


def test_device_resident_tables_and_what_if_shared_cur():
    """kas_solve_device with torch-owned HBM tables, and the what-if layout: many broker-set
    variants over ONE shared current assignment (SURVEY.md 8d, C4 'shared base cur')."""
    import torch
    P, N, R, RF, S = 20000, 200, 10, 3, 16
    cur = G.random_assignment(11, P, N, R, RF)
    fb = _batch(11, S, P, N, R, RF, G.ACTIONS)          # shapes/descriptors
    fb.cur = cur.reshape(-1).copy()                      # one shared table ...
    fb.topics["cur_off"] = 0                             # ... read by every scenario
    want = oracle_solve(fb)
    ctx = native.default_context()
    plan = native.Plan(ctx, fb)
    dev = torch.device("cuda", ctx.device)
    d_cur = torch.from_numpy(fb.cur).to(dev)
    d_out = torch.full((fb.out_len,), -7, dtype=torch.int32, device=dev)
    d_tr = torch.zeros(fb.n_topics * 16, dtype=torch.uint8, device=dev)
    d_sr = torch.zeros(fb.n_scenarios * 32, dtype=torch.uint8, device=dev)
    # a real (non-default) stream: handle 0 would mean "the context's own stream"
    st = torch.cuda.Stream(dev)
    st.wait_stream(torch.cuda.current_stream(dev))
    assert st.cuda_stream != 0
    plan.solve_device(d_cur.data_ptr(), d_out.data_ptr(), d_tr.data_ptr(), d_sr.data_ptr(),
                      stream=st.cuda_stream)
    st.synchronize()
    out = d_out.cpu().numpy()
    tr = d_tr.cpu().numpy().view(abi.TOPIC_RESULT_DTYPE)
    sr = d_sr.cpu().numpy().view(abi.SCENARIO_RESULT_DTYPE)
    np.testing.assert_array_equal(out, want.out[:fb.out_len])
    for f in ("status", "fail_partition", "moved_replicas", "moved_partitions"):
        np.testing.assert_array_equal(tr[f], want.topic_results[f])
    np.testing.assert_array_equal(sr["digest"], want.scenario_results["digest"])
    avg_us, n = plan.kernel_time_us()
    assert n == 1 and avg_us > 0
    assert plan.algorithmic_bytes == fb.algorithmic_bytes()
    stats = plan.stats()
    ok = sr["status"] == abi.KAS_OK
    # relaxation form: evaluations ([9]) and tiles ([12]) per scenario — a handful of evaluations per 64-row tile
    assert stats.shape == (S, 16) and (stats[:, 1] > 0).all() and ok.any()
    assert (stats[ok, 12] == (P + 63) // 64).all() and (stats[ok, 9] >= 2 * stats[ok, 12]).all() and (stats[ok, 9] < 12 * stats[ok, 12]).all()
    # the ticket form decides rows inside queues (rows waiting in line on one node commit together):
    # its parity run covers that path, not only the one-row-per-step path
    plan.set_flags(TICKET_ORDER)
    d_out.fill_(-7)
    plan.solve_device(d_cur.data_ptr(), d_out.data_ptr(), d_tr.data_ptr(), d_sr.data_ptr(), stream=st.cuda_stream)
    st.synchronize()
    np.testing.assert_array_equal(d_out.cpu().numpy(), want.out[:fb.out_len])
    stats = plan.stats()
    assert (stats[:, 9] > 0).all() and (stats[ok, 14] > 0).any() and (stats[ok, 6] > 0).any()
    plan.close()


def test_idempotent_on_own_output():
    """Size-independent property: feeding a successful result back in as the current
    assignment (same brokers) moves no replica."""
    P, N, R, RF = 50000, 500, 20, 3
    cur = G.random_assignment(3, P, N, R, RF)
    bs = G.perturb_brokers(N, R, remove=[17])
    fb = uniform_batch(cur[None], bs.node_id[None], bs.node_rack[None], RF)
    first = native.solve_host(fb)
    assert first.scenario_results["status"][0] == abi.KAS_OK
    fb2 = uniform_batch(first.out[:P * RF].reshape(1, P, RF), bs.node_id[None], bs.node_rack[None], RF)
    second = native.solve_host(fb2)
    assert second.scenario_results["status"][0] == abi.KAS_OK
    assert second.scenario_results["moved_replicas"][0] == 0
    assert second.scenario_results["moved_partitions"][0] == 0
    # and the invariants of KafkaTopicAssignerTest.java:159-187 at full size
    new = second.out[:P * RF].reshape(P, RF)
    assert (np.sort(new, axis=1)[:, 1:] != np.sort(new, axis=1)[:, :-1]).all()   # no broker twice
    loads = np.bincount(new.reshape(-1), minlength=N)
    assert loads.max() <= -(-P * RF // bs.node_id.shape[0])                       # <= cap
    racks = new % R
    assert (np.sort(racks, axis=1)[:, 1:] != np.sort(racks, axis=1)[:, :-1]).all()  # distinct racks


@pytest.mark.gpu
def test_solves_in_flight_leave_identical_records_for_every_kernel_family():
    """bench.py's regime, for every kernel family a solve can launch: several batches in flight on as
    many streams, all solving the same inputs.  Every solve must leave the records (status, movement,
    digest of every emitted cell) of a reference solve that ran alone and is checked against the
    oracle; >= 1000 solves per family (scripts/stress_inflight.py --suite): the headline shape (twelve
    batches of 1000 full-size scenarios) with two and one scenarios per solver wavefront, unpacked
    counter rows, the chunk-count pass; the wide ticket form for lists 5 and 4 wide (five wavefronts,
    class lists, joint solve, front[]) and with its count fields checked at the end (1,150 rows per broker); the
    spread fill with kas_spread_p4_kernel in front of both.
    (Round 2: with four fill wavefronts a P4 window could overtake an older window's orphan when the
    window in between finished early; one scenario solve in ~70,000 then put a broker one over its cap,
    which only this regime's timing brought out.  Lock-free LDS protocols are tested here or nowhere.)"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "scripts", "stress_inflight.py"), "--suite", "1000"],
                       cwd=root, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-1500:])
    import re
    m = re.search(r"suite: (\d+) of (\d+) kernel families clean", r.stdout)
    assert m and m.group(1) == m.group(2) and int(m.group(2)) >= 16, r.stdout[-3000:]
    assert r.stdout.count(": 0 scenario records differ from the reference") == int(m.group(2))


@pytest.mark.gpu
def test_slim_fill_kernel_and_the_scenarios_it_hands_back():
    """kas_fill_slim_kernel in front of kas_fill_kernel (round 6; the default for int32 cells, lists up to 3 wide, a direct id
    table, first fit handed over): 530 scenarios — from 512 on the plan takes kas_p4_kernel by itself — of which every seventh
    starts from rows that are not rack-diverse (the slim kernel flags it, the full kernel on its 256 workgroups solves it from its
    first topic), then scenarios of three topics whose last one is narrower than the batch (they stay with the slim kernel), and 2-wide lists."""
    S, P, N = 530, 1500, 60
    racks = (np.arange(N) % 6).astype(np.int32)
    ids = np.arange(N, dtype=np.int32)
    curs = [(G.cyclic_assignment(P, N, 3, s) * 6 % N) if s % 7 == 3 else G.random_assignment(900 + s, P, N, 6, 3) for s in range(S)]
    fb = uniform_batch(np.stack(curs).astype(np.int32), np.tile(ids, (S, 1))[:, :58], np.tile(racks, (S, 1))[:, :58], 3)
    want = oracle_solve(fb, threads=0)
    plan = native.Plan(native.default_context(), fb)
    d = plan.describe()
    plan.close()
    assert d.startswith("kas_fill_slim_kernel<3>[quota, chunk histograms] grid=530x256") and "kas_fill_kernel<3,4>[quota, chunk histograms] grid=256x256 lds=" in d and "for scenarios it hands back" in d and "+ kas_p4_kernel<3>" in d, d
    assert_same_outputs(fb, want, native.solve_host_with_flags(fb, 0), "hip slim fill: every seventh scenario handed back")
    assert_same_outputs(fb, want, native.solve_host_with_flags(fb, abi.KAS_PLAN_P4_WITH_ORDER), "hip slim fill + first fit beside the order kernel: every seventh handed back")
    assert_same_outputs(fb, want, native.solve_host_with_flags(fb, abi.KAS_PLAN_FULL_FILL), "hip the same without the slim kernel")
    scs = []
    for s in range(6):
        n = 30 + s
        scs.append(Scenario(brokers=list(range(n)), racks={b: "r%d" % (b % 6) for b in range(n)}, want_context=False,
                            topics=[Topic("a", {p: G.random_assignment(1 + s, 700, 32, 6, 3)[p].tolist() for p in range(700)}, 3),
                                    Topic("d", {p: G.random_assignment(40 + s, 900, 32, 6, 3)[p].tolist() for p in range(900)}, 3)] +
                                   ([Topic("c", {p: G.random_assignment(70 + s, 300, 32, 6, 2)[p].tolist() for p in range(300)}, 2)] if s % 2 else [])))
    fbt = flatten(scs)
    wantt = oracle_solve(fbt)
    for flags in (abi.KAS_PLAN_SPLIT_P4, abi.KAS_PLAN_P4_WITH_ORDER, abi.KAS_PLAN_SPLIT_P4 | abi.KAS_PLAN_FULL_FILL):
        assert_same_outputs(fbt, wantt, native.solve_host_with_flags(fbt, flags), f"hip slim fill, scenarios of several topics and widths, plan flags {flags:#x}")
    # scenarios whose SECOND topic starts from rows that are not rack-diverse: the slim kernel has written topic one's records, mid
    # rows and hand-over words by then; the full kernel solves the scenario again from its first topic over all of that
    from test_emu_parity import _later_topic_hands_back
    fb3 = _later_topic_hands_back()
    want3 = oracle_solve(fb3)
    for flags in (abi.KAS_PLAN_SPLIT_P4, abi.KAS_PLAN_P4_WITH_ORDER, 0):
        assert_same_outputs(fb3, want3, native.solve_host_with_flags(fb3, flags) if flags else native.solve_host(fb3), f"hip slim fill: a later topic hands the scenario back, plan flags {flags:#x}")
    fb2 = _batch(77, 5, 2500, 30, 6, 2, G.ACTIONS)
    assert_same_outputs(fb2, oracle_solve(fb2), native.solve_host_with_flags(fb2, abi.KAS_PLAN_SPLIT_P4), "hip slim fill, lists 2 wide")


@pytest.mark.gpu
def test_launch_behind_the_slim_kernel_grows_with_what_was_handed_back():
    """The kas_fill_kernel launch behind the slim kernel deals the flagged scenarios to its workgroups by RANK among them and leaves
    their number in a word of pinned host memory; the plan's next solve sizes that launch by it (kas_back_grid: one workgroup
    per handed-back scenario and a quarter more, in steps of 64, at most the fill's own grid).  600 scenarios of which two in three
    start from rows that are not rack-diverse (400 handed back): the first solve launches 256 workgroups behind the slim kernel, the
    second and third 512 — lists and records equal to the oracle's every time; a plan rebuilt for another batch starts small again."""
    import torch
    from kafka_assigner_amd.native import host_tables
    S, P, N = 600, 700, 60
    racks = (np.arange(N) % 6).astype(np.int32)
    ids = np.arange(N, dtype=np.int32)
    curs = [(G.cyclic_assignment(P, N, 3, s) * 6 % N) if s % 3 else G.random_assignment(500 + s, P, N, 6, 3) for s in range(S)]
    fb = uniform_batch(np.stack(curs).astype(np.int32), np.tile(ids, (S, 1))[:, :58], np.tile(racks, (S, 1))[:, :58], 3)
    want = oracle_solve(fb, threads=0)
    ctx = native.default_context()
    dev = torch.device("cuda", ctx.device)
    plan = native.Plan(ctx, fb)
    assert "kas_fill_kernel<3,4>[quota, chunk histograms] grid=256x256" in plan.describe(), plan.describe()
    d_cur = torch.from_numpy(fb.cur).to(dev)
    st = torch.cuda.Stream(dev)
    st.wait_stream(torch.cuda.current_stream(dev))
    for turn in range(3):
        _, ho = host_tables(fb)
        d_out = torch.full((fb.out_len,), -2, dtype=torch.int32, device=dev)
        d_tr = torch.zeros(fb.n_topics * 16, dtype=torch.uint8, device=dev)
        d_sr = torch.zeros(S * 32, dtype=torch.uint8, device=dev)
        st.wait_stream(torch.cuda.current_stream(dev))
        plan.solve_device(d_cur.data_ptr(), d_out.data_ptr(), d_tr.data_ptr(), d_sr.data_ptr(), stream=st.cuda_stream)
        st.synchronize()
        ho.out = d_out.cpu().numpy()
        ho.topic_results = d_tr.cpu().numpy().view(abi.TOPIC_RESULT_DTYPE)
        ho.scenario_results = d_sr.cpu().numpy().view(abi.SCENARIO_RESULT_DTYPE)
        assert_same_outputs(fb, want, ho, f"hip 400 of 600 scenarios handed back, solve {turn + 1} of one plan")
        assert "kas_fill_kernel<3,4>[quota, chunk histograms] grid=512x256" in plan.describe(), (turn, plan.describe())
    plan.close()
    fbs = uniform_batch(np.stack(curs[:530]).astype(np.int32), np.tile(ids, (530, 1))[:, :58], np.tile(racks, (530, 1))[:, :58], 3)
    plan = native.Plan(ctx, fbs)
    assert "kas_fill_kernel<3,4>[quota, chunk histograms] grid=256x256" in plan.describe(), plan.describe()
    plan.close()


@pytest.mark.gpu
def test_spread_fill_on_small_batches_and_what_it_hands_back():
    """KAS_PLAN_SPREAD_FILL: the spread fill (row scans of a scenario over several one-wavefront
    workgroups; by itself it serves batches of few scenarios of >= 131,072 rows, e.g. configs[4]) on small
    single-topic batches of every width it is built for, stranding scenarios included, and batches it
    hands back: rows that are not rack-diverse, a multi-topic batch."""
    from test_emu_parity import _multi_topic_scenarios
    for S, P, N, R, RF, acts in ((5, 9000, 120, 20, 3, G.ACTIONS), (3, 6000, 100, 20, 5, ("add_k", "mixed")),
                                 (3, 4001, 80, 16, 4, G.ACTIONS), (2, 150000, 300, 20, 3, ("mixed",))):
        fb = _batch(300 + RF, S, P, N, R, RF, acts)
        want = oracle_solve(fb, threads=0)
        plan = native.Plan(native.default_context(), fb); plan.set_flags(32)
        assert "kas_spread_" in plan.describe(), plan.describe()
        plan.close()
        assert_same_outputs(fb, want, native.solve_host_with_flags(fb, 32), f"hip spread fill RF {RF}")
    fb = _batch(77, 3, 2000, 40, 2, 3, ("remove1", "add_k"), cyclic=True)
    assert_same_outputs(fb, oracle_solve(fb), native.solve_host_with_flags(fb, 32), "hip spread fill, rows not rack-diverse")
    fb = _batch(78, 2, 3000, 60, 12, 3, ("add_k",), rack_aware=False)
    assert_same_outputs(fb, oracle_solve(fb), native.solve_host_with_flags(fb, 32), "hip spread fill, rack awareness off")
    fb = _multi_topic_scenarios(3, 2, 3, 900, 40, 8, 3)
    assert_same_outputs(fb, oracle_solve(fb), native.solve_host_with_flags(fb, 32), "hip spread flag, multi-topic batch")


def test_random_shapes_against_the_oracle_for_a_bounded_slice():
    """scripts/stress_gpu.py inside the driver-run suite (round 3 ran it by hand only): random shapes — 8 to 12,000
    brokers, 300 to 30,000 partitions, RF 2-5, every action mix, 1-8 scenarios per batch, thin rows 4-5 wide that
    overflow a count field of the wide form — each batch through one to four plan variants (relaxation form, ticket
    forms, round form, general fill, spread fill), every output compared with the oracle.  ~12 s of batches; the seed
    changes with the day so that successive driver runs draw different batches, and is printed."""
    import os
    import subprocess
    import sys
    import time
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    seed = int(time.time() // 86400)
    r = subprocess.run([sys.executable, os.path.join(root, "scripts", "stress_gpu.py"), "12", str(seed)],
                       cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "stress ok:" in r.stdout, (seed, r.stdout[-2000:], r.stderr[-2000:])
    n = int(r.stdout.split("stress ok:")[1].split()[0])
    assert n >= 100, (seed, r.stdout[-500:])
    print(r.stdout.strip().splitlines()[-1])


def test_many_rows_per_broker_keep_the_relaxation_form_up_to_16_bit_counts():
    """The relaxation form's count fields are 16 bits wide: a broker holding 4,095 rows of the scenario or more no
    longer sends the batch to the ticket form (round 4's first version: 12-bit fields).  90,000 partitions on 63
    brokers, rack awareness off (with racks the reference itself strands at this density): 4,286 rows per broker."""
    bs = G.perturb_brokers(60, 10, add=3, rack_aware=False)
    fb = uniform_batch(np.stack([G.random_assignment(61 + i, 90000, 60, 10, 3) for i in range(3)]),
                       np.stack([bs.node_id] * 3), np.stack([bs.node_rack] * 3), 3)
    want = oracle_solve(fb, threads=0)
    assert (want.scenario_results["status"] == abi.KAS_OK).any()
    plan = native.Plan(native.default_context(), fb)
    assert "kas_order_relax_kernel<3>" in plan.describe(), plan.describe()
    plan.close()
    assert_same_outputs(fb, want, native.solve_host(fb), "hip 4,286 rows per broker, relaxation form")
    assert_same_outputs(fb, want, native.solve_host_with_flags(fb, TILES_64), "hip 4,286 rows per broker, tiles of 64 rows")
    assert_same_outputs(fb, want, native.solve_host_with_flags(fb, TICKET_ORDER), "hip 4,286 rows per broker, ticket form")


def test_lds_lane_order_is_checked_and_the_sampled_verification_stays_silent():
    """Round 5: the context's self-test runs under LDS load on every CU and under partial EXEC masks, again at
    plan creation; KAS_PLAN_VERIFY_SAMPLE(k) evaluates k tiles per topic a second time row by row (no dependence on the
    LDS's lane order) — on this hardware it must agree with the relaxation everywhere; the conservation check is always on.
    tests/test_emu_lane_order.py shows what both catch when the order does NOT hold."""
    ctx = native.default_context()
    state, checked = ctx.lds_lane_order()
    assert state == 1 and checked >= 2048 * 200 * 64, (state, checked)
    fb = _batch(515, 6, 20000, 200, 10, 3, ("remove1", "add_k", "mixed"))
    want = oracle_solve(fb)
    assert (want.scenario_results["status"] == abi.KAS_OK).sum() >= 3
    plan = native.Plan(ctx, fb)                               # (a plan that may take the relaxation form: the self-test again)
    assert "kas_order_relax_kernel" in plan.describe()
    plan.close()
    assert ctx.lds_lane_order()[1] > checked
    for flags in (abi.KAS_PLAN_VERIFY_SAMPLE(255), TILES_64 | abi.KAS_PLAN_VERIFY_SAMPLE(16), TILES_128 | abi.KAS_PLAN_VERIFY_SAMPLE(255)):
        got = native.solve_host_with_flags(fb, flags)
        assert_same_outputs(fb, want, got, "hip, verification sample, flags %#x" % flags)
        assert not (got.scenario_results["status"] == abi.KAS_FAIL_WATCHDOG).any()

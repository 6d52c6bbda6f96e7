"""The host call planner (csrc/kas_host_call.h) through the emulator build of the same header: what kas_solve_host* decides before it
touches the GPU — scenario ranges, the cell width a 16-bit call is solved on, where selected rows and impact records go, the byte
size of every buffer, the error a bad call gets — and the pure half of the host path's plan cache.  Nothing is run: the library
executes the same KasHostCall (the -m gpu suites cover that: test_hip_parity.py, test_cells16.py, test_impact_gpu.py)."""
import numpy as np
import pytest

import emu_lib
from kafka_assigner_amd import abi, generator as G, sharding
from kafka_assigner_amd.flatten import FlatBatch, node_set_batch

SPLIT_MIN = 48 << 20       # KAS_HOST_SPLIT_MIN_BYTES: tables smaller than this are moved and solved as one range
SPLIT_MAX = 3              # KAS_HOST_SPLIT_MAX
BIG = (1 << 60,) * 4       # kas_tables lengths of a batch that exists as descriptors only
POOLS = ("topics", "cur", "out")


def _batch(S, P, W=3, n_nodes=40, shared_cur=False):
    """S single-topic scenarios of P rows x W cells, descriptors only"""
    ids = [np.arange(n_nodes, dtype=np.int32)] * S
    racks = [(np.arange(n_nodes) % 8).astype(np.int32)] * S
    return node_set_batch(ids, racks, P, W, W, shared_cur=shared_cur)


def _plan(fb, **kw):
    rc, plan, err = emu_lib.host_call(fb, **{"lens": BIG, **kw})
    assert rc == 0, err
    return plan


def _want_ranges(cells, cell_bytes, S, override=0):
    """the range count kas_solve_host has always chosen"""
    nbytes = cells * cell_bytes
    if nbytes < SPLIT_MIN or S < 2:
        return 1
    K = min(nbytes // (SPLIT_MIN // 2), SPLIT_MAX)
    if 1 <= override <= emu_lib.HOST_STREAMS:
        K = override
    return min(K, S)


# ---- ranges ---------------------------------------------------------------------------------------------------------------
def test_tables_below_the_threshold_are_one_range_and_at_it_two():
    # two scenarios x P x 3 cells in and out, int32: 48 P bytes, the threshold at P = 2^20 exactly
    at = SPLIT_MIN // 48
    assert _plan(_batch(2, at - 1))["K"] == 1
    assert _plan(_batch(2, at))["K"] == 2
    # 16-bit cells travel as two bytes each: the same batch is half the bytes
    assert _plan(_batch(2, 2 * at - 1), cells16=True)["K"] == 1
    assert _plan(_batch(2, 2 * at), cells16=True)["K"] == 2
    # only selected rows come back: `out` does not count
    assert _plan(_batch(2, 2 * at - 1), select=[1])["K"] == 1
    assert _plan(_batch(2, 2 * at), select=[1])["K"] == 2
    # one scenario is never cut
    assert _plan(_batch(1, 8 * at))["K"] == 1


@pytest.mark.parametrize("cells16", [False, True])
def test_range_count_follows_the_formula_capped_at_three_and_at_the_scenario_count(cells16):
    seen = set()
    for S in (2, 3, 5, 240):
        for P in (1000, 30000, 100000, 150000, 400000, 3000000):
            plan = _plan(_batch(S, P), cells16=cells16)
            want = _want_ranges(2 * S * P * 3, 2 if cells16 else 4, S)
            assert plan["K"] == want and len(plan["ranges"]) == want, (S, P, plan["K"], want)
            assert plan["K"] <= min(SPLIT_MAX, S)
            seen.add(plan["K"])
    assert seen == {1, 2, 3}


def test_the_override_counts_only_between_one_and_the_stream_count_and_only_for_a_call_that_splits():
    big, small = _batch(240, 100000), _batch(240, 1000)
    assert _plan(big)["K"] == 3
    for k in range(1, emu_lib.HOST_STREAMS + 1):
        assert _plan(big, ranges_override=k)["K"] == k
    for k in (0, -1, emu_lib.HOST_STREAMS + 1, 100):
        assert _plan(big, ranges_override=k)["K"] == 3
    for k in (2, 8):
        assert _plan(small, ranges_override=k)["K"] == 1
    assert _plan(_batch(5, 3000000), ranges_override=8)["K"] == 5     # never more ranges than scenarios


def test_ranges_are_the_shard_ranges_and_own_their_tables():
    S, P = 241, 100000
    fb = _batch(S, P)
    for k in (2, 3, 7):
        plan = _plan(fb, ranges_override=k)
        assert plan["K"] == k
        for i, r in enumerate(plan["ranges"]):
            lo, hi = sharding.shard_range(S, i, k)
            assert r["scenarios"] == (lo, hi) == emu_lib.shard_range(S, i, k)
            assert r["topics"] == (lo, hi)
            assert r["cur"] == (lo * P * 3, hi * P * 3) and r["out"] == (lo * P * 3, hi * P * 3)
            # the range's descriptors are the slice's: topics and node tables rebased to its first
            want = fb.scen[lo:hi].copy()
            want["topic_begin"] -= lo
            want["node_off"] -= fb.scen["node_off"][lo]
            assert r["scen"].tobytes() == want.tobytes()


def test_shared_or_interleaved_tables_collapse_to_one_range():
    S, P = 240, 100000
    # the what-if layout: every scenario reads one `cur`
    shared = _batch(S, P, shared_cur=True)
    assert _want_ranges(S * P * 3, 4, S) == 3                # (`out` alone is past the threshold)
    plan = _plan(shared)
    assert plan["K"] == 1 and plan["ranges"][0]["scenarios"] == (0, S)
    assert plan["ranges"][0]["cur"] == (0, P * 3) and plan["ranges"][0]["out"] == (0, S * P * 3)
    # topics in another order than the scenarios: a range's topics would not be a stretch of their own
    for order in (np.arange(S)[::-1], np.concatenate([np.arange(0, S, 2), np.arange(1, S, 2)])):
        fb = _batch(S, P)
        fb.scen["topic_begin"] = order
        assert _plan(fb)["K"] == 1
    # topics in order, their rows not: `out` of the first range ends behind where the second begins
    fb = _batch(S, P)
    fb.topics["out_off"] = fb.topics["out_off"][::-1].copy()
    assert _plan(fb)["K"] == 1
    fb = _batch(S, P)
    fb.topics["cur_off"] = fb.topics["cur_off"][::-1].copy()
    assert _plan(fb)["K"] == 1


def _ragged(rng, layout):
    """a ragged batch as descriptors: 1-12 scenarios with broker sets of their own (generator.scenario_action), 1-3 topics each of
    their own size and widths, tables laid out scenario by scenario (`ordered`), or with one shared cur (`shared`), the scenarios'
    topics in another order (`interleaved`) or the topics' rows in another order (`shuffled`)"""
    S = int(rng.integers(1, 13))
    sets = [G.scenario_action(int(rng.integers(1 << 30)), s, 60, 6, max_add=20)[1] for s in range(S)]
    counts = rng.integers(1, 4, size=S)
    T = int(counts.sum())
    scale = int(rng.choice([1000, 200000, 2000000]))
    scen = np.zeros(S, dtype=abi.SCENARIO_DESC_DTYPE)
    topics = np.zeros(T, dtype=abi.TOPIC_DESC_DTYPE)
    scen["n_nodes"] = [len(b.node_id) for b in sets]
    scen["node_off"] = np.concatenate([[0], np.cumsum(scen["n_nodes"])[:-1]])
    scen["topic_count"] = counts
    scen["topic_begin"] = np.concatenate([[0], np.cumsum(counts)[:-1]])
    scen["ctx_off"] = -1
    topics["n_partitions"] = rng.integers(1, scale + 1, size=T)
    topics["out_width"] = rng.integers(1, 6, size=T)
    topics["cur_width"] = rng.integers(1 if layout == "shared" else 0, topics["out_width"] + 1)
    topics["rf"] = topics["out_width"]
    topics["name_hash"] = rng.integers(-1000, 1000, size=T)
    cur_cells = topics["n_partitions"].astype(np.int64) * topics["cur_width"]
    out_cells = topics["n_partitions"].astype(np.int64) * topics["out_width"]
    topics["cur_off"] = np.concatenate([[0], np.cumsum(cur_cells)[:-1]])
    topics["out_off"] = np.concatenate([[0], np.cumsum(out_cells)[:-1]])
    for f in ("cur_len_off", "in_partitions_off", "part_id_off"):
        topics[f] = -1
    if layout == "shared":                                    # (every topic has rows there: cur_width >= 1 above)
        topics["cur_off"] = 0
    elif layout == "interleaved" and S > 1:
        order = rng.permutation(S)                            # scenario s takes the topics scenario order[s] had
        scen["topic_begin"], scen["topic_count"] = scen["topic_begin"][order].copy(), scen["topic_count"][order].copy()
    elif layout == "shuffled" and T > 1:
        order = rng.permutation(T)
        topics["out_off"][order] = np.concatenate([[0], np.cumsum(out_cells[order])[:-1]])
    return FlatBatch(scen=scen, topics=topics, node_id=np.concatenate([b.node_id for b in sets]).astype(np.int32),
                     node_rack=np.concatenate([b.node_rack for b in sets]).astype(np.int32), cur=np.zeros(1, np.int32),
                     aux=np.zeros(0, np.int32), ctx=np.zeros(0, np.int32), out_len=int(out_cells.sum()))


def test_ranges_of_random_ragged_batches_are_disjoint_and_cover_the_batch():
    rng = np.random.default_rng(20261016)
    split = {}
    for n in range(400):
        layout = ("ordered", "ordered", "shared", "interleaved", "shuffled")[n % 5]
        fb = _ragged(rng, layout)
        S, T = fb.n_scenarios, fb.n_topics
        cells16 = bool(n & 1)
        plan = _plan(fb, cells16=cells16)
        K, rs = plan["K"], plan["ranges"]
        cells = int((fb.topics["n_partitions"].astype(np.int64) * fb.topics["cur_width"]).sum() if layout != "shared" else
                    (fb.topics["n_partitions"].astype(np.int64) * fb.topics["cur_width"]).max()) + fb.out_len
        assert K in (1, _want_ranges(cells, 2 if cells16 else 4, S)), (n, layout, K)
        if layout == "ordered":                               # tables in scenario order are cut whenever the formula says so
            assert K == _want_ranges(cells, 2 if cells16 else 4, S), (n, K)
        assert [r["scenarios"] for r in rs] == [sharding.shard_range(S, i, K) for i in range(K)]
        full = {"topics": (0, T), **plan["full"]}
        for pool in POOLS:
            ext = [r[pool] for r in rs]
            assert all(lo <= hi for lo, hi in ext)
            assert all(ext[i][1] <= ext[i + 1][0] for i in range(K - 1)), (n, layout, pool, ext)     # ascending: pairwise disjoint
            assert sum(hi - lo for lo, hi in ext) == full[pool][1] - full[pool][0], (n, layout, pool, ext, full[pool])   # ... and nothing left out
            assert ext[0][0] == full[pool][0] and ext[-1][1] == full[pool][1]
        split[layout] = split.get(layout, 0) + (K > 1)
    assert split["ordered"] >= 40 and split["shared"] == 0, split


# ---- select ---------------------------------------------------------------------------------------------------------------
def test_selected_rows_are_packed_at_the_prefix_sums():
    rng = np.random.default_rng(7)
    for n in range(40):
        fb = _ragged(rng, "ordered")
        S = fb.n_scenarios
        select = rng.integers(0, S, size=int(rng.integers(0, 2 * S + 1)))
        rows = np.zeros(S, dtype=np.int64)
        for s in range(S):
            t = fb.topics[fb.scen["topic_begin"][s]:fb.scen["topic_begin"][s] + fb.scen["topic_count"][s]]
            rows[s] = (t["n_partitions"].astype(np.int64) * t["out_width"]).sum()
        want = np.concatenate([[0], np.cumsum(rows[select])]).astype(np.int64)
        plan = _plan(fb, select=select, lens=(BIG[0], int(want[-1]), 0, 0))
        assert plan["sel_off"] == want.tolist()
        assert _plan(fb)["sel_off"] == []                      # every row where the descriptors say: nothing to pack


def test_a_bad_selection_gets_the_code_and_text_it_always_got():
    fb = _batch(4, 100)
    lens = (4 * 300, 4 * 300, 0, 0)
    bad = abi.KAS_E_INVALID_ARG
    for select in ([4], [-1], [0, 1, 7]):
        assert emu_lib.host_call(fb, lens, select=select)[::2] == (bad, "select: scenario index out of range")
    assert emu_lib.host_call(fb, (4 * 300, 599, 0, 0), select=[0, 3])[::2] == (bad, "select: out / out_len too small for the selected scenarios' rows")
    assert emu_lib.host_call(fb, (4 * 300, 600, 0, 0), select=[0, 3])[0] == 0
    assert emu_lib.host_call(fb, lens, select=[0, 3], missing=("out",))[::2] == (bad, "select: out / out_len too small for the selected scenarios' rows")
    assert emu_lib.host_call(fb, lens, select=[], missing=("out",))[0] == 0


def test_the_checks_run_in_the_order_callers_know():
    fb = _batch(4, 100)
    bad = abi.KAS_E_INVALID_ARG
    beyond = "a descriptor offset reaches beyond the pool length given in kas_tables"
    null = "a table the descriptors refer to is NULL"
    assert emu_lib.host_call(fb, (1199, 1200, 0, 0))[::2] == (bad, beyond)
    assert emu_lib.host_call(fb, (1200, 1199, 0, 0))[::2] == (bad, beyond)
    assert emu_lib.host_call(fb, (1200, 0, 0, 0), select=[])[0] == 0              # (out_len is the selection's business then)
    assert emu_lib.host_call(fb, (1199, 1200, 0, 0), select=[9], missing=("cur",))[::2] == (bad, beyond)     # lengths, then tables, then the selection
    assert emu_lib.host_call(fb, (1200, 1200, 0, 0), select=[9], missing=("cur",))[::2] == (bad, null)
    for m in ("cur", "out", "topic_results", "scenario_results"):
        assert emu_lib.host_call(fb, (1200, 1200, 0, 0), missing=(m,))[::2] == (bad, null)
    assert emu_lib.host_call(fb, (1200, 1200, 0, 0), missing=("aux", "ctx"))[0] == 0  # (no descriptor refers to them)
    # the batch's own shape is refused before any table is looked at
    wide = _batch(2, 100)
    wide.topics["out_width"] = 9
    rc, _, err = emu_lib.host_call(wide, (0, 0, 0, 0), missing=("cur", "out"))
    assert rc == abi.KAS_E_UNSUPPORTED and "out_width outside" in err
    # impact records: scenario s's node block starts at the sum of the n_nodes before it
    rag = _ragged(np.random.default_rng(3), "ordered")
    plan = _plan(rag, impact=True)
    assert plan["imp_base"] == np.concatenate([[0], np.cumsum(rag.scen["n_nodes"])]).tolist()
    assert plan["bytes"]["imp_nodes"] == abi.NODE_IMPACT_DTYPE.itemsize * (plan["imp_base"][-1] + 1)
    assert plan["bytes"]["imp_scen"] == abi.SCENARIO_IMPACT_DTYPE.itemsize * (rag.n_scenarios + 1)
    assert _plan(rag)["imp_base"] == [] and _plan(rag)["bytes"]["imp_nodes"] == _plan(rag)["bytes"]["imp_scen"] == 0
    for m in ("imp_nodes", "imp_scenarios"):
        assert emu_lib.host_call(rag, BIG, impact=True, missing=(m,))[::2] == (bad, "kas_impact_tables: nodes / scenarios == NULL")


# ---- 16-bit cells ---------------------------------------------------------------------------------------------------------
def test_a_16_bit_call_is_solved_on_its_own_cells_exactly_where_the_16_bit_kernels_take_the_batch():
    native = widened = 0
    for W in (2, 3, 4, 5):
        for n_nodes in (100, 1050, 9000):
            fb = _batch(24, 20000, W, n_nodes)
            rc, sh, err = emu_lib.plan_shape(fb)
            if rc != 0:                                        # no plan takes the shape: the call is refused with the same words
                assert emu_lib.host_call(fb, BIG, cells16=True)[::2] == (rc, err) == emu_lib.host_call(fb, BIG)[::2]
                continue
            cells = 24 * 20000 * W
            for lane in (True, False):
                for built in (emu_lib.BUILT_ALL, emu_lib.BUILT_ALL & ~emu_lib.BUILT_RELAX):
                    # kas_cells16_ok (kas_launch_plan.h) on the shape
                    want = W <= 3 and bool((sh["relax_ok"] and lane and (built & emu_lib.BUILT_RELAX)) or sh["round_fits"])
                    plan = _plan(fb, cells16=True, lane_order_ok=lane, built=built)
                    by = plan["bytes"]
                    assert plan["native16"] == want and plan["need32"] == (not want), (W, n_nodes, lane, built)
                    assert by["cur16"] == by["out16"] == 2 * (cells + 8)
                    assert by["cur"] == by["out"] == (0 if want else 4 * (cells + 8))     # a native call reserves no int32 pools, a widened one both
                    if lane and built == emu_lib.BUILT_ALL:    # the describe path's own verdict (a passed self-test, every family built)
                        assert want == (emu_lib.describe(fb, cells16=True)[0] == 0), (W, n_nodes)
                    native += want
                    widened += not want
            plan = _plan(fb)                                   # the int32 call: no 16-bit pools
            assert not plan["native16"] and plan["need32"]
            assert plan["bytes"]["cur16"] == plan["bytes"]["out16"] == 0 and plan["bytes"]["cur"] == plan["bytes"]["out"] == 4 * (cells + 8)
            assert plan["bytes"]["aux"] == plan["bytes"]["ctx"] == 4 * 8
            assert plan["bytes"]["tr"] == plan["bytes"]["tr_pin"] == abi.TOPIC_RESULT_DTYPE.itemsize * 25
            assert plan["bytes"]["sr"] == plan["bytes"]["sr_pin"] == abi.SCENARIO_RESULT_DTYPE.itemsize * 25
    assert native >= 12 and widened >= 12, (native, widened)


# ---- the plan cache's choice ----------------------------------------------------------------------------------------------
KEY, SIG, CALL = 0xAAAA, 0x5151, 77


def _entries(n=16, **at):
    """n occupied entries of other batches, used at clock 100 + i by earlier calls; at[i] = overrides of entry i"""
    es = [dict(occupied=1, key=1000 + i, sig=2000 + i, last_use=100 + i, call=CALL - 1) for i in range(n)]
    for i, over in at.items():
        es[int(i[1:])].update(over)
    return [(e["occupied"], e["key"], e["sig"], e["last_use"], e["call"]) for e in es]


def test_a_hit_beats_everything():
    # ... the same-signature entry, the free entry and the oldest entry; also when this call has used it already
    es = _entries(e3=dict(sig=SIG, last_use=1), e5=dict(occupied=0), e9=dict(key=KEY, sig=SIG, last_use=500))
    assert emu_lib.cache_choose(es, KEY, SIG, CALL)[0] == 9
    es = _entries(e9=dict(key=KEY, sig=SIG, call=CALL))
    assert emu_lib.cache_choose(es, KEY, SIG, CALL)[0] == 9
    assert emu_lib.cache_choose(_entries(), KEY, SIG, CALL)[0] == -1
    assert emu_lib.cache_choose(_entries(e2=dict(occupied=0, key=KEY)), KEY, SIG, CALL)[0] == -1    # (a free entry holds no plan)


def test_a_miss_rebuilds_same_signature_then_fills_a_free_entry_then_evicts_the_oldest():
    es = _entries(e3=dict(sig=SIG, last_use=400), e7=dict(sig=SIG, last_use=300), e5=dict(occupied=0), e11=dict(last_use=1))
    assert emu_lib.cache_choose(es, KEY, SIG, CALL) == (-1, 7)           # the least recently used of the same signature
    es = _entries(e5=dict(occupied=0), e8=dict(occupied=0), e11=dict(last_use=1))
    assert emu_lib.cache_choose(es, KEY, SIG, CALL) == (-1, 5)           # the first free entry, before any eviction
    es = _entries(e11=dict(last_use=1))
    assert emu_lib.cache_choose(es, KEY, SIG, CALL) == (-1, 11)          # the least recently used of any shape
    assert emu_lib.cache_choose(_entries(), KEY, SIG, CALL) == (-1, 0)


def test_entries_of_the_current_call_are_never_victims():
    es = _entries(e3=dict(sig=SIG, last_use=1, call=CALL), e7=dict(sig=SIG, last_use=300))
    assert emu_lib.cache_choose(es, KEY, SIG, CALL) == (-1, 7)
    es = _entries(e0=dict(call=CALL), e1=dict(call=CALL), e3=dict(sig=SIG, call=CALL))
    assert emu_lib.cache_choose(es, KEY, SIG, CALL) == (-1, 2)
    es = _entries(e0=dict(call=CALL), e6=dict(occupied=0, call=CALL))
    assert emu_lib.cache_choose(es, KEY, SIG, CALL) == (-1, 6)           # (a free entry has no call to protect)
    # all sixteen stamped with this call: nothing to evict — the library's KAS_E_NOMEM, "plan cache exhausted by one call"
    es = _entries(**{"e%d" % i: dict(call=CALL) for i in range(16)})
    assert emu_lib.cache_choose(es, KEY, SIG, CALL) == (-1, -1)
    es[4] = (1, KEY, SIG, 104, CALL)
    assert emu_lib.cache_choose(es, KEY, SIG, CALL) == (4, -1)           # ... unless one of them is the batch's own plan


def test_what_if_variants_share_a_signature_and_cell_widths_do_not():
    a, b = _batch(6, 500), _batch(6, 500)
    b.node_rack = ((b.node_rack + 1) % 8).astype(np.int32)    # same snapshot, other broker racks
    (ka, sa), (kb, sb) = emu_lib.batch_ident(a), emu_lib.batch_ident(b)
    assert ka != kb and sa == sb
    assert emu_lib.batch_ident(a) == (ka, sa)
    k16, s16 = emu_lib.batch_ident(a, cells16=True)
    assert k16 != ka and s16 != sa
    ks, ss = emu_lib.batch_ident(_batch(6, 501))
    assert ks != ka and ss != sa


# ---- slicing --------------------------------------------------------------------------------------------------------------
def test_the_headers_slicing_is_the_librarys():
    """kas_shard_range / kas_batch_slice of the header against the library's exports (host arithmetic: no device) and
    kafka_assigner_amd.sharding, on the ranges and the batch of test_sharding_gloo.py"""
    from kafka_assigner_amd import native
    from test_emu_parity import _batch as parity_batch
    L = native.load()
    for n in (0, 1, 7, 64, 1000, 64000):
        for world in (1, 2, 3, 8):
            for rank in range(world):
                assert emu_lib.shard_range(n, rank, world) == emu_lib.shard_range(n, rank, world, L.kas_shard_range) == sharding.shard_range(n, rank, world)
    assert emu_lib.shard_range(10, 5, 3) == emu_lib.shard_range(10, 5, 3, L.kas_shard_range) == sharding.shard_range(10, 2, 3)   # (clamped)
    for n in (6, 7):
        fb = parity_batch(4242, n, 600, 30, 6, 3, G.ACTIONS)
        for lo, hi in [sharding.shard_range(n, r, 2) for r in range(2)] + [(0, n), (2, 2), (1, n - 1)]:
            rc, mine = emu_lib.batch_slice(fb, lo, hi)
            rc_lib, theirs = emu_lib.batch_slice(fb, lo, hi, L.kas_batch_slice)
            assert rc == rc_lib == 0 and mine == theirs
            assert (mine["n_scenarios"], mine["n_topics"]) == (hi - lo, hi - lo)
            if hi > lo:
                assert mine["topic"] == lo and mine["topic_results"] == lo and mine["scenario_results"] == lo
                assert mine["node_id"] == mine["node_rack"] == int(fb.scen["node_off"][lo])
        for lo, hi in ((-1, 2), (3, 2), (0, n + 1)):
            assert emu_lib.batch_slice(fb, lo, hi)[0] == emu_lib.batch_slice(fb, lo, hi, L.kas_batch_slice)[0] == abi.KAS_E_INVALID_ARG
            assert L.kas_last_error() == b"kas_batch_slice: bad range / NULL argument"

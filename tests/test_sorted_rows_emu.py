"""Round 7 on the CPU emulator: the slim fill's row pass with the holders taken as a set (p3_rows' SORTED_OUT and DISTINCT forms) and
the order kernel's final lists straight from the dword's fields (relax_pick3, the broker ids read at the top of the tile) must
reproduce the oracle bit for bit — records and every list — on batches of the headline's kind: 512 scenarios, so that the plan takes
the slim fill, kas_p4_kernel and tiles of 64 rows by batch size.  The same batches on the packed 16-bit rows (KAS_PLAN_NO_MID32),
whose code the round leaves alone.  (The 1,100- and 2,046-broker batches take the emulator 4 and 8 s a solve: its time goes with the
node tables of 512 scenarios.)"""
import functools

import numpy as np
import pytest

import emu_lib
import sorted_rows_cases as cases
from emu_lib import NO_MID32, emu_solve
from oracle_lib import oracle_solve
from parity_util import assert_same_outputs

NAMES = ("40 brokers", "1100 brokers", "2046 brokers")


@functools.lru_cache(maxsize=None)
def _case(name):
    """(batch, the oracle's outputs): computed once, shared, never written to"""
    fb = cases.batch_40() if name == "40 brokers" else cases.batch_wide(int(name.split()[0]))
    return fb, oracle_solve(fb, threads=0)


def test_the_batches_hold_the_rows_they_are_meant_to():
    fb, want = _case("40 brokers")
    assert fb.n_scenarios == 512 and fb.n_topics == 513
    assert cases.kept_counts(fb, 1, range(6)) == [0, 1, 2, 3, 1, 1]          # rows that keep 0..3 replicas, the unknown ids named twice
    assert int(fb.scen[2]["n_nodes"]) == 90                                   # 50 brokers joined: quotas run out inside the tiles
    cap = -(-cases.P * 3 // 90)
    t2 = int(fb.scen[2]["topic_begin"])
    assert want.topic_results["moved_replicas"][t2] >= cases.P * 3 - 40 * cap   # ... the 40 old brokers keep at most cap replicas each
    assert [int(fb.topics[int(fb.scen[s]["topic_begin"])]["cur_width"]) for s in (4, 5)] == [3, 2]   # a topic narrower than the batch
    assert int(fb.scen[7]["topic_count"]) == 2
    assert (want.scenario_results["status"][[1, 2, 5, 7, 9, 300]] == 0).all()      # (the scenarios made by hand are solved, not failed)
    assert 0.5 < (want.scenario_results["status"] == 0).mean() < 1.0                  # (some of the others strand a partition, KAS:183-184)
    for name in NAMES[1:]:
        fbw, _ = _case(name)
        assert int(fbw.scen["n_nodes"].max()) <= 2047 and int(fbw.scen["n_nodes"].min()) >= 1024, name
    # unknown ids named twice: the row loses a broker (moved), whatever stands in the third cell is kept
    t1 = int(fb.scen[1]["topic_begin"])
    assert want.topic_results["moved_partitions"][t1] >= 5


@pytest.mark.parametrize("flags", [0, NO_MID32], ids=["dword rows", "16-bit rows"])
@pytest.mark.parametrize("name", NAMES)
def test_emu_equals_oracle_on_the_headlines_kernels(name, flags):
    fb, want = _case(name)
    rc, what = emu_lib.describe(fb, flags)
    assert rc == 0 and "kas_fill_slim_kernel<3>" in what and "kas_p4_kernel<3>" in what and "tiles of 64 rows" in what, what
    assert ("dword mid rows" in what) == (flags == 0), what
    got = emu_solve(fb, flags=flags, p4_by_batch_size=True)
    assert emu_lib.last_mid32() == (1 if flags == 0 else 0)
    assert emu_lib.last_split_p4() == 1
    assert_same_outputs(fb, want, got, f"emu, {name}, plan flags {flags:#x}")
    # rows that name a KNOWN broker twice are not rack-diverse: those scenarios, and no others, go back to kas_fill_kernel — rows that
    # name an unknown broker twice (scenario 1) stay with the slim kernel
    back = len(cases.HANDED_BACK_40) if name == "40 brokers" else 0
    assert emu_lib.last_handback() == back and emu_lib.last_slim_fill() == 512 - back, (emu_lib.last_handback(), emu_lib.last_slim_fill())
    if name == "40 brokers":
        np.testing.assert_array_equal(got.topic_results["moved_partitions"], want.topic_results["moved_partitions"])

"""The launch resolver (csrc/kas_launch_plan.h) through the emulator build of the same header: the text kas_plan_describe renders
for the headline batch is the one the GPU test and bench.py's roofline.kernel name, and over a matrix of shapes x plan switches
every resolved launch is launchable — LDS within 160 KiB, one order stage, every kernel identity an instance of the emulator's
mapping and among the launches kas_plan_set_kernels enumerates (kas_enumerate_launches, the same header).

The library's own mapping (identity -> __global__ function) only compiles with hipcc: that an identity is an instance of the
library is checked where it is launched, by the -m gpu suites (a resolved kernel the build does not hold is a solve error)."""
import os

import numpy as np
import pytest

import emu_lib
from kafka_assigner_amd import abi
from kafka_assigner_amd.flatten import node_set_batch
from test_headline_launch import CELLS16_KERNELS, FULL_FILL_KERNELS, HEADLINE_KERNELS, M32, MID32_BY_DEFAULT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _batch(n_nodes, rf, S, P, ctx=False):
    """S scenarios of one topic, from descriptors only (no tables)"""
    ids = [np.arange(n_nodes, dtype=np.int32)] * S
    racks = [(np.arange(n_nodes) % 20).astype(np.int32)] * S
    fb = node_set_batch(ids, racks, P, rf, rf)
    if ctx:                                            # every scenario hands a Context in and wants it back
        off = 0
        for s in range(S):
            fb.scen["ctx_off"][s] = off
            fb.scen["ctx_width"][s] = rf
            off += n_nodes * rf
    return fb


def test_describe_text_of_the_headline_batch_is_the_one_the_gpu_test_asserts():
    fb = _batch(1050, 3, 1000, 100000)
    m32 = M32 if MID32_BY_DEFAULT else ""
    assert emu_lib.describe(fb) == (0, HEADLINE_KERNELS % m32)
    assert emu_lib.describe(fb, abi.KAS_PLAN_NO_MID32) == (0, HEADLINE_KERNELS % "")
    assert emu_lib.describe(fb, abi.KAS_PLAN_MID32) == (0, HEADLINE_KERNELS % M32)
    assert emu_lib.describe(fb, abi.KAS_PLAN_FULL_FILL) == (0, FULL_FILL_KERNELS % ("", m32))
    assert emu_lib.describe(fb, abi.KAS_PLAN_INDEX_ROWS) == (0, FULL_FILL_KERNELS % (", index rows", ""))
    assert emu_lib.describe(fb, cells16=True) == (0, CELLS16_KERNELS)


SWITCHES = [0, abi.KAS_PLAN_GENERIC_FILL, abi.KAS_PLAN_ROUND_ORDER, abi.KAS_PLAN_WIDE_COUNTERS, abi.KAS_PLAN_TWO_PASS_HIST,
            abi.KAS_PLAN_FULL_FILL, abi.KAS_PLAN_SPREAD_FILL, abi.KAS_PLAN_NO_INDEX_ROWS, abi.KAS_PLAN_INDEX_ROWS,
            abi.KAS_PLAN_TICKET_ORDER, abi.KAS_PLAN_RELAX_TILES_64, abi.KAS_PLAN_RELAX_TILES_128,
            abi.KAS_PLAN_RELAX_TILES_64 | abi.KAS_PLAN_RELAX_TILES_128, abi.KAS_PLAN_MID32, abi.KAS_PLAN_NO_MID32,
            abi.KAS_PLAN_NO_RTN_QUOTA, abi.KAS_PLAN_SPLIT_P4, abi.KAS_PLAN_FILL_WITH_P4, abi.KAS_PLAN_P4_WITH_ORDER,
            1 << 24,                                   # KAS_PLAN_VERIFY_SAMPLE(1)
            1 << 12, 4 << 12, 1 << 8, 2 << 8,          # KAS_PLAN_GROUPS(1 / 4), KAS_PLAN_WAVES(1 / 2)
            # the combinations the GPU suites use
            abi.KAS_PLAN_SPLIT_P4 | abi.KAS_PLAN_RELAX_TILES_64,
            abi.KAS_PLAN_SPLIT_P4 | abi.KAS_PLAN_RELAX_TILES_64 | abi.KAS_PLAN_INDEX_ROWS,
            abi.KAS_PLAN_P4_WITH_ORDER | abi.KAS_PLAN_NO_MID32,
            abi.KAS_PLAN_P4_WITH_ORDER | abi.KAS_PLAN_RELAX_TILES_64 | abi.KAS_PLAN_RELAX_TILES_128,
            abi.KAS_PLAN_TICKET_ORDER | abi.KAS_PLAN_WIDE_COUNTERS, abi.KAS_PLAN_FILL_WITH_P4 | abi.KAS_PLAN_RELAX_TILES_128]


def test_every_resolved_launch_of_the_matrix_is_launchable():
    """widths 2-5 and 8; 100 / 1,050 / 5,000 / 9,000 brokers; with and without Context; both cell widths; 24 and 1000 scenarios; every
    KAS_PLAN_* switch alone and the combinations the GPU tests use: every stage's LDS within 160 KiB, exactly one order stage, every
    kernel identity an instance of the emulator's mapping and one of those kas_plan_set_kernels enumerates (emu_lib.launch_check)."""
    resolved = refused = 0
    for rf in (2, 3, 4, 5, 8):
        for n in (100, 1050, 5000, 9000):
            for ctx in (False, True):
                for S in (24, 1000):
                    fb = _batch(n, rf, S, 20000, ctx)
                    for c16 in (False, True):
                        for flags in SWITCHES:
                            rc, text = emu_lib.launch_check(fb, flags, c16)
                            assert rc <= 0, (rf, n, ctx, S, c16, hex(flags), text)
                            assert rc == 0 or rc in (abi.KAS_E_UNSUPPORTED, abi.KAS_E_INVALID_ARG), (rc, text)
                            resolved += rc == 0
                            refused += rc != 0
    assert resolved + refused == 5 * 4 * 2 * 2 * 2 * len(SWITCHES) and resolved > refused, (resolved, refused)


@pytest.mark.parametrize("flags", [0, abi.KAS_PLAN_P4_WITH_ORDER, abi.KAS_PLAN_TICKET_ORDER, abi.KAS_PLAN_ROUND_ORDER])
def test_describe_names_what_the_emulator_then_runs(flags):
    """the text and the emulator's observables come off one resolved launch"""
    from kafka_assigner_amd import generator as G
    from kafka_assigner_amd.flatten import uniform_batch
    cur = np.stack([G.random_assignment(40 + s, 600, 40, 8, 3) for s in range(3)]).astype(np.int32)
    ids = np.tile(np.arange(40, dtype=np.int32), (3, 1))
    fb = uniform_batch(cur, ids, ids % 8, 3)
    rc, text = emu_lib.describe(fb, flags)
    assert rc == 0, text
    emu_lib.emu_solve(fb, flags=flags, p4_by_batch_size=True)
    assert ("kas_p4_order_kernel<3>" in text) == bool(emu_lib.last_p4_order())
    assert (" + kas_p4_kernel<3>" in text) == bool(emu_lib.last_split_p4())
    assert ("dword mid rows" in text) == bool(emu_lib.last_mid32())
    assert text.startswith("kas_fill_slim_kernel<3>") == (emu_lib.last_slim_fill() > 0)
    form = {3: "kas_order_relax_kernel<3>", 1: "kas_order_ticket_kernel<3,", 0: "kas_order_round_kernel<3>"}[emu_lib.last_order_form()]
    assert form in text, text

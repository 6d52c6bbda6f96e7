"""ctypes binding of the C ABI (include/kas_abi.h) implemented by csrc/libkas_hip.so.

There is no fallback: if the library has not been built, or no gfx950 device is visible, every
solve entry point raises.  The library is looked up in-tree only (kafka-assigner_amd/csrc/).
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import abi
from .flatten import FlatBatch, HostOutputs, batch_desc, host_tables

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "csrc", "libkas_hip.so")

# every symbol include/kas_abi.h declares
SYMBOLS = [
    "kas_abi_version", "kas_strerror", "kas_status_string", "kas_last_error", "kas_device_count",
    "kas_ctx_create", "kas_ctx_destroy", "kas_ctx_synchronize", "kas_plan_create",
    "kas_plan_destroy", "kas_plan_algorithmic_bytes", "kas_solve_device", "kas_solve_host",
    "kas_plan_kernel_time_us", "kas_plan_phase_times_us", "kas_plan_stats", "kas_plan_set_flags",
    "kas_plan_describe", "kas_ctx_host_stats", "kas_solve_host_select", "kas_host_alloc", "kas_host_free",
    "kas_shard_range", "kas_batch_slice", "kas_solve_host_sharded", "kas_ctx_lds_lane_order", "kas_solve_host16",
    "kas_plan_create16", "kas_solve_device16", "kas_resolve_replication_factor", "kas_failure_text",
    "kas_impact_device", "kas_impact_device16", "kas_solve_host_impact", "kas_solve_host16_impact",
    "kas_rank_device", "kas_choose_device", "kas_choose_device16", "kas_solve_host_choose", "kas_solve_host16_choose",
    "kas_moves_device", "kas_moves_device16", "kas_solve_host_moves", "kas_solve_host16_moves", "kas_solve_host_choose_moves",
    "kas_solve_host16_choose_moves",
    "kas_front_rank_device", "kas_front_device", "kas_front_device16", "kas_solve_host_front", "kas_solve_host16_front",
    "kas_rack_impact_device", "kas_rack_impact_device16", "kas_solve_host_rack_impact", "kas_solve_host16_rack_impact",
    "kas_rank_device_racks", "kas_front_rank_device_racks", "kas_choose_device_racks", "kas_choose_device16_racks",
    "kas_front_device_racks", "kas_front_device16_racks", "kas_solve_host_choose_racks", "kas_solve_host16_choose_racks",
    "kas_solve_host_front_racks", "kas_solve_host16_front_racks",
    "kas_topic_impact_device", "kas_topic_impact_device16", "kas_solve_host_topic_impact", "kas_solve_host16_topic_impact",
    "kas_rank_device_topics", "kas_front_rank_device_topics", "kas_choose_device_topics", "kas_choose_device16_topics",
    "kas_front_device_topics", "kas_front_device16_topics", "kas_solve_host_choose_topics", "kas_solve_host16_choose_topics",
    "kas_solve_host_front_topics", "kas_solve_host16_front_topics",
    "kas_batches_device", "kas_batches_device16", "kas_solve_host_batches", "kas_solve_host16_batches",
    "kas_rounds_device", "kas_rounds_device16", "kas_solve_host_rounds", "kas_solve_host16_rounds",
]

_LIB = None


class KasError(RuntimeError):
    def __init__(self, code: int, detail: str):
        super().__init__(f"kas error {code}: {detail}")
        self.code = code
        self.detail = detail


def load():
    """dlopen csrc/libkas_hip.so and declare prototypes.  Raises if it is not built."""
    global _LIB
    if _LIB is not None:
        return _LIB
    lib_path = os.environ.get("KAS_HIP_LIB", LIB_PATH)     # tuning builds of the same library
    if not os.path.exists(lib_path):
        raise ImportError(
            f"{lib_path} is missing: build it with `python -m kafka_assigner_amd.build` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    # PyTorch bundles its own libamdhip64.so.7 / libhsa-runtime64.so.1 with the same SONAMEs as
    # /opt/rocm's; whichever is loaded first serves the whole process, and mixing them (ours
    # first, torch second) leaves HIP without devices.  Torch owns device memory and streams in
    # this project, so its runtime must be the one: import it before the dlopen.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(lib_path)
    L.kas_abi_version.restype = C.c_int
    L.kas_strerror.restype = C.c_char_p; L.kas_strerror.argtypes = [C.c_int]
    L.kas_status_string.restype = C.c_char_p; L.kas_status_string.argtypes = [C.c_int]
    L.kas_last_error.restype = C.c_char_p
    L.kas_device_count.restype = C.c_int
    L.kas_ctx_create.restype = C.c_int; L.kas_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.kas_ctx_destroy.restype = None; L.kas_ctx_destroy.argtypes = [C.c_void_p]
    L.kas_ctx_synchronize.restype = C.c_int; L.kas_ctx_synchronize.argtypes = [C.c_void_p]
    L.kas_plan_create.restype = C.c_int
    L.kas_plan_create.argtypes = [C.c_void_p, C.POINTER(abi.BatchDesc), C.POINTER(C.c_void_p)]
    L.kas_plan_destroy.restype = None; L.kas_plan_destroy.argtypes = [C.c_void_p]
    L.kas_plan_algorithmic_bytes.restype = C.c_int64; L.kas_plan_algorithmic_bytes.argtypes = [C.c_void_p]
    L.kas_solve_device.restype = C.c_int
    L.kas_solve_device.argtypes = [C.c_void_p, C.POINTER(abi.Tables), C.c_void_p]
    L.kas_solve_host.restype = C.c_int
    L.kas_solve_host.argtypes = [C.c_void_p, C.POINTER(abi.BatchDesc), C.POINTER(abi.Tables)]
    L.kas_solve_host_select.restype = C.c_int
    L.kas_solve_host_select.argtypes = [C.c_void_p, C.POINTER(abi.BatchDesc), C.POINTER(abi.Tables),
                                        C.POINTER(C.c_int32), C.c_int32]
    L.kas_solve_host16.restype = C.c_int         # (kas_tables16 has kas_tables' layout: abi.Tables holds untyped pointers)
    L.kas_solve_host16.argtypes = [C.c_void_p, C.POINTER(abi.BatchDesc), C.POINTER(abi.Tables),
                                   C.POINTER(C.c_int32), C.c_int32]
    L.kas_plan_create16.restype = C.c_int
    L.kas_plan_create16.argtypes = [C.c_void_p, C.POINTER(abi.BatchDesc), C.POINTER(C.c_void_p)]
    L.kas_solve_device16.restype = C.c_int
    L.kas_solve_device16.argtypes = [C.c_void_p, C.POINTER(abi.Tables), C.c_void_p]
    L.kas_solve_host_sharded.restype = C.c_int
    L.kas_solve_host_sharded.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.POINTER(abi.BatchDesc), C.POINTER(abi.Tables)]
    L.kas_host_alloc.restype = C.c_int; L.kas_host_alloc.argtypes = [C.c_int64, C.POINTER(C.c_void_p)]
    L.kas_host_free.restype = None; L.kas_host_free.argtypes = [C.c_void_p]
    L.kas_shard_range.restype = None
    L.kas_shard_range.argtypes = [C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.kas_batch_slice.restype = C.c_int
    L.kas_batch_slice.argtypes = [C.POINTER(abi.BatchDesc), C.c_int64, C.c_int64, C.POINTER(abi.ScenarioDesc),
                                  C.POINTER(abi.BatchDesc), C.POINTER(abi.Tables), C.POINTER(abi.Tables)]
    L.kas_plan_kernel_time_us.restype = C.c_int
    L.kas_plan_kernel_time_us.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int)]
    L.kas_plan_phase_times_us.restype = C.c_int
    L.kas_plan_phase_times_us.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                          C.POINTER(C.c_int)]
    L.kas_plan_set_flags.restype = C.c_int
    L.kas_plan_set_flags.argtypes = [C.c_void_p, C.c_uint32]
    L.kas_ctx_host_stats.restype = C.c_int
    L.kas_ctx_host_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.kas_plan_describe.restype = C.c_int
    L.kas_plan_describe.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    L.kas_plan_stats.restype = C.c_int
    L.kas_plan_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.c_int64]
    L.kas_resolve_replication_factor.restype = C.c_int
    L.kas_resolve_replication_factor.argtypes = [C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_int32,
                                                 C.POINTER(abi.RfResult)]
    L.kas_failure_text.restype = C.c_int
    L.kas_failure_text.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_char_p, C.c_int]
    L.kas_impact_device.restype = C.c_int
    L.kas_impact_device.argtypes = [C.c_void_p, C.POINTER(abi.Tables), C.POINTER(abi.ImpactTables), C.c_void_p]
    L.kas_impact_device16.restype = C.c_int
    L.kas_impact_device16.argtypes = [C.c_void_p, C.POINTER(abi.Tables), C.POINTER(abi.ImpactTables), C.c_void_p]
    L.kas_solve_host_impact.restype = C.c_int
    L.kas_solve_host_impact.argtypes = [C.c_void_p, C.POINTER(abi.BatchDesc), C.POINTER(abi.Tables),
                                        C.POINTER(C.c_int32), C.c_int32, C.POINTER(abi.ImpactTables)]
    L.kas_solve_host16_impact.restype = C.c_int
    L.kas_solve_host16_impact.argtypes = [C.c_void_p, C.POINTER(abi.BatchDesc), C.POINTER(abi.Tables),
                                          C.POINTER(C.c_int32), C.c_int32, C.POINTER(abi.ImpactTables)]
    for fn in (L.kas_rack_impact_device, L.kas_rack_impact_device16):
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.POINTER(abi.Tables), C.POINTER(abi.ImpactTables), C.c_void_p, C.POINTER(abi.RackTables), C.c_void_p]
    for fn in (L.kas_solve_host_rack_impact, L.kas_solve_host16_rack_impact):
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.POINTER(abi.BatchDesc), C.POINTER(abi.Tables), C.POINTER(C.c_int32), C.c_int32,
                       C.POINTER(abi.ImpactTables), C.c_void_p, C.POINTER(abi.RackTables)]
    for fn in (L.kas_topic_impact_device, L.kas_topic_impact_device16):
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.POINTER(abi.Tables), C.POINTER(abi.TopicImpactTables), C.c_void_p]
    for fn in (L.kas_solve_host_topic_impact, L.kas_solve_host16_topic_impact):
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.POINTER(abi.BatchDesc), C.POINTER(abi.Tables), C.POINTER(C.c_int32), C.c_int32,
                       C.POINTER(abi.ImpactTables), C.POINTER(abi.TopicImpactTables)]
    L.kas_rank_device.restype = C.c_int
    L.kas_rank_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(abi.ChooseSpec), C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p]
    for fn in (L.kas_choose_device, L.kas_choose_device16):
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.POINTER(abi.Tables), C.POINTER(abi.ImpactTables), C.POINTER(abi.ChooseSpec),
                       C.POINTER(abi.Choice), C.c_void_p]
    for fn in (L.kas_solve_host_choose, L.kas_solve_host16_choose):
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.POINTER(abi.BatchDesc), C.POINTER(abi.Tables), C.POINTER(abi.ChooseSpec),
                       C.POINTER(abi.Choice), C.POINTER(abi.ImpactTables)]
    for fn in (L.kas_moves_device, L.kas_moves_device16):
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.POINTER(abi.Tables), C.c_void_p, C.c_int32, C.POINTER(abi.Moves), C.c_void_p]
    for fn in (L.kas_solve_host_moves, L.kas_solve_host16_moves):
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.POINTER(abi.BatchDesc), C.POINTER(abi.Tables), C.POINTER(C.c_int32), C.c_int32, C.POINTER(abi.Moves)]
    for fn in (L.kas_batches_device, L.kas_batches_device16):
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.POINTER(abi.Tables), C.c_void_p, C.c_int32, C.POINTER(abi.BatchSpec), C.POINTER(abi.Batches), C.c_void_p]
    for fn in (L.kas_solve_host_batches, L.kas_solve_host16_batches):
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.POINTER(abi.BatchDesc), C.POINTER(abi.Tables), C.POINTER(C.c_int32), C.c_int32, C.POINTER(abi.BatchSpec),
                       C.POINTER(abi.Batches)]
    for fn in (L.kas_rounds_device, L.kas_rounds_device16):
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.POINTER(abi.Tables), C.c_void_p, C.c_int32, C.POINTER(abi.RoundSpec), C.POINTER(abi.Rounds), C.c_void_p]
    for fn in (L.kas_solve_host_rounds, L.kas_solve_host16_rounds):
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.POINTER(abi.BatchDesc), C.POINTER(abi.Tables), C.POINTER(C.c_int32), C.c_int32, C.POINTER(abi.RoundSpec),
                       C.POINTER(abi.Rounds)]
    for fn in (L.kas_solve_host_choose_moves, L.kas_solve_host16_choose_moves):
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.POINTER(abi.BatchDesc), C.POINTER(abi.Tables), C.POINTER(abi.ChooseSpec),
                       C.POINTER(abi.Choice), C.POINTER(abi.ImpactTables), C.POINTER(abi.Moves)]
    L.kas_front_rank_device.restype = C.c_int
    L.kas_front_rank_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(abi.FrontSpec), C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p]
    for fn in (L.kas_front_device, L.kas_front_device16):
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.POINTER(abi.Tables), C.POINTER(abi.ImpactTables), C.POINTER(abi.FrontSpec),
                       C.POINTER(abi.Choice), C.c_void_p, C.c_void_p]
    for fn in (L.kas_solve_host_front, L.kas_solve_host16_front):
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.POINTER(abi.BatchDesc), C.POINTER(abi.Tables), C.POINTER(abi.FrontSpec),
                       C.POINTER(abi.Choice), C.c_void_p, C.POINTER(abi.ImpactTables), C.POINTER(abi.Moves)]
    # the *_racks entries: their parents' prototypes with the scenario rack records (device entries) or report_rack and
    # kas_rack_tables (host entries) added
    L.kas_rank_device_racks.restype = C.c_int
    L.kas_rank_device_racks.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(abi.ChooseSpec), C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p]
    L.kas_front_rank_device_racks.restype = C.c_int
    L.kas_front_rank_device_racks.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(abi.FrontSpec), C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    for fn in (L.kas_choose_device_racks, L.kas_choose_device16_racks):
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.POINTER(abi.Tables), C.POINTER(abi.ImpactTables), C.c_void_p, C.POINTER(abi.ChooseSpec),
                       C.POINTER(abi.Choice), C.c_void_p]
    for fn in (L.kas_front_device_racks, L.kas_front_device16_racks):
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.POINTER(abi.Tables), C.POINTER(abi.ImpactTables), C.c_void_p, C.POINTER(abi.FrontSpec),
                       C.POINTER(abi.Choice), C.c_void_p, C.c_void_p]
    for fn in (L.kas_solve_host_choose_racks, L.kas_solve_host16_choose_racks):
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.POINTER(abi.BatchDesc), C.POINTER(abi.Tables), C.POINTER(abi.ChooseSpec), C.POINTER(abi.Choice),
                       C.POINTER(abi.ImpactTables), C.POINTER(abi.Moves), C.c_void_p, C.POINTER(abi.RackTables)]
    for fn in (L.kas_solve_host_front_racks, L.kas_solve_host16_front_racks):
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.POINTER(abi.BatchDesc), C.POINTER(abi.Tables), C.POINTER(abi.FrontSpec), C.POINTER(abi.Choice),
                       C.c_void_p, C.POINTER(abi.ImpactTables), C.POINTER(abi.Moves), C.c_void_p, C.POINTER(abi.RackTables)]
    # the *_topics entries: the *_racks prototypes with the scenario topic records (device entries) or kas_topic_impact_tables
    # (host entries) added
    L.kas_rank_device_topics.restype = C.c_int
    L.kas_rank_device_topics.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(abi.ChooseSpec),
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.kas_front_rank_device_topics.restype = C.c_int
    L.kas_front_rank_device_topics.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(abi.FrontSpec),
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    for fn in (L.kas_choose_device_topics, L.kas_choose_device16_topics):
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.POINTER(abi.Tables), C.POINTER(abi.ImpactTables), C.c_void_p, C.c_void_p, C.POINTER(abi.ChooseSpec),
                       C.POINTER(abi.Choice), C.c_void_p]
    for fn in (L.kas_front_device_topics, L.kas_front_device16_topics):
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.POINTER(abi.Tables), C.POINTER(abi.ImpactTables), C.c_void_p, C.c_void_p, C.POINTER(abi.FrontSpec),
                       C.POINTER(abi.Choice), C.c_void_p, C.c_void_p]
    for fn in (L.kas_solve_host_choose_topics, L.kas_solve_host16_choose_topics):
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.POINTER(abi.BatchDesc), C.POINTER(abi.Tables), C.POINTER(abi.ChooseSpec), C.POINTER(abi.Choice),
                       C.POINTER(abi.ImpactTables), C.POINTER(abi.Moves), C.c_void_p, C.POINTER(abi.RackTables),
                       C.POINTER(abi.TopicImpactTables)]
    for fn in (L.kas_solve_host_front_topics, L.kas_solve_host16_front_topics):
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.POINTER(abi.BatchDesc), C.POINTER(abi.Tables), C.POINTER(abi.FrontSpec), C.POINTER(abi.Choice),
                       C.c_void_p, C.POINTER(abi.ImpactTables), C.POINTER(abi.Moves), C.c_void_p, C.POINTER(abi.RackTables),
                       C.POINTER(abi.TopicImpactTables)]
    if L.kas_abi_version() != abi.KAS_ABI_VERSION:
        raise ImportError("libkas_hip.so ABI version mismatch")
    _LIB = L
    return L


def _check(rc: int):
    if rc != 0:
        L = load()
        raise KasError(rc, (L.kas_last_error() or b"").decode() or L.kas_strerror(rc).decode())


def resolve_replication_factor(partition_ids, list_sizes, desired_rf: int, n_brokers: int) -> "abi.RfResult":
    """kas_resolve_replication_factor (KTA:47-69; host arithmetic, needs no device): entries in the caller's map order."""
    pid = np.ascontiguousarray(partition_ids, dtype=np.int32)
    ls = np.ascontiguousarray(list_sizes, dtype=np.int32)
    assert pid.shape == ls.shape and pid.ndim == 1
    res = abi.RfResult()
    _check(load().kas_resolve_replication_factor(pid.ctypes.data_as(C.POINTER(C.c_int32)), ls.ctypes.data_as(C.POINTER(C.c_int32)),
                                                 int(pid.size), int(desired_rf), int(n_brokers), C.byref(res)))
    return res


def failure_text(topic, status: int, fail_partition: int = -1, rf: int = -1, list_size: int = -1) -> str:
    """kas_failure_text: the message of the exception the reference throws for this status ('' where it has none)."""
    buf = C.create_string_buffer(1024)
    n = load().kas_failure_text(None if topic is None else str(topic).encode("utf-8"), int(status), int(fail_partition), int(rf),
                                int(list_size), buf, 1024)
    return buf.raw[:n].decode("utf-8")


class DeviceContext:
    """kas_ctx: one HIP device + stream."""

    def __init__(self, device: int = 0):
        self._lib = load()
        self._h = C.c_void_p()
        _check(self._lib.kas_ctx_create(device, C.byref(self._h)))
        self.device = device

    def synchronize(self):
        _check(self._lib.kas_ctx_synchronize(self._h))

    def lds_lane_order(self):
        """(state, lane-operations checked): kas_ctx_lds_lane_order — 1 the LDS served every checked atomic-with-return in
        lane order, 0 violated, -1 the self-test could not run, -2 switched off (KAS_NO_LANE_ORDER=1)."""
        n = C.c_int64()
        self._lib.kas_ctx_lds_lane_order.restype = C.c_int
        self._lib.kas_ctx_lds_lane_order.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        return int(self._lib.kas_ctx_lds_lane_order(self._h, C.byref(n))), n.value

    def host_stats(self):
        """(kas_solve_host calls, calls served by a cached plan, device allocations made)."""
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        _check(self._lib.kas_ctx_host_stats(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def close(self):
        if self._h:
            self._lib.kas_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Plan:
    """kas_plan: validated batch shape with descriptors and node tables resident in HBM."""

    def __init__(self, ctx: DeviceContext, fb: FlatBatch, cells16: bool = False):
        """cells16: kas_plan_create16 — the plan's solves read and write uint16 node-index cells (solve_device with
        pointers to uint16 pools; fb.node_id is not read)."""
        self._lib = load()
        self._ctx = ctx
        self._fb = fb                      # keeps the host descriptor arrays alive
        self.cells16 = bool(cells16)
        bd = batch_desc(fb)
        self._h = C.c_void_p()
        if cells16:
            bd.node_id = None
            _check(self._lib.kas_plan_create16(ctx._h, C.byref(bd), C.byref(self._h)))
        else:
            _check(self._lib.kas_plan_create(ctx._h, C.byref(bd), C.byref(self._h)))

    @property
    def algorithmic_bytes(self) -> int:
        return int(self._lib.kas_plan_algorithmic_bytes(self._h))

    def solve_device(self, cur: int, out: int, topic_results: int, scenario_results: int,
                     aux: int = 0, ctx: int = 0, stream: int = 0):
        """Enqueue one solve; every argument is a raw device pointer (int)."""
        t = abi.Tables()
        t.cur = cur or None; t.out = out or None; t.aux = aux or None; t.ctx = ctx or None
        t.topic_results = topic_results or None; t.scenario_results = scenario_results or None
        fn = self._lib.kas_solve_device16 if self.cells16 else self._lib.kas_solve_device
        _check(fn(self._h, C.byref(t), C.c_void_p(stream) if stream else None))

    def impact_device(self, cur: int, out: int, topic_results: int, nodes: int, scenarios: int, aux: int = 0,
                      stream: int = 0):
        """kas_impact_device / 16: the impact of this plan's previous solve, from the tables it used, into the device arrays
        `nodes` (kas_node_impact [sum of n_nodes]) and `scenarios` (kas_scenario_impact [S]).  Raw device pointers (int)."""
        t = abi.Tables()
        t.cur = cur or None; t.out = out or None; t.aux = aux or None; t.topic_results = topic_results or None
        imp = abi.ImpactTables(nodes or None, scenarios or None)
        fn = self._lib.kas_impact_device16 if self.cells16 else self._lib.kas_impact_device
        _check(fn(self._h, C.byref(t), C.byref(imp), C.c_void_p(stream) if stream else None))

    def topic_impact_device(self, cur: int, out: int, topic_results: int, topics: int, scenarios: int, aux: int = 0, stream: int = 0):
        """kas_topic_impact_device / 16: the topic impact of this plan's previous solve, from the tables it used, into the device
        arrays `topics` (kas_topic_impact [T]) and `scenarios` (kas_scenario_topic_impact [S]).  Raw device pointers (int)."""
        t = abi.Tables()
        t.cur = cur or None; t.out = out or None; t.aux = aux or None; t.topic_results = topic_results or None
        tp = abi.TopicImpactTables(topics or None, scenarios or None)
        fn = self._lib.kas_topic_impact_device16 if self.cells16 else self._lib.kas_topic_impact_device
        _check(fn(self._h, C.byref(t), C.byref(tp), C.c_void_p(stream) if stream else None))

    def rack_impact_device(self, cur: int, out: int, topic_results: int, nodes: int, scenarios: int, racks: int, racks_cap: int,
                           rack_scenarios: int, report_rack=None, aux: int = 0, stream: int = 0) -> np.ndarray:
        """kas_rack_impact_device / 16: the rack impact of this plan's previous solve and impact pass (whose records are the
        device arrays `nodes` / `scenarios`) into the device arrays `racks` (kas_rack_impact [racks_cap]) and `rack_scenarios`
        (kas_scenario_rack_impact [S]).  report_rack: host int32 [node_pool_len] or None (the batch's node_rack).  Raw device
        pointers (int).  Returns rack_off, int64 [S + 1]."""
        t = abi.Tables()
        t.cur = cur or None; t.out = out or None; t.aux = aux or None; t.topic_results = topic_results or None
        imp = abi.ImpactTables(nodes or None, scenarios or None)
        rack_off = np.zeros(self._fb.n_scenarios + 1, dtype=np.int64)
        rep = None if report_rack is None else np.ascontiguousarray(report_rack, dtype=np.int32)
        rk = abi.RackTables(racks or None, rack_scenarios or None, rack_off.ctypes.data, int(racks_cap))
        fn = self._lib.kas_rack_impact_device16 if self.cells16 else self._lib.kas_rack_impact_device
        _check(fn(self._h, C.byref(t), C.byref(imp), None if rep is None else C.c_void_p(rep.ctypes.data), C.byref(rk),
                  C.c_void_p(stream) if stream else None))
        return rack_off

    def choose_device(self, keys, k: int, out: int, scenario_results: int, nodes: int, scenarios: int, rank: int, chosen: int,
                      row_off: int, node_off: int, n_ok: int, rows: int, rows_cap: int, choice_nodes: int, nodes_cap: int,
                      stream: int = 0):
        """kas_choose_device / 16: rank this plan's previous solve and impact pass by `keys` (criterion names, abi.KEY_NAMES)
        and gather the k best scenarios' rows (from `out`) and node blocks (from `nodes`) into `rows` / `choice_nodes`.  Raw
        device pointers (int): rank int32 [S], chosen int32 [k], row_off / node_off int64 [k + 1], n_ok int32 [1]."""
        t = abi.Tables()
        t.out = out or None; t.scenario_results = scenario_results or None
        imp = abi.ImpactTables(nodes or None, scenarios or None)
        spec = abi.choose_spec(keys, k)
        ch = abi.Choice(rank or None, chosen or None, row_off or None, node_off or None, n_ok or None, rows or None, int(rows_cap),
                        choice_nodes or None, int(nodes_cap))
        fn = self._lib.kas_choose_device16 if self.cells16 else self._lib.kas_choose_device
        _check(fn(self._h, C.byref(t), C.byref(imp), C.byref(spec), C.byref(ch), C.c_void_p(stream) if stream else None))

    def front_device(self, spec, out: int, scenario_results: int, nodes: int, scenarios: int, rank: int, chosen: int,
                     row_off: int, node_off: int, n_ok: int, rows: int, rows_cap: int, choice_nodes: int, nodes_cap: int, counts: int,
                     stream: int = 0):
        """kas_front_device / 16: choose_device with the Pareto front under `spec` (abi.front_spec) in place of the ranking;
        counts: int32 [4] on the device (n_ok, n_eligible, n_front, 0).  Raw device pointers (int)."""
        t = abi.Tables()
        t.out = out or None; t.scenario_results = scenario_results or None
        imp = abi.ImpactTables(nodes or None, scenarios or None)
        ch = abi.Choice(rank or None, chosen or None, row_off or None, node_off or None, n_ok or None, rows or None, int(rows_cap),
                        choice_nodes or None, int(nodes_cap))
        fn = self._lib.kas_front_device16 if self.cells16 else self._lib.kas_front_device
        _check(fn(self._h, C.byref(t), C.byref(imp), C.byref(spec), C.byref(ch), counts or None, C.c_void_p(stream) if stream else None))

    def choose_device_racks(self, keys, k: int, out: int, scenario_results: int, nodes: int, scenarios: int, rack_scenarios: int,
                            rank: int, chosen: int, row_off: int, node_off: int, n_ok: int, rows: int, rows_cap: int, choice_nodes: int,
                            nodes_cap: int, stream: int = 0):
        """kas_choose_device_racks / 16: choose_device with `rack_scenarios`, the device array of scenario rack records this plan's
        rack pass wrote (rack_impact_device), as a third source of criteria: `keys` names abi.KEY_NAMES and abi.RACK_KEY_NAMES."""
        t = abi.Tables()
        t.out = out or None; t.scenario_results = scenario_results or None
        imp = abi.ImpactTables(nodes or None, scenarios or None)
        spec = abi.rack_choose_spec(keys, k)
        ch = abi.Choice(rank or None, chosen or None, row_off or None, node_off or None, n_ok or None, rows or None, int(rows_cap),
                        choice_nodes or None, int(nodes_cap))
        fn = self._lib.kas_choose_device16_racks if self.cells16 else self._lib.kas_choose_device_racks
        _check(fn(self._h, C.byref(t), C.byref(imp), rack_scenarios or None, C.byref(spec), C.byref(ch), C.c_void_p(stream) if stream else None))

    def front_device_racks(self, spec, out: int, scenario_results: int, nodes: int, scenarios: int, rack_scenarios: int, rank: int,
                           chosen: int, row_off: int, node_off: int, n_ok: int, rows: int, rows_cap: int, choice_nodes: int,
                           nodes_cap: int, counts: int, stream: int = 0):
        """kas_front_device_racks / 16: front_device with the scenario rack records; `spec`: abi.rack_front_spec."""
        t = abi.Tables()
        t.out = out or None; t.scenario_results = scenario_results or None
        imp = abi.ImpactTables(nodes or None, scenarios or None)
        ch = abi.Choice(rank or None, chosen or None, row_off or None, node_off or None, n_ok or None, rows or None, int(rows_cap),
                        choice_nodes or None, int(nodes_cap))
        fn = self._lib.kas_front_device16_racks if self.cells16 else self._lib.kas_front_device_racks
        _check(fn(self._h, C.byref(t), C.byref(imp), rack_scenarios or None, C.byref(spec), C.byref(ch), counts or None,
                  C.c_void_p(stream) if stream else None))

    def choose_device_topics(self, keys, k: int, out: int, scenario_results: int, nodes: int, scenarios: int, rack_scenarios: int,
                             topic_scenarios: int, rank: int, chosen: int, row_off: int, node_off: int, n_ok: int, rows: int, rows_cap: int,
                             choice_nodes: int, nodes_cap: int, stream: int = 0):
        """kas_choose_device_topics / 16: choose_device_racks with `topic_scenarios`, the device array of scenario topic records
        this plan's topic pass wrote (topic_impact_device), as a further source of criteria: `keys` names abi.KEY_NAMES,
        abi.RACK_KEY_NAMES and abi.TOPIC_KEY_NAMES.  rack_scenarios / topic_scenarios may be 0 when no criterion of the set is named."""
        t = abi.Tables()
        t.out = out or None; t.scenario_results = scenario_results or None
        imp = abi.ImpactTables(nodes or None, scenarios or None)
        spec = abi.topic_choose_spec(keys, k)
        ch = abi.Choice(rank or None, chosen or None, row_off or None, node_off or None, n_ok or None, rows or None, int(rows_cap),
                        choice_nodes or None, int(nodes_cap))
        fn = self._lib.kas_choose_device16_topics if self.cells16 else self._lib.kas_choose_device_topics
        _check(fn(self._h, C.byref(t), C.byref(imp), rack_scenarios or None, topic_scenarios or None, C.byref(spec), C.byref(ch),
                  C.c_void_p(stream) if stream else None))

    def front_device_topics(self, spec, out: int, scenario_results: int, nodes: int, scenarios: int, rack_scenarios: int,
                            topic_scenarios: int, rank: int, chosen: int, row_off: int, node_off: int, n_ok: int, rows: int, rows_cap: int,
                            choice_nodes: int, nodes_cap: int, counts: int, stream: int = 0):
        """kas_front_device_topics / 16: front_device_racks with the scenario topic records; `spec`: abi.topic_front_spec."""
        t = abi.Tables()
        t.out = out or None; t.scenario_results = scenario_results or None
        imp = abi.ImpactTables(nodes or None, scenarios or None)
        ch = abi.Choice(rank or None, chosen or None, row_off or None, node_off or None, n_ok or None, rows or None, int(rows_cap),
                        choice_nodes or None, int(nodes_cap))
        fn = self._lib.kas_front_device16_topics if self.cells16 else self._lib.kas_front_device_topics
        _check(fn(self._h, C.byref(t), C.byref(imp), rack_scenarios or None, topic_scenarios or None, C.byref(spec), C.byref(ch),
                  counts or None, C.c_void_p(stream) if stream else None))

    def moves_device(self, mask, select: int, n_select: int, cur: int, out: int, topic_results: int, move_off: int, cell_off: int,
                     moves: int, moves_cap: int, cells: int, cells_cap: int, aux: int = 0, stream: int = 0):
        """kas_moves_device / 16: the moves (kinds `mask`: names of abi.MOVE_KINDS or a KAS_MOVE_* mask) of this plan's previous
        solve for the scenarios in the device array `select` (int32 [n_select]; a choice's chosen[] as it is) into the device
        arrays move_off / cell_off (int64 [n_select + 1]), moves (kas_move [moves_cap]) and cells.  Raw device pointers (int)."""
        t = abi.Tables()
        t.cur = cur or None; t.out = out or None; t.aux = aux or None; t.topic_results = topic_results or None
        mv = abi.Moves(abi.move_mask(mask), 0, move_off or None, cell_off or None, moves or None, int(moves_cap), cells or None, int(cells_cap))
        fn = self._lib.kas_moves_device16 if self.cells16 else self._lib.kas_moves_device
        _check(fn(self._h, C.byref(t), select or None, int(n_select), C.byref(mv), C.c_void_p(stream) if stream else None))

    def batches_device(self, caps, select: int, n_select: int, cur: int, out: int, topic_results: int, scenarios: int, batches: int = 0,
                       stride: int = 0, aux: int = 0, stream: int = 0):
        """kas_batches_device / 16: the execution batches (caps: abi.batch_spec) of this plan's previous solve for the scenarios in
        the device array `select` (int32 [n_select]; a choice's chosen[] as it is) into the device arrays scenarios
        (kas_scenario_batches [n_select]) and batches (kas_move_batch [n_select * stride]; 0 with stride 0: the counts only).
        Raw device pointers (int)."""
        t = abi.Tables()
        t.cur = cur or None; t.out = out or None; t.aux = aux or None; t.topic_results = topic_results or None
        spec = abi.batch_spec(caps)
        o = abi.Batches(scenarios or None, batches or None, int(stride))
        fn = self._lib.kas_batches_device16 if self.cells16 else self._lib.kas_batches_device
        _check(fn(self._h, C.byref(t), select or None, int(n_select), C.byref(spec), C.byref(o), C.c_void_p(stream) if stream else None))

    def rounds_device(self, caps, select: int, n_select: int, cur: int, out: int, topic_results: int, scenarios: int, rounds: int = 0,
                      round_stride: int = 0, round_of: int = 0, move_stride: int = 0, aux: int = 0, stream: int = 0):
        """kas_rounds_device / 16: the packed rounds (caps: abi.round_spec) of this plan's previous solve for the scenarios in the
        device array `select` (int32 [n_select]; a choice's chosen[] as it is) into the device arrays scenarios
        (kas_scenario_rounds [n_select]), rounds (kas_move_round [n_select * round_stride]) and round_of (int32 [n_select *
        move_stride]); 0 with stride 0: none of that kind.  Raw device pointers (int)."""
        t = abi.Tables()
        t.cur = cur or None; t.out = out or None; t.aux = aux or None; t.topic_results = topic_results or None
        spec = abi.round_spec(caps)
        o = abi.Rounds(scenarios or None, rounds or None, int(round_stride), round_of or None, int(move_stride))
        fn = self._lib.kas_rounds_device16 if self.cells16 else self._lib.kas_rounds_device
        _check(fn(self._h, C.byref(t), select or None, int(n_select), C.byref(spec), C.byref(o), C.c_void_p(stream) if stream else None))

    def set_flags(self, flags: int):
        _check(self._lib.kas_plan_set_flags(self._h, flags))

    def describe(self) -> str:
        """The kernels a solve of this plan launches (template arguments, grids, LDS)."""
        buf = C.create_string_buffer(512)
        n = self._lib.kas_plan_describe(self._h, buf, 512)
        if n < 0:
            _check(n)
        return buf.value.decode()

    def stats(self) -> np.ndarray:
        """Per-scenario device counters of the last solve: int64 [S, 16] =
        (setup, P2, P3+P4, P5 time in 10 ns ticks; P4 windows, P4 node steps, P5 rounds,
        P2 overflow tiles)."""
        n = self._fb.n_scenarios
        a = np.zeros((n, 16), dtype=np.int64)
        _check(self._lib.kas_plan_stats(self._h, a.ctypes.data_as(C.POINTER(C.c_int64)), a.size))
        return a

    def kernel_time_us(self):
        avg = C.c_double(); n = C.c_int()
        _check(self._lib.kas_plan_kernel_time_us(self._h, C.byref(avg), C.byref(n)))
        return avg.value, n.value

    def phase_times_us(self):
        """(fill kernel avg us, order kernel avg us, launches) since the last call."""
        f = C.c_double(); o = C.c_double(); n = C.c_int()
        _check(self._lib.kas_plan_phase_times_us(self._h, C.byref(f), C.byref(o), C.byref(n)))
        return f.value, o.value, n.value

    def close(self):
        if self._h:
            self._lib.kas_plan_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_DEFAULT_CTX: Optional[DeviceContext] = None


def default_context() -> DeviceContext:
    global _DEFAULT_CTX
    if _DEFAULT_CTX is None:
        _DEFAULT_CTX = DeviceContext(int(os.environ.get("LOCAL_RANK", "0")) if
                                     load().kas_device_count() > 1 else 0)
    return _DEFAULT_CTX


def solve_host(fb: FlatBatch, ctx: Optional[DeviceContext] = None) -> HostOutputs:
    """kas_solve_host: copy in, solve on the GPU, copy out (blocking)."""
    L = load()
    ctx = ctx or default_context()
    bd = batch_desc(fb)
    t, ho = host_tables(fb)
    _check(L.kas_solve_host(ctx._h, C.byref(bd), C.byref(t)))
    return ho


def selected_out_len(fb: FlatBatch, select) -> int:
    """int32 cells kas_solve_host_select returns for the scenarios in `select` (their rows, packed)."""
    n = 0
    for s in select:
        if not 0 <= int(s) < fb.n_scenarios:
            continue                       # (the library refuses the call: KAS_E_INVALID_ARG)
        sd = fb.scen[int(s)]
        t = fb.topics[int(sd["topic_begin"]): int(sd["topic_begin"]) + int(sd["topic_count"])]
        n += int((t["n_partitions"].astype(np.int64) * t["out_width"]).sum())
    return n


def solve_host_select(fb: FlatBatch, select, ctx: Optional[DeviceContext] = None, ho: Optional[HostOutputs] = None,
                      tables=None) -> HostOutputs:
    """kas_solve_host_select: every scenario is solved and reports its records, rows come back only
    for the scenarios in `select`, packed in that order (the what-if form: one assignment printed)."""
    L = load()
    ctx = ctx or default_context()
    bd = batch_desc(fb)
    sel = np.ascontiguousarray(select, dtype=np.int32)
    if tables is None:
        tables, ho = host_tables(fb, out_len=selected_out_len(fb, sel))
    _check(L.kas_solve_host_select(ctx._h, C.byref(bd), C.byref(tables),
                                   sel.ctypes.data_as(C.POINTER(C.c_int32)), int(sel.size)))
    return ho


def solve_host16(fb: FlatBatch, ctx: Optional[DeviceContext] = None, select=None, cur16=None, tables=None,
                 ho: Optional[HostOutputs] = None) -> HostOutputs:
    """kas_solve_host16: the host call with 16-bit cells (node indices; flatten.to_cells16 / cells16_to_ids).
    HostOutputs.out is the uint16 out pool; select = scenario indices whose rows come back packed (None: every row)."""
    from .flatten import host_tables16, to_cells16
    L = load()
    ctx = ctx or default_context()
    bd = batch_desc(fb)
    bd.node_id = None                      # (not read: node i has id i)
    sel = None if select is None else np.ascontiguousarray(select, dtype=np.int32)
    if tables is None:
        cur16 = to_cells16(fb) if cur16 is None else cur16
        tables, ho = host_tables16(fb, cur16, out_len=None if sel is None else selected_out_len(fb, sel))
    _check(L.kas_solve_host16(ctx._h, C.byref(bd), C.byref(tables),
                              None if sel is None else sel.ctypes.data_as(C.POINTER(C.c_int32)),
                              -1 if sel is None else int(sel.size)))
    return ho


def impact_arrays(fb: FlatBatch):
    """Zeroed host arrays for the impact records of `fb`: (nodes NODE_IMPACT_DTYPE [sum of n_nodes], scenarios
    SCENARIO_IMPACT_DTYPE [S]); scenario s's block of nodes starts at node_blocks(fb)[s]."""
    n = int(np.clip(fb.scen["n_nodes"], 0, None).sum())
    return (np.zeros(max(n, 1), dtype=abi.NODE_IMPACT_DTYPE)[:n],
            np.zeros(max(fb.n_scenarios, 1), dtype=abi.SCENARIO_IMPACT_DTYPE)[:fb.n_scenarios])


def node_blocks(fb: FlatBatch) -> np.ndarray:
    """int64 [S + 1]: where each scenario's block of node impact records starts (and the total behind the last)."""
    return np.concatenate([[0], np.cumsum(np.clip(fb.scen["n_nodes"], 0, None).astype(np.int64))]).astype(np.int64)


def solve_host_impact(fb: FlatBatch, select=None, cells16: bool = False, ctx: Optional[DeviceContext] = None):
    """kas_solve_host_impact / kas_solve_host16_impact: the host call plus the per-broker impact of every scenario.
    select=None: every row in place (HostOutputs.out is the whole out pool); a list of scenario indices: their rows, packed
    (kas_solve_host_select); an empty list: no rows at all, the what-if call.  cells16: 16-bit node-index cells
    (HostOutputs.out is then uint16).  Returns (HostOutputs, nodes, scenarios) — see impact_arrays."""
    from .flatten import host_tables16, to_cells16
    L = load()
    ctx = ctx or default_context()
    bd = batch_desc(fb)
    sel = None if select is None else np.ascontiguousarray(select, dtype=np.int32)
    out_len = None if sel is None else selected_out_len(fb, sel)
    if cells16:
        bd.node_id = None
        cur16 = to_cells16(fb)
        t, ho = host_tables16(fb, cur16, out_len=out_len)
    else:
        t, ho = host_tables(fb, out_len=out_len)
    nodes, scen = impact_arrays(fb)
    imp = abi.ImpactTables(nodes.ctypes.data if nodes.size else None, scen.ctypes.data if scen.size else None)
    fn = L.kas_solve_host16_impact if cells16 else L.kas_solve_host_impact
    _check(fn(ctx._h, C.byref(bd), C.byref(t), None if sel is None or sel.size == 0 else sel.ctypes.data_as(C.POINTER(C.c_int32)),
              -1 if sel is None else int(sel.size), C.byref(imp)))
    return ho, nodes, scen


def topic_impact_arrays(fb: FlatBatch):
    """Zeroed host arrays for the topic pass's records of `fb`: (topics TOPIC_IMPACT_DTYPE [T], scenarios
    SCENARIO_TOPIC_IMPACT_DTYPE [S])."""
    return (np.zeros(max(fb.n_topics, 1), dtype=abi.TOPIC_IMPACT_DTYPE)[:fb.n_topics],
            np.zeros(max(fb.n_scenarios, 1), dtype=abi.SCENARIO_TOPIC_IMPACT_DTYPE)[:fb.n_scenarios])


@dataclass
class TopicReport:
    """What kas_solve_host_topic_impact returns beside the solve."""
    topics: np.ndarray                   # TOPIC_IMPACT_DTYPE [T], in descriptor order
    scenarios: np.ndarray                # SCENARIO_TOPIC_IMPACT_DTYPE [S]
    nodes: Optional[np.ndarray] = None   # the node impact records, when they were asked for
    impact: Optional[np.ndarray] = None  # every scenario's kas_scenario_impact, when the impact pass ran


def solve_host_topic_impact(fb: FlatBatch, select=None, cells16: bool = False, impact: bool = True, nodes: bool = True,
                            ctx: Optional[DeviceContext] = None):
    """kas_solve_host_topic_impact / 16: solve_host_impact plus the topic pass.  impact=False: host_impact == NULL, no impact
    pass runs; nodes=False: the node records stay on the device (host_impact->nodes == NULL).  select, cells16: as in
    solve_host_impact.  Returns (HostOutputs, TopicReport)."""
    from .flatten import host_tables16, to_cells16
    L = load()
    ctx = ctx or default_context()
    bd = batch_desc(fb)
    sel = None if select is None else np.ascontiguousarray(select, dtype=np.int32)
    out_len = None if sel is None else selected_out_len(fb, sel)
    if cells16:
        bd.node_id = None
        cur16 = to_cells16(fb)
        t, ho = host_tables16(fb, cur16, out_len=out_len)
    else:
        t, ho = host_tables(fb, out_len=out_len)
    n_rec, scen = impact_arrays(fb)
    imp = abi.ImpactTables(n_rec.ctypes.data if (n_rec.size and nodes) else None, scen.ctypes.data if scen.size else None)
    topics, tscen = topic_impact_arrays(fb)
    tp = abi.TopicImpactTables(topics.ctypes.data if topics.size else None, tscen.ctypes.data if tscen.size else None)
    fn = L.kas_solve_host16_topic_impact if cells16 else L.kas_solve_host_topic_impact
    _check(fn(ctx._h, C.byref(bd), C.byref(t), None if sel is None or sel.size == 0 else sel.ctypes.data_as(C.POINTER(C.c_int32)),
              -1 if sel is None else int(sel.size), C.byref(imp) if impact else None, C.byref(tp)))
    return ho, TopicReport(topics=topics, scenarios=tscen, nodes=n_rec if (impact and nodes) else None, impact=scen if impact else None)


def rack_counts(fb: FlatBatch, report_rack=None) -> np.ndarray:
    """int64 [S]: R_s = 1 + the largest rack index of each scenario's nodes in `report_rack` (None: fb.node_rack)."""
    table = fb.node_rack if report_rack is None else np.asarray(report_rack)
    out = np.zeros(fb.n_scenarios, dtype=np.int64)
    for s in range(fb.n_scenarios):
        off, n = int(fb.scen["node_off"][s]), int(fb.scen["n_nodes"][s])
        out[s] = int(table[off:off + n].max()) + 1 if n > 0 else 0
    return out


@dataclass
class RackReport:
    """What kas_solve_host_rack_impact returns beside the solve: scenario s's rack records are racks[rack_off[s]:rack_off[s + 1]]."""
    racks: np.ndarray                    # RACK_IMPACT_DTYPE
    scenarios: np.ndarray                # SCENARIO_RACK_IMPACT_DTYPE [S]
    rack_off: np.ndarray                 # int64 [S + 1]
    nodes: Optional[np.ndarray] = None   # the node impact records, when they were asked for
    impact: Optional[np.ndarray] = None  # every scenario's kas_scenario_impact

    def of(self, s: int) -> np.ndarray:
        return self.racks[int(self.rack_off[s]):int(self.rack_off[s + 1])]


def solve_host_rack_impact(fb: FlatBatch, report_rack=None, select=None, cells16: bool = False, nodes: bool = True,
                           racks_cap: Optional[int] = None, ctx: Optional[DeviceContext] = None):
    """kas_solve_host_rack_impact / 16: solve_host_impact plus the rack pass.  report_rack: int32 [node_pool_len] parallel to
    fb.node_rack, or None (the batch's own racks).  nodes=False: the node records stay on the device (host_impact->nodes ==
    NULL).  racks_cap: the capacity handed to the library (default: exactly what the table needs).
    Returns (HostOutputs, RackReport)."""
    from .flatten import host_tables16, to_cells16
    L = load()
    ctx = ctx or default_context()
    bd = batch_desc(fb)
    sel = None if select is None else np.ascontiguousarray(select, dtype=np.int32)
    out_len = None if sel is None else selected_out_len(fb, sel)
    if cells16:
        bd.node_id = None
        cur16 = to_cells16(fb)
        t, ho = host_tables16(fb, cur16, out_len=out_len)
    else:
        t, ho = host_tables(fb, out_len=out_len)
    n_rec, scen = impact_arrays(fb)
    imp = abi.ImpactTables(n_rec.ctypes.data if (n_rec.size and nodes) else None, scen.ctypes.data if scen.size else None)
    rep = None if report_rack is None else np.ascontiguousarray(report_rack, dtype=np.int32)
    S = fb.n_scenarios
    cap = max(int(rack_counts(fb, rep).sum()), 0) if racks_cap is None else int(racks_cap)
    racks = np.zeros(max(cap, 1), dtype=abi.RACK_IMPACT_DTYPE)
    rscen = np.zeros(max(S, 1), dtype=abi.SCENARIO_RACK_IMPACT_DTYPE)
    rack_off = np.zeros(S + 1, dtype=np.int64)
    rk = abi.RackTables(racks.ctypes.data, rscen.ctypes.data, rack_off.ctypes.data, cap)
    fn = L.kas_solve_host16_rack_impact if cells16 else L.kas_solve_host_rack_impact
    _check(fn(ctx._h, C.byref(bd), C.byref(t), None if sel is None or sel.size == 0 else sel.ctypes.data_as(C.POINTER(C.c_int32)),
              -1 if sel is None else int(sel.size), C.byref(imp), None if rep is None else C.c_void_p(rep.ctypes.data), C.byref(rk)))
    return ho, RackReport(racks=racks[:int(rack_off[S])], scenarios=rscen[:S], rack_off=rack_off, nodes=n_rec if nodes else None, impact=scen)


def rank_device(scenario_results: int, scenario_impact: int, n_scenarios: int, keys, k: int, rank: int, chosen: int, n_ok: int,
                stream: int = 0, ctx: Optional[DeviceContext] = None):
    """kas_rank_device: rank n_scenarios records on the device by `keys` (criterion names, abi.KEY_NAMES).  Raw device pointers
    (int): the two record arrays in, rank int32 [S], chosen int32 [k] and n_ok int32 [1] out.  Asynchronous on `stream`."""
    ctx = ctx or default_context()
    spec = abi.choose_spec(keys, k)
    _check(load().kas_rank_device(ctx._h, scenario_results or None, scenario_impact or None, int(n_scenarios), C.byref(spec),
                                  rank or None, chosen or None, n_ok or None, C.c_void_p(stream) if stream else None))


def packed_cells(fb: FlatBatch) -> np.ndarray:
    """int64 [S]: cells of each scenario's out rows when packed (its topics' P x out_width, as kas_solve_host_select packs them)"""
    per_topic = np.clip(fb.topics["n_partitions"], 0, None).astype(np.int64) * np.clip(fb.topics["out_width"], 0, None)
    cum = np.concatenate([[0], np.cumsum(per_topic)])
    b = fb.scen["topic_begin"].astype(np.int64)
    c = np.clip(fb.scen["topic_count"], 0, None).astype(np.int64)
    return np.where(c > 0, cum[np.minimum(b + c, fb.n_topics)] - cum[np.minimum(b, fb.n_topics)], 0).astype(np.int64)


@dataclass
class Choice:
    """What kas_solve_host_choose leaves (include/kas_abi.h, kas_choice): rows holds row_off[k] cells, nodes node_off[k] records."""
    rank: np.ndarray
    chosen: np.ndarray
    row_off: np.ndarray
    node_off: np.ndarray
    n_ok: int
    rows: np.ndarray
    nodes: np.ndarray
    scenarios: np.ndarray                # every scenario's kas_scenario_impact


def solve_host_choose(fb: FlatBatch, keys, k: int, cells16: bool = False, ctx: Optional[DeviceContext] = None):
    """kas_solve_host_choose / kas_solve_host16_choose: every scenario is solved and reduced to its records on the GPU, which
    also ranks them by `keys` (criterion names, abi.KEY_NAMES; smaller is better, the scenario index breaks ties); rows and
    node impact records come back for the k best only.  Returns (HostOutputs without rows, Choice)."""
    from .flatten import host_tables16, to_cells16
    L = load()
    ctx = ctx or default_context()
    spec = abi.choose_spec(keys, k)
    bd = batch_desc(fb)
    if cells16:
        bd.node_id = None
        cur16 = to_cells16(fb)
        t, ho = host_tables16(fb, cur16, out_len=0)
    else:
        t, ho = host_tables(fb, out_len=0)
    t.out = None
    S, kk = fb.n_scenarios, max(int(k), 0)
    rows_cap = int(np.sort(packed_cells(fb))[::-1][:kk].sum())
    nodes_cap = int(np.sort(np.clip(fb.scen["n_nodes"], 0, None).astype(np.int64))[::-1][:kk].sum())
    c = Choice(rank=np.full(max(S, 1), -9, np.int32)[:S], chosen=np.full(max(kk, 1), -9, np.int32)[:kk],
               row_off=np.full(kk + 1, -9, np.int64), node_off=np.full(kk + 1, -9, np.int64), n_ok=-9,
               rows=np.zeros(max(rows_cap, 1), np.uint16 if cells16 else np.int32)[:rows_cap],
               nodes=np.zeros(max(nodes_cap, 1), abi.NODE_IMPACT_DTYPE)[:nodes_cap],
               scenarios=np.zeros(max(S, 1), abi.SCENARIO_IMPACT_DTYPE)[:S])
    n_ok = np.full(1, -9, np.int32)

    def p(a):
        return a.ctypes.data if a.size else None
    ch = abi.Choice(p(c.rank), p(c.chosen), p(c.row_off), p(c.node_off), p(n_ok), p(c.rows), rows_cap, p(c.nodes), nodes_cap)
    imp = abi.ImpactTables(None, p(c.scenarios))
    fn = L.kas_solve_host16_choose if cells16 else L.kas_solve_host_choose
    _check(fn(ctx._h, C.byref(bd), C.byref(t), C.byref(spec), C.byref(ch), C.byref(imp)))
    c.n_ok = int(n_ok[0])
    c.rows = c.rows[:int(c.row_off[kk])]
    c.nodes = c.nodes[:int(c.node_off[kk])]
    return ho, c


@dataclass
class MoveList:
    """What a moves call leaves (include/kas_abi.h, kas_moves): listed scenario j owns moves[move_off[j]:move_off[j + 1]] and
    cells[cell_off[j]:cell_off[j + 1]]; a record's new list is cells[cell_off[j] + cell_at:][:len].  moves / cells hold what
    the capacities let through; move_off[-1] / cell_off[-1] are the true totals."""
    mask: int
    select: np.ndarray                   # the listed scenarios (a choice: its chosen[])
    move_off: np.ndarray
    cell_off: np.ndarray
    moves: np.ndarray                    # abi.MOVE_DTYPE
    cells: np.ndarray                    # int32 broker ids, or uint16 node indices

    @property
    def truncated(self) -> bool:
        return int(self.move_off[-1]) > self.moves.size or int(self.cell_off[-1]) > self.cells.size

    def of(self, j: int):
        """(records, cells) of listed scenario j: the block's records and its cells (cell_at indexes the latter)"""
        return (self.moves[int(self.move_off[j]):int(self.move_off[j + 1])], self.cells[int(self.cell_off[j]):int(self.cell_off[j + 1])])


def scenario_rows(fb: FlatBatch) -> np.ndarray:
    """int64 [S]: rows of each scenario (its topics' P): the most moves it can have"""
    per_topic = np.clip(fb.topics["n_partitions"], 0, None).astype(np.int64)
    cum = np.concatenate([[0], np.cumsum(per_topic)])
    b = fb.scen["topic_begin"].astype(np.int64)
    c = np.clip(fb.scen["topic_count"], 0, None).astype(np.int64)
    return np.where(c > 0, cum[np.minimum(b + c, fb.n_topics)] - cum[np.minimum(b, fb.n_topics)], 0).astype(np.int64)


def moves_room(fb: FlatBatch, select) -> tuple:
    """(rows, packed cells) of the scenarios in `select` (entries outside 0..S-1 take none): always enough room for their moves"""
    sel = np.asarray(list(select) if not isinstance(select, np.ndarray) else select, dtype=np.int64).reshape(-1)
    sel = sel[(sel >= 0) & (sel < fb.n_scenarios)]
    return int(scenario_rows(fb)[sel].sum()), int(packed_cells(fb)[sel].sum())


def _move_arrays(mask, n, moves_cap, cells_cap, cells16):
    ml = MoveList(mask=abi.move_mask(mask), select=None, move_off=np.full(n + 1, -9, np.int64), cell_off=np.full(n + 1, -9, np.int64),
                  moves=np.zeros(max(moves_cap, 1), abi.MOVE_DTYPE)[:moves_cap],
                  cells=np.zeros(max(cells_cap, 1), np.uint16 if cells16 else np.int32)[:cells_cap])
    mv = abi.Moves(ml.mask, 0, ml.move_off.ctypes.data, ml.cell_off.ctypes.data, ml.moves.ctypes.data if moves_cap else None, moves_cap,
                   ml.cells.ctypes.data if cells_cap else None, cells_cap)
    return ml, mv


def _trim(ml: MoveList):
    n_moves = min(int(ml.move_off[-1]), ml.moves.size)
    ml.moves = ml.moves[:n_moves]
    ml.cells = ml.cells[:min(int(ml.cell_off[-1]), ml.cells.size)]
    return ml


def solve_host_moves(fb: FlatBatch, mask=("replicas",), select=None, cells16: bool = False, moves_cap: Optional[int] = None,
                     cells_cap: Optional[int] = None, ctx: Optional[DeviceContext] = None):
    """kas_solve_host_moves / kas_solve_host16_moves: every scenario is solved and reports its records; no rows come back, but
    the moves of the scenarios in `select` (None: every scenario) under `mask` (kind names of abi.MOVE_KINDS, or a KAS_MOVE_*
    mask).  Capacities default to what is always enough (moves_room).  Returns (HostOutputs without rows, MoveList)."""
    from .flatten import host_tables16, to_cells16
    L = load()
    ctx = ctx or default_context()
    bd = batch_desc(fb)
    if cells16:
        bd.node_id = None
        cur16 = to_cells16(fb)                 # (held until the call returns: the table only borrows it)
        t, ho = host_tables16(fb, cur16, out_len=0)
    else:
        t, ho = host_tables(fb, out_len=0)
    t.out = None
    sel = None if select is None else np.ascontiguousarray(select, dtype=np.int32)
    listed = np.arange(fb.n_scenarios, dtype=np.int32) if sel is None else sel
    room = moves_room(fb, listed)
    ml, mv = _move_arrays(mask, int(listed.size), room[0] if moves_cap is None else int(moves_cap),
                          room[1] if cells_cap is None else int(cells_cap), cells16)
    ml.select = listed
    fn = L.kas_solve_host16_moves if cells16 else L.kas_solve_host_moves
    _check(fn(ctx._h, C.byref(bd), C.byref(t), None if sel is None or sel.size == 0 else sel.ctypes.data_as(C.POINTER(C.c_int32)),
              -1 if sel is None else int(sel.size), C.byref(mv)))
    return ho, _trim(ml)


@dataclass
class BatchList:
    """What a batches call leaves (include/kas_abi.h, kas_batches): one kas_scenario_batches per listed scenario, and listed
    scenario j's first min(n_batches, stride) kas_move_batch records at batches[j * stride:]."""
    spec: "abi.BatchSpec"
    select: np.ndarray                   # the listed scenarios
    scenarios: np.ndarray                # abi.SCENARIO_BATCHES_DTYPE [n]
    batches: np.ndarray                  # abi.MOVE_BATCH_DTYPE [n * stride]
    stride: int

    def truncated(self, j: int) -> bool:
        return int(self.scenarios["n_batches"][j]) > self.stride

    def of(self, j: int) -> np.ndarray:
        """the written records of listed scenario j"""
        n = min(int(self.scenarios["n_batches"][j]), self.stride)
        return self.batches[j * self.stride:j * self.stride + n]


def solve_host_batches(fb: FlatBatch, caps, select=None, stride: int = 0, cells16: bool = False, ctx: Optional[DeviceContext] = None,
                       fill: int = 0):
    """kas_solve_host_batches / kas_solve_host16_batches: every scenario is solved and reports its records; no rows come back, but
    the execution batches of the scenarios in `select` (None: every scenario) under `caps` (abi.batch_spec: a dict with inbound,
    outbound, max_moves).  stride: room for batch records per listed scenario (0: the counts only).  fill: the int32 word the
    output arrays hold before the call (tests: what the call does not write stays).  Returns (HostOutputs without rows, BatchList)."""
    from .flatten import host_tables16, to_cells16
    L = load()
    ctx = ctx or default_context()
    bd = batch_desc(fb)
    if cells16:
        bd.node_id = None
        cur16 = to_cells16(fb)                 # (held until the call returns: the table only borrows it)
        t, ho = host_tables16(fb, cur16, out_len=0)
    else:
        t, ho = host_tables(fb, out_len=0)
    t.out = None
    sel = None if select is None else np.ascontiguousarray(select, dtype=np.int32)
    listed = np.arange(fb.n_scenarios, dtype=np.int32) if sel is None else sel
    n, stride = int(listed.size), int(stride)
    spec = abi.batch_spec(caps)
    scen = np.full(max(n, 1), fill, abi.SCENARIO_BATCHES_DTYPE)[:n]
    recs = np.full(max(n * max(stride, 0), 1), fill, abi.MOVE_BATCH_DTYPE)[:n * max(stride, 0)]
    o = abi.Batches(scen.ctypes.data if n else None, recs.ctypes.data if recs.size else None, stride)
    fn = L.kas_solve_host16_batches if cells16 else L.kas_solve_host_batches
    _check(fn(ctx._h, C.byref(bd), C.byref(t), None if sel is None or sel.size == 0 else sel.ctypes.data_as(C.POINTER(C.c_int32)),
              -1 if sel is None else n, C.byref(spec), C.byref(o)))
    return ho, BatchList(spec=spec, select=listed, scenarios=scen, batches=recs, stride=stride)


@dataclass
class RoundList:
    """What a rounds call leaves (include/kas_abi.h, kas_rounds): one kas_scenario_rounds per listed scenario, listed scenario j's
    first min(n_rounds, round_stride) kas_move_round records at rounds[j * round_stride:] and the rounds of its first
    min(n_moves, move_stride) moves at round_of[j * move_stride:]."""
    spec: "abi.RoundSpec"
    select: np.ndarray                   # the listed scenarios
    scenarios: np.ndarray                # abi.SCENARIO_ROUNDS_DTYPE [n]
    rounds: np.ndarray                   # abi.MOVE_ROUND_DTYPE [n * round_stride]
    round_stride: int
    round_of: np.ndarray                 # int32 [n * move_stride]
    move_stride: int

    def truncated(self, j: int) -> bool:
        return int(self.scenarios["n_rounds"][j]) > self.round_stride or int(self.scenarios["n_moves"][j]) > self.move_stride

    def of(self, j: int) -> np.ndarray:
        """the written round records of listed scenario j"""
        n = min(int(self.scenarios["n_rounds"][j]), self.round_stride)
        return self.rounds[j * self.round_stride:j * self.round_stride + n]

    def round_of_moves(self, j: int) -> np.ndarray:
        """the written rounds of listed scenario j's moves"""
        n = min(int(self.scenarios["n_moves"][j]), self.move_stride)
        return self.round_of[j * self.move_stride:j * self.move_stride + n]


def solve_host_rounds(fb: FlatBatch, caps, select=None, round_stride: int = 0, move_stride: int = 0, cells16: bool = False,
                      ctx: Optional[DeviceContext] = None, fill: int = 0):
    """kas_solve_host_rounds / kas_solve_host16_rounds: every scenario is solved and reports its records; no rows come back, but
    the packed rounds of the scenarios in `select` (None: every scenario) under `caps` (abi.round_spec: a dict with inbound,
    outbound).  round_stride / move_stride: room for round records / for round_of entries per listed scenario (0: none).
    fill: the int32 word the output arrays hold before the call (tests: what the call does not write stays).  Returns
    (HostOutputs without rows, RoundList)."""
    from .flatten import host_tables16, to_cells16
    L = load()
    ctx = ctx or default_context()
    bd = batch_desc(fb)
    if cells16:
        bd.node_id = None
        cur16 = to_cells16(fb)                 # (held until the call returns: the table only borrows it)
        t, ho = host_tables16(fb, cur16, out_len=0)
    else:
        t, ho = host_tables(fb, out_len=0)
    t.out = None
    sel = None if select is None else np.ascontiguousarray(select, dtype=np.int32)
    listed = np.arange(fb.n_scenarios, dtype=np.int32) if sel is None else sel
    n, rs, ms = int(listed.size), int(round_stride), int(move_stride)
    spec = abi.round_spec(caps)
    scen = np.full(max(n, 1), fill, abi.SCENARIO_ROUNDS_DTYPE)[:n]
    recs = np.full(max(n * max(rs, 0), 1), fill, abi.MOVE_ROUND_DTYPE)[:n * max(rs, 0)]
    rof = np.full(max(n * max(ms, 0), 1), fill, np.int32)[:n * max(ms, 0)]
    o = abi.Rounds(scen.ctypes.data if n else None, recs.ctypes.data if recs.size else None, rs, rof.ctypes.data if rof.size else None, ms)
    fn = L.kas_solve_host16_rounds if cells16 else L.kas_solve_host_rounds
    _check(fn(ctx._h, C.byref(bd), C.byref(t), None if sel is None or sel.size == 0 else sel.ctypes.data_as(C.POINTER(C.c_int32)),
              -1 if sel is None else n, C.byref(spec), C.byref(o)))
    return ho, RoundList(spec=spec, select=listed, scenarios=scen, rounds=recs, round_stride=rs, round_of=rof, move_stride=ms)


def solve_host_choose_moves(fb: FlatBatch, keys, k: int, mask=("replicas",), rows: bool = True, cells16: bool = False,
                            moves_cap: Optional[int] = None, cells_cap: Optional[int] = None, ctx: Optional[DeviceContext] = None):
    """kas_solve_host_choose_moves / 16: solve_host_choose plus the moves of the chosen, in rank order; rows=False hands the
    library no rows array (rows == NULL, rows_cap == 0): nothing but records, node blocks and moves comes back.
    Returns (HostOutputs without rows, Choice, MoveList)."""
    from .flatten import host_tables16, to_cells16
    L = load()
    ctx = ctx or default_context()
    spec = abi.choose_spec(keys, k)
    bd = batch_desc(fb)
    if cells16:
        bd.node_id = None
        cur16 = to_cells16(fb)                 # (held until the call returns: the table only borrows it)
        t, ho = host_tables16(fb, cur16, out_len=0)
    else:
        t, ho = host_tables(fb, out_len=0)
    t.out = None
    S, kk = fb.n_scenarios, max(int(k), 0)
    rows_cap = int(np.sort(packed_cells(fb))[::-1][:kk].sum()) if rows else 0
    nodes_cap = int(np.sort(np.clip(fb.scen["n_nodes"], 0, None).astype(np.int64))[::-1][:kk].sum())
    c = Choice(rank=np.full(max(S, 1), -9, np.int32)[:S], chosen=np.full(max(kk, 1), -9, np.int32)[:kk],
               row_off=np.full(kk + 1, -9, np.int64), node_off=np.full(kk + 1, -9, np.int64), n_ok=-9,
               rows=np.zeros(max(rows_cap, 1), np.uint16 if cells16 else np.int32)[:rows_cap],
               nodes=np.zeros(max(nodes_cap, 1), abi.NODE_IMPACT_DTYPE)[:nodes_cap],
               scenarios=np.zeros(max(S, 1), abi.SCENARIO_IMPACT_DTYPE)[:S])
    n_ok = np.full(1, -9, np.int32)

    def p(a):
        return a.ctypes.data if a.size else None
    ch = abi.Choice(p(c.rank), p(c.chosen), p(c.row_off), p(c.node_off), p(n_ok), p(c.rows), rows_cap, p(c.nodes), nodes_cap)
    imp = abi.ImpactTables(None, p(c.scenarios))
    room_rows = int(np.sort(scenario_rows(fb))[::-1][:kk].sum())
    room_cells = int(np.sort(packed_cells(fb))[::-1][:kk].sum())
    ml, mv = _move_arrays(mask, kk, room_rows if moves_cap is None else int(moves_cap), room_cells if cells_cap is None else int(cells_cap),
                          cells16)
    fn = L.kas_solve_host16_choose_moves if cells16 else L.kas_solve_host_choose_moves
    _check(fn(ctx._h, C.byref(bd), C.byref(t), C.byref(spec), C.byref(ch), C.byref(imp), C.byref(mv)))
    c.n_ok = int(n_ok[0])
    c.rows = c.rows[:int(c.row_off[kk])] if rows else c.rows[:0]
    c.nodes = c.nodes[:int(c.node_off[kk])]
    ml.select = c.chosen
    return ho, c, _trim(ml)


def front_rank_device(scenario_results: int, scenario_impact: int, n_scenarios: int, spec, rank: int, chosen: int, counts: int,
                      scratch: int, stream: int = 0, ctx: Optional[DeviceContext] = None):
    """kas_front_rank_device: mark and rank the Pareto front of n_scenarios records on the device under `spec` (abi.front_spec).
    Raw device pointers (int): the two record arrays in, rank int32 [S], chosen int32 [k] and counts int32 [4] out, scratch
    int32 [S].  Asynchronous on `stream`."""
    ctx = ctx or default_context()
    _check(load().kas_front_rank_device(ctx._h, scenario_results or None, scenario_impact or None, int(n_scenarios), C.byref(spec),
                                        rank or None, chosen or None, counts or None, scratch or None,
                                        C.c_void_p(stream) if stream else None))


@dataclass
class Front(Choice):
    """What kas_solve_host_front leaves: a Choice whose rank holds a member's rank or a class code (abi.KAS_FRONT_*), plus the
    counts; n_front > len(chosen) when k cut the list."""
    n_eligible: int = 0
    n_front: int = 0


def solve_host_front(fb: FlatBatch, spec, mask=None, rows: bool = True, cells16: bool = False, moves_cap: Optional[int] = None,
                     cells_cap: Optional[int] = None, ctx: Optional[DeviceContext] = None):
    """kas_solve_host_front / 16: solve_host_choose_moves with the Pareto front under `spec` (abi.front_spec) in place of the
    ranking.  mask=None asks for no moves; rows=False hands the library no rows array.
    Returns (HostOutputs without rows, Front, MoveList or None)."""
    from .flatten import host_tables16, to_cells16
    L = load()
    ctx = ctx or default_context()
    bd = batch_desc(fb)
    if cells16:
        bd.node_id = None
        cur16 = to_cells16(fb)                 # (held until the call returns: the table only borrows it)
        t, ho = host_tables16(fb, cur16, out_len=0)
    else:
        t, ho = host_tables(fb, out_len=0)
    t.out = None
    S, kk = fb.n_scenarios, max(int(spec.k), 0)
    rows_cap = int(np.sort(packed_cells(fb))[::-1][:kk].sum()) if rows else 0
    nodes_cap = int(np.sort(np.clip(fb.scen["n_nodes"], 0, None).astype(np.int64))[::-1][:kk].sum())
    c = Front(rank=np.full(max(S, 1), -9, np.int32)[:S], chosen=np.full(max(kk, 1), -9, np.int32)[:kk],
              row_off=np.full(kk + 1, -9, np.int64), node_off=np.full(kk + 1, -9, np.int64), n_ok=-9,
              rows=np.zeros(max(rows_cap, 1), np.uint16 if cells16 else np.int32)[:rows_cap],
              nodes=np.zeros(max(nodes_cap, 1), abi.NODE_IMPACT_DTYPE)[:nodes_cap],
              scenarios=np.zeros(max(S, 1), abi.SCENARIO_IMPACT_DTYPE)[:S])
    n_ok = np.full(1, -9, np.int32)
    counts = np.full(4, -9, np.int32)

    def p(a):
        return a.ctypes.data if a.size else None
    ch = abi.Choice(p(c.rank), p(c.chosen), p(c.row_off), p(c.node_off), p(n_ok), p(c.rows), rows_cap, p(c.nodes), nodes_cap)
    imp = abi.ImpactTables(None, p(c.scenarios))
    ml = mv = None
    if mask is not None:
        room_rows = int(np.sort(scenario_rows(fb))[::-1][:kk].sum())
        room_cells = int(np.sort(packed_cells(fb))[::-1][:kk].sum())
        ml, mv = _move_arrays(mask, kk, room_rows if moves_cap is None else int(moves_cap),
                              room_cells if cells_cap is None else int(cells_cap), cells16)
    fn = L.kas_solve_host16_front if cells16 else L.kas_solve_host_front
    _check(fn(ctx._h, C.byref(bd), C.byref(t), C.byref(spec), C.byref(ch), counts.ctypes.data, C.byref(imp),
              C.byref(mv) if mv is not None else None))
    c.n_ok, c.n_eligible, c.n_front = int(n_ok[0]), int(counts[1]), int(counts[2])
    assert int(counts[0]) == c.n_ok and int(counts[3]) == 0
    c.rows = c.rows[:int(c.row_off[kk])] if rows else c.rows[:0]
    c.nodes = c.nodes[:int(c.node_off[kk])]
    if ml is not None:
        ml.select = c.chosen
        ml = _trim(ml)
    return ho, c, ml


def rank_device_racks(scenario_results: int, scenario_impact: int, rack_scenarios: int, n_scenarios: int, keys, k: int, rank: int,
                      chosen: int, n_ok: int, stream: int = 0, ctx: Optional[DeviceContext] = None):
    """kas_rank_device_racks: rank_device with the scenario rack records (a raw device pointer, or 0) as a third source of
    criteria; `keys`: names of abi.KEY_NAMES and abi.RACK_KEY_NAMES."""
    ctx = ctx or default_context()
    spec = abi.rack_choose_spec(keys, k)
    _check(load().kas_rank_device_racks(ctx._h, scenario_results or None, scenario_impact or None, rack_scenarios or None, int(n_scenarios),
                                        C.byref(spec), rank or None, chosen or None, n_ok or None, C.c_void_p(stream) if stream else None))


def front_rank_device_racks(scenario_results: int, scenario_impact: int, rack_scenarios: int, n_scenarios: int, spec, rank: int,
                            chosen: int, counts: int, scratch: int, stream: int = 0, ctx: Optional[DeviceContext] = None):
    """kas_front_rank_device_racks: front_rank_device with the scenario rack records; `spec`: abi.rack_front_spec."""
    ctx = ctx or default_context()
    _check(load().kas_front_rank_device_racks(ctx._h, scenario_results or None, scenario_impact or None, rack_scenarios or None,
                                              int(n_scenarios), C.byref(spec), rank or None, chosen or None, counts or None,
                                              scratch or None, C.c_void_p(stream) if stream else None))


def _rack_arrays(fb: FlatBatch, report_rack, racks_cap):
    """(report table or None, RackReport with zeroed arrays, abi.RackTables) for a call with the rack pass"""
    rep = None if report_rack is None else np.ascontiguousarray(report_rack, dtype=np.int32)
    S = fb.n_scenarios
    cap = max(int(rack_counts(fb, rep).sum()), 0) if racks_cap is None else int(racks_cap)
    rr = RackReport(racks=np.zeros(max(cap, 1), dtype=abi.RACK_IMPACT_DTYPE), scenarios=np.zeros(max(S, 1), dtype=abi.SCENARIO_RACK_IMPACT_DTYPE),
                    rack_off=np.zeros(S + 1, dtype=np.int64))
    return rep, rr, abi.RackTables(rr.racks.ctypes.data, rr.scenarios.ctypes.data, rr.rack_off.ctypes.data, cap)


def _choice_records(fb, spec, front, report_rack, mask, rows, cells16, moves_cap, cells_cap, racks_cap, ctx, racks=True, topics=False):
    """the shared body of solve_host_choose_racks / solve_host_front_racks and, with topics=True, of solve_host_choose_topics /
    solve_host_front_topics (the *_topics entries; host_racks == NULL when racks=False).  Always five results: (HostOutputs, Choice or
    Front, MoveList or None, RackReport or None, TopicReport or None)"""
    from .flatten import host_tables16, to_cells16
    L = load()
    ctx = ctx or default_context()
    bd = batch_desc(fb)
    if cells16:
        bd.node_id = None
        cur16 = to_cells16(fb)                 # (held until the call returns: the table only borrows it)
        t, ho = host_tables16(fb, cur16, out_len=0)
    else:
        t, ho = host_tables(fb, out_len=0)
    t.out = None
    S, kk = fb.n_scenarios, max(int(spec.k), 0)
    rows_cap = int(np.sort(packed_cells(fb))[::-1][:kk].sum()) if rows else 0
    nodes_cap = int(np.sort(np.clip(fb.scen["n_nodes"], 0, None).astype(np.int64))[::-1][:kk].sum())
    c = (Front if front else Choice)(rank=np.full(max(S, 1), -9, np.int32)[:S], chosen=np.full(max(kk, 1), -9, np.int32)[:kk],
                                     row_off=np.full(kk + 1, -9, np.int64), node_off=np.full(kk + 1, -9, np.int64), n_ok=-9,
                                     rows=np.zeros(max(rows_cap, 1), np.uint16 if cells16 else np.int32)[:rows_cap],
                                     nodes=np.zeros(max(nodes_cap, 1), abi.NODE_IMPACT_DTYPE)[:nodes_cap],
                                     scenarios=np.zeros(max(S, 1), abi.SCENARIO_IMPACT_DTYPE)[:S])
    n_ok = np.full(1, -9, np.int32)
    counts = np.full(4, -9, np.int32)

    def p(a):
        return a.ctypes.data if a.size else None
    ch = abi.Choice(p(c.rank), p(c.chosen), p(c.row_off), p(c.node_off), p(n_ok), p(c.rows), rows_cap, p(c.nodes), nodes_cap)
    imp = abi.ImpactTables(None, p(c.scenarios))
    ml = mv = None
    if mask is not None:
        room_rows = int(np.sort(scenario_rows(fb))[::-1][:kk].sum())
        room_cells = int(np.sort(packed_cells(fb))[::-1][:kk].sum())
        ml, mv = _move_arrays(mask, kk, room_rows if moves_cap is None else int(moves_cap),
                              room_cells if cells_cap is None else int(cells_cap), cells16)
    rep, rr, rk = _rack_arrays(fb, report_rack, racks_cap) if racks else (None, None, None)
    tail = (C.byref(imp), C.byref(mv) if mv is not None else None, None if rep is None else C.c_void_p(rep.ctypes.data),
            C.byref(rk) if racks else None)
    tr = None
    if topics:
        tt, tscen = topic_impact_arrays(fb)
        tp = abi.TopicImpactTables(tt.ctypes.data if tt.size else None, tscen.ctypes.data if tscen.size else None)
        tr = TopicReport(topics=tt, scenarios=tscen, impact=c.scenarios)
        tail += (C.byref(tp),)
    if front:
        fn = getattr(L, "kas_solve_host%s_front_%s" % ("16" if cells16 else "", "topics" if topics else "racks"))
        _check(fn(ctx._h, C.byref(bd), C.byref(t), C.byref(spec), C.byref(ch), counts.ctypes.data, *tail))
        c.n_eligible, c.n_front = int(counts[1]), int(counts[2])
        assert int(counts[0]) == int(n_ok[0]) and int(counts[3]) == 0
    else:
        fn = getattr(L, "kas_solve_host%s_choose_%s" % ("16" if cells16 else "", "topics" if topics else "racks"))
        _check(fn(ctx._h, C.byref(bd), C.byref(t), C.byref(spec), C.byref(ch), *tail))
    c.n_ok = int(n_ok[0])
    c.rows = c.rows[:int(c.row_off[kk])] if rows else c.rows[:0]
    c.nodes = c.nodes[:int(c.node_off[kk])]
    if ml is not None:
        ml.select = c.chosen
        ml = _trim(ml)
    if racks:
        rr.racks, rr.scenarios, rr.impact = rr.racks[:int(rr.rack_off[S])], rr.scenarios[:S], c.scenarios
    return ho, c, ml, rr, tr


def solve_host_choose_racks(fb: FlatBatch, keys, k: int, report_rack=None, mask=None, rows: bool = True, cells16: bool = False,
                            moves_cap: Optional[int] = None, cells_cap: Optional[int] = None, racks_cap: Optional[int] = None,
                            ctx: Optional[DeviceContext] = None):
    """kas_solve_host_choose_racks / 16: solve_host_choose_moves plus the rack pass against `report_rack` (None: the batch's own
    racks); `keys` may name rack criteria (abi.RACK_KEY_NAMES) beside abi.KEY_NAMES.  mask=None asks for no moves; rows=False
    hands the library no rows array.  Rows, node blocks and moves come back for the chosen, the rack records for every scenario.
    Returns (HostOutputs without rows, Choice, MoveList or None, RackReport without node records)."""
    return _choice_records(fb, abi.rack_choose_spec(keys, k), False, report_rack, mask, rows, cells16, moves_cap, cells_cap, racks_cap, ctx)[:4]


def solve_host_front_racks(fb: FlatBatch, spec, report_rack=None, mask=None, rows: bool = True, cells16: bool = False,
                           moves_cap: Optional[int] = None, cells_cap: Optional[int] = None, racks_cap: Optional[int] = None,
                           ctx: Optional[DeviceContext] = None):
    """kas_solve_host_front_racks / 16: solve_host_front plus the rack pass; `spec` (abi.rack_front_spec) may name rack criteria
    among its criteria and its bounds.  Returns (HostOutputs without rows, Front, MoveList or None, RackReport)."""
    return _choice_records(fb, spec, True, report_rack, mask, rows, cells16, moves_cap, cells_cap, racks_cap, ctx)[:4]


def rank_device_topics(scenario_results: int, scenario_impact: int, rack_scenarios: int, topic_scenarios: int, n_scenarios: int, keys,
                       k: int, rank: int, chosen: int, n_ok: int, stream: int = 0, ctx: Optional[DeviceContext] = None):
    """kas_rank_device_topics: rank_device_racks with the scenario topic records (a raw device pointer, or 0) as a further source
    of criteria; `keys`: names of abi.KEY_NAMES, abi.RACK_KEY_NAMES and abi.TOPIC_KEY_NAMES."""
    ctx = ctx or default_context()
    spec = abi.topic_choose_spec(keys, k)
    _check(load().kas_rank_device_topics(ctx._h, scenario_results or None, scenario_impact or None, rack_scenarios or None,
                                         topic_scenarios or None, int(n_scenarios), C.byref(spec), rank or None, chosen or None,
                                         n_ok or None, C.c_void_p(stream) if stream else None))


def front_rank_device_topics(scenario_results: int, scenario_impact: int, rack_scenarios: int, topic_scenarios: int, n_scenarios: int,
                             spec, rank: int, chosen: int, counts: int, scratch: int, stream: int = 0,
                             ctx: Optional[DeviceContext] = None):
    """kas_front_rank_device_topics: front_rank_device_racks with the scenario topic records; `spec`: abi.topic_front_spec."""
    ctx = ctx or default_context()
    _check(load().kas_front_rank_device_topics(ctx._h, scenario_results or None, scenario_impact or None, rack_scenarios or None,
                                               topic_scenarios or None, int(n_scenarios), C.byref(spec), rank or None, chosen or None,
                                               counts or None, scratch or None, C.c_void_p(stream) if stream else None))


def solve_host_choose_topics(fb: FlatBatch, keys, k: int, racks: bool = False, report_rack=None, mask=None, rows: bool = True,
                             cells16: bool = False, moves_cap: Optional[int] = None, cells_cap: Optional[int] = None,
                             racks_cap: Optional[int] = None, ctx: Optional[DeviceContext] = None):
    """kas_solve_host_choose_topics / 16: solve_host_choose_racks plus the topic pass; `keys` may name topic criteria
    (abi.TOPIC_KEY_NAMES) beside abi.KEY_NAMES and, with racks=True (the rack pass, against `report_rack`), abi.RACK_KEY_NAMES.
    racks=False hands the library no rack tables (host_racks == NULL).  Every scenario's topic records come back.
    Returns (HostOutputs without rows, Choice, MoveList or None, RackReport or None, TopicReport)."""
    return _choice_records(fb, abi.topic_choose_spec(keys, k), False, report_rack, mask, rows, cells16, moves_cap, cells_cap, racks_cap, ctx,
                         racks=racks, topics=True)


def solve_host_front_topics(fb: FlatBatch, spec, racks: bool = False, report_rack=None, mask=None, rows: bool = True,
                            cells16: bool = False, moves_cap: Optional[int] = None, cells_cap: Optional[int] = None,
                            racks_cap: Optional[int] = None, ctx: Optional[DeviceContext] = None):
    """kas_solve_host_front_topics / 16: solve_host_front_racks plus the topic pass; `spec` (abi.topic_front_spec) may name topic
    criteria among its criteria and its bounds.  Returns (HostOutputs without rows, Front, MoveList or None, RackReport or None,
    TopicReport)."""
    return _choice_records(fb, spec, True, report_rack, mask, rows, cells16, moves_cap, cells_cap, racks_cap, ctx, racks=racks, topics=True)


def solve_host_sharded(fb: FlatBatch, ctxs) -> HostOutputs:
    """kas_solve_host_sharded: contiguous scenario ranges over several contexts (devices), one host
    thread each; the caller's host arrays are the gather."""
    L = load()
    bd = batch_desc(fb)
    t, ho = host_tables(fb)
    arr = (C.c_void_p * len(ctxs))(*[c._h for c in ctxs])
    _check(L.kas_solve_host_sharded(arr, len(ctxs), C.byref(bd), C.byref(t)))
    return ho


class PinnedArray:
    """int32 (or uint16: 16-bit cells) numpy array over kas_host_alloc memory (pinned: kas_solve_host moves it by DMA
    without staging)."""

    def __init__(self, n: int, dtype=np.int32):
        self._lib = load()
        self._p = C.c_void_p()
        item = np.dtype(dtype).itemsize
        _check(self._lib.kas_host_alloc(item * max(int(n), 1), C.byref(self._p)))
        buf = (C.c_uint8 * (item * max(int(n), 1))).from_address(self._p.value)
        self.array = np.frombuffer(buf, dtype=dtype)[:int(n)]

    def close(self):
        if self._p:
            self.array = None
            self._lib.kas_host_free(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def shard_range(total: int, rank: int, world: int):
    """kas_shard_range (the C mirror of sharding.shard_range)."""
    lo, hi = C.c_int64(), C.c_int64()
    load().kas_shard_range(total, rank, world, C.byref(lo), C.byref(hi))
    return lo.value, hi.value


def solve_host_with_flags(fb: FlatBatch, flags: int, ctx: Optional[DeviceContext] = None) -> HostOutputs:
    """Same as solve_host but through plan + device tables so plan flags can be set."""
    import torch
    ctx = ctx or default_context()
    dev = torch.device("cuda", ctx.device)
    plan = Plan(ctx, fb)
    plan.set_flags(flags)
    _, ho = host_tables(fb)
    d_cur = torch.from_numpy(fb.cur).to(dev)
    d_aux = torch.from_numpy(fb.aux).to(dev) if fb.aux.size else None
    d_ctx = torch.from_numpy(ho.ctx).to(dev) if ho.ctx.size else None
    d_out = torch.full((max(fb.out_len, 1),), -2, dtype=torch.int32, device=dev)
    d_tr = torch.zeros(max(fb.n_topics, 1) * 16, dtype=torch.uint8, device=dev)
    d_sr = torch.zeros(max(fb.n_scenarios, 1) * 32, dtype=torch.uint8, device=dev)
    st = torch.cuda.Stream(dev)
    st.wait_stream(torch.cuda.current_stream(dev))
    plan.solve_device(d_cur.data_ptr(), d_out.data_ptr(), d_tr.data_ptr(), d_sr.data_ptr(),
                      aux=d_aux.data_ptr() if d_aux is not None else 0,
                      ctx=d_ctx.data_ptr() if d_ctx is not None else 0, stream=st.cuda_stream)
    st.synchronize()
    ho.out = d_out.cpu().numpy()
    ho.topic_results = d_tr.cpu().numpy().view(abi.TOPIC_RESULT_DTYPE)
    ho.scenario_results = d_sr.cpu().numpy().view(abi.SCENARIO_RESULT_DTYPE)
    if d_ctx is not None:
        ho.ctx = d_ctx.cpu().numpy()
    plan.close()
    return ho


def solve_device16_with_flags(fb: FlatBatch, flags: int = 0, ctx: Optional[DeviceContext] = None, cur16=None) -> HostOutputs:
    """kas_plan_create16 + kas_solve_device16: the batch solved on uint16 node-index cells resident in HBM (HostOutputs.out is
    the uint16 out pool).  Raises KasError(KAS_E_UNSUPPORTED) for batches the 16-bit kernels do not take."""
    import torch
    from .flatten import to_cells16
    ctx = ctx or default_context()
    dev = torch.device("cuda", ctx.device)
    plan = Plan(ctx, fb, cells16=True)
    try:
        if flags:
            plan.set_flags(flags)
        _, ho = host_tables(fb)
        c16 = to_cells16(fb) if cur16 is None else cur16
        d_cur = torch.from_numpy(c16.view(np.int16)).to(dev)
        d_aux = torch.from_numpy(fb.aux).to(dev) if fb.aux.size else None
        d_ctx = torch.from_numpy(ho.ctx).to(dev) if ho.ctx.size else None
        d_out = torch.full((max(fb.out_len, 1),), -2, dtype=torch.int16, device=dev)
        d_tr = torch.zeros(max(fb.n_topics, 1) * 16, dtype=torch.uint8, device=dev)
        d_sr = torch.zeros(max(fb.n_scenarios, 1) * 32, dtype=torch.uint8, device=dev)
        st = torch.cuda.Stream(dev)
        st.wait_stream(torch.cuda.current_stream(dev))
        plan.solve_device(d_cur.data_ptr(), d_out.data_ptr(), d_tr.data_ptr(), d_sr.data_ptr(),
                          aux=d_aux.data_ptr() if d_aux is not None else 0,
                          ctx=d_ctx.data_ptr() if d_ctx is not None else 0, stream=st.cuda_stream)
        st.synchronize()
        ho.out = d_out.cpu().numpy().view(np.uint16)
        ho.topic_results = d_tr.cpu().numpy().view(abi.TOPIC_RESULT_DTYPE)
        ho.scenario_results = d_sr.cpu().numpy().view(abi.SCENARIO_RESULT_DTYPE)
        if d_ctx is not None:
            ho.ctx = d_ctx.cpu().numpy()
        ho.describe = plan.describe()
    finally:
        plan.close()
    return ho

"""ctypes mirror of include/kas_abi.h (structs, constants, digest function).

Pure declarations: nothing here loads a library.  Field order and types must match the header
byte for byte; tests/test_abi_layout.py checks sizes and offsets against a C probe.
"""
from __future__ import annotations

import ctypes as C

KAS_ABI_VERSION = 6
KAS_MAX_WIDTH = 8
KAS_CELL16_NONE = 0xFFFF      # 16-bit cells (kas_solve_host16): no such broker in cur, pad in out

KAS_E_OK = 0
KAS_E_INVALID_ARG = -1
KAS_E_HIP = -2
KAS_E_UNSUPPORTED = -3
KAS_E_NOMEM = -4

KAS_OK = 0
KAS_FAIL_UNASSIGNABLE = 1
KAS_FAIL_RF_NOT_POSITIVE = 2
KAS_FAIL_RF_GT_BROKERS = 3
KAS_FAIL_HASH_INDEX = 4
KAS_FAIL_RF_MISMATCH = 5
KAS_SKIPPED = 6
KAS_FAIL_BAD_NODES = 7
KAS_FAIL_WATCHDOG = 8

# plan flags (kas_plan_set_flags; include/kas_abi.h)
KAS_PLAN_GENERIC_FILL = 1
KAS_PLAN_ROUND_ORDER = 2
KAS_PLAN_WIDE_COUNTERS = 4
KAS_PLAN_TWO_PASS_HIST = 8
KAS_PLAN_SPREAD_FILL = 32
KAS_PLAN_FULL_FILL = 16
KAS_PLAN_NO_INDEX_ROWS = 64
KAS_PLAN_INDEX_ROWS = 128
KAS_PLAN_MID32 = 0x80000
KAS_PLAN_NO_MID32 = 0x100000
KAS_PLAN_TICKET_ORDER = 0x10000
KAS_PLAN_RELAX_TILES_64 = 0x20000     # KAS_PLAN_RELAX_TILES(1)
KAS_PLAN_RELAX_TILES_128 = 0x40000    # KAS_PLAN_RELAX_TILES(2)
KAS_PLAN_NO_RTN_QUOTA = 0x200000
KAS_PLAN_SPLIT_P4 = 0x400000          # first fit in kas_p4_kernel whatever the batch size (default: from 512 scenarios on)
KAS_PLAN_FILL_WITH_P4 = 0x800000      # first fit inside the fill workgroup whatever the batch size
KAS_PLAN_P4_WITH_ORDER = 0xC00000     # both: first fit as a second wavefront of the order kernel's workgroup (kas_p4_order_kernel)


def KAS_PLAN_VERIFY_SAMPLE(k: int) -> int:
    """relaxation form: k tiles per topic evaluated a second time row by row (include/kas_abi.h)"""
    return (k & 0xff) << 24

STATUS_NAMES = {
    KAS_OK: "OK",
    KAS_FAIL_UNASSIGNABLE: "FAIL_UNASSIGNABLE",
    KAS_FAIL_RF_NOT_POSITIVE: "FAIL_RF_NOT_POSITIVE",
    KAS_FAIL_RF_GT_BROKERS: "FAIL_RF_GT_BROKERS",
    KAS_FAIL_HASH_INDEX: "FAIL_HASH_INDEX",
    KAS_FAIL_RF_MISMATCH: "FAIL_RF_MISMATCH",
    KAS_SKIPPED: "SKIPPED",
    KAS_FAIL_BAD_NODES: "FAIL_BAD_NODES",
    KAS_FAIL_WATCHDOG: "FAIL_WATCHDOG",
}


class TopicDesc(C.Structure):
    _fields_ = [
        ("name_hash", C.c_int32),
        ("n_partitions", C.c_int32),
        ("cur_width", C.c_int32),
        ("rf", C.c_int32),
        ("out_width", C.c_int32),
        ("reserved", C.c_int32),
        ("cur_off", C.c_int64),
        ("out_off", C.c_int64),
        ("cur_len_off", C.c_int64),
        ("in_partitions_off", C.c_int64),
        ("part_id_off", C.c_int64),
    ]


class ScenarioDesc(C.Structure):
    _fields_ = [
        ("n_nodes", C.c_int32),
        ("topic_begin", C.c_int32),
        ("topic_count", C.c_int32),
        ("ctx_width", C.c_int32),
        ("node_off", C.c_int64),
        ("ctx_off", C.c_int64),
    ]


class TopicResult(C.Structure):
    _fields_ = [
        ("status", C.c_int32),
        ("fail_partition", C.c_int32),
        ("moved_replicas", C.c_int32),
        ("moved_partitions", C.c_int32),
    ]


class ScenarioResult(C.Structure):
    _fields_ = [
        ("status", C.c_int32),
        ("fail_topic", C.c_int32),
        ("fail_partition", C.c_int32),
        ("moved_replicas", C.c_int32),
        ("moved_partitions", C.c_int32),
        ("reserved", C.c_int32),
        ("digest", C.c_uint64),
    ]


class BatchDesc(C.Structure):
    _fields_ = [
        ("n_scenarios", C.c_int32),
        ("n_topics", C.c_int32),
        ("scenarios", C.POINTER(ScenarioDesc)),
        ("topics", C.POINTER(TopicDesc)),
        ("node_id", C.POINTER(C.c_int32)),
        ("node_rack", C.POINTER(C.c_int32)),
        ("node_pool_len", C.c_int64),
    ]


class Tables(C.Structure):
    _fields_ = [
        ("cur", C.c_void_p),
        ("out", C.c_void_p),
        ("aux", C.c_void_p),
        ("ctx", C.c_void_p),
        ("topic_results", C.c_void_p),
        ("scenario_results", C.c_void_p),
        ("cur_len", C.c_int64),
        ("out_len", C.c_int64),
        ("aux_len", C.c_int64),
        ("ctx_len", C.c_int64),
    ]


class RfResult(C.Structure):
    """kas_rf_result: what kas_resolve_replication_factor leaves (KTA:47-69 as data)."""
    _fields_ = [("status", C.c_int32), ("rf", C.c_int32), ("fail_partition", C.c_int32), ("fail_list_size", C.c_int32)]


# numpy structured dtypes with the same layout as TopicResult / ScenarioResult
import numpy as _np  # noqa: E402

TOPIC_RESULT_DTYPE = _np.dtype([
    ("status", "<i4"), ("fail_partition", "<i4"),
    ("moved_replicas", "<i4"), ("moved_partitions", "<i4")])
SCENARIO_RESULT_DTYPE = _np.dtype([
    ("status", "<i4"), ("fail_topic", "<i4"), ("fail_partition", "<i4"),
    ("moved_replicas", "<i4"), ("moved_partitions", "<i4"), ("reserved", "<i4"),
    ("digest", "<u8")])
TOPIC_DESC_DTYPE = _np.dtype([
    ("name_hash", "<i4"), ("n_partitions", "<i4"), ("cur_width", "<i4"), ("rf", "<i4"),
    ("out_width", "<i4"), ("reserved", "<i4"), ("cur_off", "<i8"), ("out_off", "<i8"),
    ("cur_len_off", "<i8"), ("in_partitions_off", "<i8"), ("part_id_off", "<i8")])
SCENARIO_DESC_DTYPE = _np.dtype([
    ("n_nodes", "<i4"), ("topic_begin", "<i4"), ("topic_count", "<i4"), ("ctx_width", "<i4"),
    ("node_off", "<i8"), ("ctx_off", "<i8")])

# ABI v6: the impact records (kas_node_impact / kas_scenario_impact) and where they go (kas_impact_tables)
NODE_IMPACT_FIELDS = ("replicas_before", "replicas_after", "leaders_before", "leaders_after", "inbound", "outbound")
SCENARIO_IMPACT_FIELDS = ("departed_replicas", "leaders_moved", "max_inbound", "max_outbound",
                          "min_replicas_after", "max_replicas_after", "min_leaders_after", "max_leaders_after")
NODE_IMPACT_DTYPE = _np.dtype([(f, "<i4") for f in NODE_IMPACT_FIELDS] + [("reserved", "<i4", (2,))])
SCENARIO_IMPACT_DTYPE = _np.dtype([(f, "<i4") for f in SCENARIO_IMPACT_FIELDS])


class ImpactTables(C.Structure):
    _fields_ = [("nodes", C.c_void_p), ("scenarios", C.c_void_p)]


# choosing the best scenarios on the device (kas_choose_spec / kas_choice): criterion name -> KAS_KEY_*
KAS_CHOOSE_MAX_KEYS = 4
KEY_NAMES = ("moved_replicas", "moved_partitions", "leaders_moved", "departed_replicas", "max_inbound", "max_outbound",
             "replica_spread", "leader_spread", "max_replicas_after", "max_leaders_after")
KEYS = {name: i for i, name in enumerate(KEY_NAMES)}
(KAS_KEY_MOVED_REPLICAS, KAS_KEY_MOVED_PARTITIONS, KAS_KEY_LEADERS_MOVED, KAS_KEY_DEPARTED_REPLICAS, KAS_KEY_MAX_INBOUND,
 KAS_KEY_MAX_OUTBOUND, KAS_KEY_REPLICA_SPREAD, KAS_KEY_LEADER_SPREAD, KAS_KEY_MAX_REPLICAS_AFTER, KAS_KEY_MAX_LEADERS_AFTER) = range(10)
KAS_KEY_COUNT = 10
CHOOSE_ENTRIES = ("kas_rank_device", "kas_choose_device", "kas_choose_device16", "kas_solve_host_choose", "kas_solve_host16_choose")


class ChooseSpec(C.Structure):
    _fields_ = [("n_keys", C.c_int32), ("key", C.c_int32 * KAS_CHOOSE_MAX_KEYS), ("k", C.c_int32)]


class Choice(C.Structure):
    _fields_ = [("rank", C.c_void_p), ("chosen", C.c_void_p), ("row_off", C.c_void_p), ("node_off", C.c_void_p),
                ("n_ok", C.c_void_p), ("rows", C.c_void_p), ("rows_cap", C.c_int64), ("nodes", C.c_void_p),
                ("nodes_cap", C.c_int64)]


def choose_spec(keys, k: int) -> "ChooseSpec":
    """kas_choose_spec from criterion names (KEY_NAMES) or KAS_KEY_* numbers; unknown names raise ValueError."""
    keys = [keys] if isinstance(keys, (str, int)) else list(keys)
    ids = []
    for name in keys:
        if isinstance(name, str):
            if name not in KEYS:
                raise ValueError("unknown criterion %r (one of %s)" % (name, ", ".join(KEY_NAMES)))
            name = KEYS[name]
        ids.append(int(name))
    spec = ChooseSpec()
    spec.n_keys = len(ids)
    for i, v in enumerate(ids[:KAS_CHOOSE_MAX_KEYS]):
        spec.key[i] = v
    spec.k = int(k)
    return spec


# the Pareto front of the scenarios (kas_front_spec): the criteria traded off, hard bounds, the class codes a non-member's rank holds
KAS_FRONT_NOT_OK, KAS_FRONT_OVER_LIMIT, KAS_FRONT_DOMINATED = -1, -2, -3
FRONT_CLASSES = {0: "member", KAS_FRONT_NOT_OK: "failed", KAS_FRONT_OVER_LIMIT: "over_limit", KAS_FRONT_DOMINATED: "dominated"}
FRONT_ENTRIES = ("kas_front_rank_device", "kas_front_device", "kas_front_device16", "kas_solve_host_front", "kas_solve_host16_front")


class FrontSpec(C.Structure):
    _fields_ = [("n_keys", C.c_int32), ("key", C.c_int32 * KAS_CHOOSE_MAX_KEYS), ("n_limits", C.c_int32),
                ("limit_key", C.c_int32 * KAS_CHOOSE_MAX_KEYS), ("limit", C.c_int32 * KAS_CHOOSE_MAX_KEYS), ("k", C.c_int32)]


def _key_id(name) -> int:
    if isinstance(name, str):
        if name not in KEYS:
            raise ValueError("unknown criterion %r (one of %s)" % (name, ", ".join(KEY_NAMES)))
        return KEYS[name]
    return int(name)


def front_spec(by, within=None, k: int = 0) -> "FrontSpec":
    """kas_front_spec: `by` the criteria traded off (names of KEY_NAMES or KAS_KEY_* numbers), `within` hard bounds as
    {criterion: limit} (or a list of pairs), k members to return; unknown names raise ValueError."""
    ids = [_key_id(n) for n in ([by] if isinstance(by, (str, int)) else list(by))]
    pairs = list(within.items()) if isinstance(within, dict) else list(within or ())
    spec = FrontSpec()
    spec.n_keys = len(ids)
    for i, v in enumerate(ids[:KAS_CHOOSE_MAX_KEYS]):
        spec.key[i] = v
    spec.n_limits = len(pairs)
    for i, (name, limit) in enumerate(pairs[:KAS_CHOOSE_MAX_KEYS]):
        spec.limit_key[i] = _key_id(name)
        spec.limit[i] = int(limit)
    spec.k = int(k)
    return spec


# the rack pass behind the impact pass (kas_rack_impact / kas_scenario_rack_impact) and where its records go (kas_rack_tables)
KAS_RACK_LIMIT = 4096
RACK_IMPACT_FIELDS = ("nodes", "replicas_before", "replicas_after", "leaders_before", "leaders_after", "inbound", "outbound")
SCENARIO_RACK_ROW_FIELDS = ("colocated_before", "colocated_after", "rows_colocated_before", "rows_colocated_after",
                            "single_rack_rows_before", "single_rack_rows_after", "new_rack_replicas", "rows_losing_racks")
SCENARIO_RACK_FIELDS = SCENARIO_RACK_ROW_FIELDS + ("n_racks", "max_rack_inbound", "max_rack_outbound", "min_rack_replicas_after",
                                                   "max_rack_replicas_after", "min_rack_leaders_after", "max_rack_leaders_after")
RACK_IMPACT_DTYPE = _np.dtype([(f, "<i4") for f in RACK_IMPACT_FIELDS] + [("reserved", "<i4")])
SCENARIO_RACK_IMPACT_DTYPE = _np.dtype([(f, "<i4") for f in SCENARIO_RACK_FIELDS] + [("reserved", "<i4")])
RACK_ENTRIES = ("kas_rack_impact_device", "kas_rack_impact_device16", "kas_solve_host_rack_impact", "kas_solve_host16_rack_impact")


class RackTables(C.Structure):
    _fields_ = [("racks", C.c_void_p), ("scenarios", C.c_void_p), ("rack_off", C.c_void_p), ("racks_cap", C.c_int64)]


# the topic pass behind a solve (kas_topic_impact / kas_scenario_topic_impact) and where its records go (kas_topic_impact_tables)
KAS_TOPIC_SCRATCH_LIMIT = 256 << 20
TOPIC_IMPACT_FIELDS = ("departed_replicas", "leaders_moved", "max_inbound", "max_outbound", "min_replicas_after", "max_replicas_after",
                       "min_leaders_after", "max_leaders_after")
SCENARIO_TOPIC_FIELDS = ("topics_ok", "topics_moved", "topics_leaders_moved", "topics_departed", "max_topic_moved_replicas",
                         "max_topic_moved_partitions", "max_topic_leaders_moved", "max_topic_inbound", "max_topic_outbound",
                         "max_topic_replica_spread", "max_topic_leader_spread", "max_topic_replicas_after", "max_topic_leaders_after",
                         "sum_topic_replica_spread", "sum_topic_leader_spread")
TOPIC_IMPACT_DTYPE = _np.dtype([(f, "<i4") for f in TOPIC_IMPACT_FIELDS])
SCENARIO_TOPIC_IMPACT_DTYPE = _np.dtype([(f, "<i4") for f in SCENARIO_TOPIC_FIELDS] + [("reserved", "<i4")])
TOPIC_ENTRIES = ("kas_topic_impact_device", "kas_topic_impact_device16", "kas_solve_host_topic_impact", "kas_solve_host16_topic_impact")


class TopicImpactTables(C.Structure):
    _fields_ = [("topics", C.c_void_p), ("scenarios", C.c_void_p)]


assert TOPIC_IMPACT_DTYPE.itemsize == 32 and SCENARIO_TOPIC_IMPACT_DTYPE.itemsize == 64 and C.sizeof(TopicImpactTables) == 16


# rack criteria of the *_racks entries: key KAS_KEY_RACK_BASE + i is int32 word i of kas_scenario_rack_impact, two spreads behind
KAS_KEY_RACK_BASE = 16
RACK_KEY_NAMES = SCENARIO_RACK_FIELDS + ("rack_replica_spread", "rack_leader_spread")
RACK_KEYS = {name: KAS_KEY_RACK_BASE + i for i, name in enumerate(RACK_KEY_NAMES)}
KAS_KEY_RACK_REPLICA_SPREAD, KAS_KEY_RACK_LEADER_SPREAD = RACK_KEYS["rack_replica_spread"], RACK_KEYS["rack_leader_spread"]
KAS_KEY_RACK_END = KAS_KEY_RACK_BASE + len(RACK_KEY_NAMES)
RACK_CHOOSE_ENTRIES = ("kas_rank_device_racks", "kas_front_rank_device_racks", "kas_choose_device_racks", "kas_choose_device16_racks",
                       "kas_front_device_racks", "kas_front_device16_racks", "kas_solve_host_choose_racks",
                       "kas_solve_host16_choose_racks", "kas_solve_host_front_racks", "kas_solve_host16_front_racks")
assert KAS_KEY_RACK_END == 33 and not set(KEYS) & set(RACK_KEYS)


def is_rack_key(name) -> bool:
    """is `name` (a criterion name or a KAS_KEY_* number) a rack criterion"""
    return name in RACK_KEYS if isinstance(name, str) else KAS_KEY_RACK_BASE <= int(name) < KAS_KEY_RACK_END


def rack_key_id(name) -> int:
    """KAS_KEY_* of a criterion name of either set (KEY_NAMES, RACK_KEY_NAMES), or the number itself; unknown names raise
    ValueError listing both sets."""
    if isinstance(name, str):
        if name in KEYS:
            return KEYS[name]
        if name in RACK_KEYS:
            return RACK_KEYS[name]
        raise ValueError("unknown criterion %r (one of %s; rack criteria: %s)" % (name, ", ".join(KEY_NAMES), ", ".join(RACK_KEY_NAMES)))
    return int(name)


def rack_choose_spec(keys, k: int) -> "ChooseSpec":
    """kas_choose_spec for the *_racks entries: names of KEY_NAMES and RACK_KEY_NAMES (or KAS_KEY_* numbers), in any mix."""
    ids = [rack_key_id(n) for n in ([keys] if isinstance(keys, (str, int)) else list(keys))]
    spec = ChooseSpec()
    spec.n_keys = len(ids)
    for i, v in enumerate(ids[:KAS_CHOOSE_MAX_KEYS]):
        spec.key[i] = v
    spec.k = int(k)
    return spec


def rack_front_spec(by, within=None, k: int = 0) -> "FrontSpec":
    """kas_front_spec for the *_racks entries: front_spec with both name sets, among the criteria and among the bounds."""
    ids = [rack_key_id(n) for n in ([by] if isinstance(by, (str, int)) else list(by))]
    pairs = list(within.items()) if isinstance(within, dict) else list(within or ())
    spec = FrontSpec()
    spec.n_keys = len(ids)
    for i, v in enumerate(ids[:KAS_CHOOSE_MAX_KEYS]):
        spec.key[i] = v
    spec.n_limits = len(pairs)
    for i, (name, limit) in enumerate(pairs[:KAS_CHOOSE_MAX_KEYS]):
        spec.limit_key[i] = rack_key_id(name)
        spec.limit[i] = int(limit)
    spec.k = int(k)
    return spec


# topic criteria of the *_topics entries: key KAS_KEY_TOPIC_BASE + i is int32 word i of kas_scenario_topic_impact (no derived keys)
KAS_KEY_TOPIC_BASE = 48
TOPIC_KEY_NAMES = SCENARIO_TOPIC_FIELDS
TOPIC_KEYS = {name: KAS_KEY_TOPIC_BASE + i for i, name in enumerate(TOPIC_KEY_NAMES)}
KAS_KEY_TOPIC_END = KAS_KEY_TOPIC_BASE + len(TOPIC_KEY_NAMES)
TOPIC_CHOOSE_ENTRIES = ("kas_rank_device_topics", "kas_front_rank_device_topics", "kas_choose_device_topics", "kas_choose_device16_topics",
                        "kas_front_device_topics", "kas_front_device16_topics", "kas_solve_host_choose_topics",
                        "kas_solve_host16_choose_topics", "kas_solve_host_front_topics", "kas_solve_host16_front_topics")
assert KAS_KEY_TOPIC_END == 63 and not (set(KEYS) | set(RACK_KEYS)) & set(TOPIC_KEYS)


def is_topic_key(name) -> bool:
    """is `name` (a criterion name or a KAS_KEY_* number) a topic criterion"""
    return name in TOPIC_KEYS if isinstance(name, str) else KAS_KEY_TOPIC_BASE <= int(name) < KAS_KEY_TOPIC_END


def topic_key_id(name) -> int:
    """KAS_KEY_* of a criterion name of any of the three sets (KEY_NAMES, RACK_KEY_NAMES, TOPIC_KEY_NAMES), or the number itself;
    unknown names raise ValueError listing the three sets."""
    if isinstance(name, str):
        for keys in (KEYS, RACK_KEYS, TOPIC_KEYS):
            if name in keys:
                return keys[name]
        raise ValueError("unknown criterion %r (one of %s; rack criteria: %s; topic criteria: %s)" %
                         (name, ", ".join(KEY_NAMES), ", ".join(RACK_KEY_NAMES), ", ".join(TOPIC_KEY_NAMES)))
    return int(name)


def topic_choose_spec(keys, k: int) -> "ChooseSpec":
    """kas_choose_spec for the *_topics entries: names of the three sets (or KAS_KEY_* numbers), in any mix."""
    ids = [topic_key_id(n) for n in ([keys] if isinstance(keys, (str, int)) else list(keys))]
    spec = ChooseSpec()
    spec.n_keys = len(ids)
    for i, v in enumerate(ids[:KAS_CHOOSE_MAX_KEYS]):
        spec.key[i] = v
    spec.k = int(k)
    return spec


def topic_front_spec(by, within=None, k: int = 0) -> "FrontSpec":
    """kas_front_spec for the *_topics entries: front_spec with the three name sets, among the criteria and among the bounds."""
    ids = [topic_key_id(n) for n in ([by] if isinstance(by, (str, int)) else list(by))]
    pairs = list(within.items()) if isinstance(within, dict) else list(within or ())
    spec = FrontSpec()
    spec.n_keys = len(ids)
    for i, v in enumerate(ids[:KAS_CHOOSE_MAX_KEYS]):
        spec.key[i] = v
    spec.n_limits = len(pairs)
    for i, (name, limit) in enumerate(pairs[:KAS_CHOOSE_MAX_KEYS]):
        spec.limit_key[i] = topic_key_id(name)
        spec.limit[i] = int(limit)
    spec.k = int(k)
    return spec


# the move list (kas_move / kas_moves): a row's flags, the 16-byte record, where a list goes
KAS_MOVE_REPLICAS, KAS_MOVE_LEADER, KAS_MOVE_ORDER = 1, 2, 4
MOVE_KINDS = {"replicas": KAS_MOVE_REPLICAS, "leader": KAS_MOVE_LEADER, "order": KAS_MOVE_ORDER}
MOVE_DTYPE = _np.dtype([("topic", "<i4"), ("partition", "<i4"), ("flags", "u1"), ("len", "u1"), ("gained", "u1"), ("lost", "u1"),
                        ("cell_at", "<i4")])
MOVES_ENTRIES = ("kas_moves_device", "kas_moves_device16", "kas_solve_host_moves", "kas_solve_host16_moves",
                 "kas_solve_host_choose_moves", "kas_solve_host16_choose_moves")


class Move(C.Structure):
    _fields_ = [("topic", C.c_int32), ("partition", C.c_int32), ("flags", C.c_uint8), ("len", C.c_uint8), ("gained", C.c_uint8),
                ("lost", C.c_uint8), ("cell_at", C.c_int32)]


class Moves(C.Structure):
    _fields_ = [("mask", C.c_int32), ("reserved", C.c_int32), ("move_off", C.c_void_p), ("cell_off", C.c_void_p),
                ("moves", C.c_void_p), ("moves_cap", C.c_int64), ("cells", C.c_void_p), ("cells_cap", C.c_int64)]


def move_mask(kinds) -> int:
    """KAS_MOVE_* mask from kind names (MOVE_KINDS: replicas, leader, order) or a mask number; unknown names raise ValueError."""
    if isinstance(kinds, int):
        return int(kinds)
    mask = 0
    for name in ([kinds] if isinstance(kinds, str) else list(kinds)):
        if name not in MOVE_KINDS:
            raise ValueError("unknown kind of move %r (one of %s)" % (name, ", ".join(MOVE_KINDS)))
        mask |= MOVE_KINDS[name]
    return mask


# execution batches (kas_batch_spec / kas_move_batch / kas_scenario_batches / kas_batches): a scenario's REPLICAS moves cut by caps
KAS_BATCH_END_OF_LIST, KAS_BATCH_MAX_MOVES, KAS_BATCH_INBOUND, KAS_BATCH_OUTBOUND = 0, 1, 2, 3
BATCH_CLOSED_BY = ("end_of_list", "max_moves", "inbound", "outbound")
KAS_BATCH_NODE_LIMIT = 9362
MOVE_BATCH_FIELDS = ("first_move", "n_moves", "topic", "partition", "replicas", "max_inbound", "max_outbound", "closed_by")
SCENARIO_BATCHES_FIELDS = ("n_batches", "n_moves", "replicas", "max_batch_moves", "max_batch_replicas", "closed_by_max_moves",
                           "closed_by_inbound", "closed_by_outbound")
MOVE_BATCH_DTYPE = _np.dtype([(f, "<i4") for f in MOVE_BATCH_FIELDS])
SCENARIO_BATCHES_DTYPE = _np.dtype([(f, "<i4") for f in SCENARIO_BATCHES_FIELDS])
BATCHES_ENTRIES = ("kas_batches_device", "kas_batches_device16", "kas_solve_host_batches", "kas_solve_host16_batches")


class BatchSpec(C.Structure):
    _fields_ = [("cap_inbound", C.c_int32), ("cap_outbound", C.c_int32), ("max_moves", C.c_int32), ("reserved", C.c_int32)]


class Batches(C.Structure):
    _fields_ = [("scenarios", C.c_void_p), ("batches", C.c_void_p), ("stride", C.c_int64)]


def batch_spec(caps) -> "BatchSpec":
    """kas_batch_spec from a BatchSpec or a dict with the keys inbound, outbound, max_moves (missing: 0 = no bound); other keys
    raise ValueError.  The library refuses negative bounds and a spec without any bound."""
    if isinstance(caps, BatchSpec):
        return caps
    caps = dict(caps)
    unknown = set(caps) - {"inbound", "outbound", "max_moves"}
    if unknown:
        raise ValueError("unknown batch bound %s (inbound, outbound, max_moves)" % ", ".join(sorted(map(repr, unknown))))
    spec = BatchSpec()
    spec.cap_inbound, spec.cap_outbound, spec.max_moves = (int(caps.get(k, 0)) for k in ("inbound", "outbound", "max_moves"))
    return spec


# packed rounds (kas_round_spec / kas_move_round / kas_scenario_rounds / kas_rounds): a scenario's REPLICAS moves scheduled under caps
KAS_ROUNDS_MONOTONE = 0
KAS_ROUND_NODE_LIMIT = 9192
MOVE_ROUND_FIELDS = ("n_moves", "replicas", "first_move", "reserved")
SCENARIO_ROUNDS_FIELDS = ("n_rounds", "n_moves", "replicas", "max_round_moves", "max_round_replicas", "raised_by_inbound",
                          "raised_by_outbound", "reserved")
MOVE_ROUND_DTYPE = _np.dtype([(f, "<i4") for f in MOVE_ROUND_FIELDS])
SCENARIO_ROUNDS_DTYPE = _np.dtype([(f, "<i4") for f in SCENARIO_ROUNDS_FIELDS])
ROUNDS_ENTRIES = ("kas_rounds_device", "kas_rounds_device16", "kas_solve_host_rounds", "kas_solve_host16_rounds")


class RoundSpec(C.Structure):
    _fields_ = [("cap_inbound", C.c_int32), ("cap_outbound", C.c_int32), ("policy", C.c_int32), ("reserved", C.c_int32)]


class Rounds(C.Structure):
    _fields_ = [("scenarios", C.c_void_p), ("rounds", C.c_void_p), ("round_stride", C.c_int64), ("round_of", C.c_void_p),
                ("move_stride", C.c_int64)]


def round_spec(caps) -> "RoundSpec":
    """kas_round_spec from a RoundSpec or a dict with the keys inbound, outbound (missing: 0 = no bound) and policy (missing:
    KAS_ROUNDS_MONOTONE); other keys raise ValueError.  The library refuses negative caps and a spec without any cap."""
    if isinstance(caps, RoundSpec):
        return caps
    caps = dict(caps)
    unknown = set(caps) - {"inbound", "outbound", "policy"}
    if unknown:
        raise ValueError("unknown round bound %s (inbound, outbound, policy)" % ", ".join(sorted(map(repr, unknown))))
    spec = RoundSpec()
    spec.cap_inbound, spec.cap_outbound, spec.policy = (int(caps.get(k, 0)) for k in ("inbound", "outbound", "policy"))
    return spec


assert MOVE_ROUND_DTYPE.itemsize == 16 and SCENARIO_ROUNDS_DTYPE.itemsize == 32 and C.sizeof(RoundSpec) == 16 and C.sizeof(Rounds) == 40
assert MOVE_BATCH_DTYPE.itemsize == 32 and SCENARIO_BATCHES_DTYPE.itemsize == 32 and C.sizeof(BatchSpec) == 16 and C.sizeof(Batches) == 24
assert MOVE_DTYPE.itemsize == C.sizeof(Move) == 16 and C.sizeof(Moves) == 56
assert NODE_IMPACT_DTYPE.itemsize == 32 and SCENARIO_IMPACT_DTYPE.itemsize == 32
assert RACK_IMPACT_DTYPE.itemsize == 32 and SCENARIO_RACK_IMPACT_DTYPE.itemsize == 64 and C.sizeof(RackTables) == 32
assert C.sizeof(ChooseSpec) == 24 and C.sizeof(Choice) == 72 and C.sizeof(FrontSpec) == 60
assert TOPIC_RESULT_DTYPE.itemsize == C.sizeof(TopicResult) == 16
assert SCENARIO_RESULT_DTYPE.itemsize == C.sizeof(ScenarioResult) == 32
assert TOPIC_DESC_DTYPE.itemsize == C.sizeof(TopicDesc) == 64
assert SCENARIO_DESC_DTYPE.itemsize == C.sizeof(ScenarioDesc) == 32

_M64 = (1 << 64) - 1


def digest_cell(topic: int, row: int, slot: int, broker: int) -> int:
    """Python twin of kas_digest_cell() in include/kas_abi.h."""
    m32 = 0xFFFFFFFF
    tlo = ((topic + 1) * 0x9E3779B1) & m32
    thi = ((topic + 1) * 0x85EBCA77) & m32
    b = ((broker & m32) ^ tlo ^ 0x7F4A7C15) & m32
    r = ((((row << 4) & m32) | ((slot & 7) << 1) | 1) ^ (thi & 0xFFFFFFFE)) & m32
    x = (b * r + ((r << 32) | b)) & _M64
    x ^= x >> 29
    return x

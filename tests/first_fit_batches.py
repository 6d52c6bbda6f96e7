"""Batches for the first-fit tests whose stranded partitions are reported under ids of the caller's (part_id_off >= 0).

First fit (P4, KAS:162-186) fails a topic at the first partition it cannot place and reports that partition (KAS:183-184).
The kernels find a ROW; the record carries the id the caller knows the row by — aux[part_id_off + row] where the topic has
such a list, else the row index.  Every topic here gets ids 3 p + 5 + topic_index, so an id is never a row index of the
failing row (3 p + 5 + t > p) and says which topic's list it came from.
"""
from __future__ import annotations

import numpy as np

from kafka_assigner_amd import abi
from kafka_assigner_amd.flatten import FlatBatch
from test_emu_parity import _batch, _multi_topic_scenarios


def with_sparse_partition_ids(fb: FlatBatch) -> FlatBatch:
    """the batch with every topic's partitions known as 3 p + 5 + topic_index (appended to the aux pool)"""
    aux = [fb.aux.astype(np.int32)]
    off = int(fb.aux.shape[0])
    topics = fb.topics.copy()
    for t in range(fb.n_topics):
        P = int(topics["n_partitions"][t])
        topics["part_id_off"][t] = off
        aux.append((3 * np.arange(P, dtype=np.int64) + 5 + t).astype(np.int32))
        off += P
    return FlatBatch(scen=fb.scen, topics=topics, node_id=fb.node_id, node_rack=fb.node_rack, cur=fb.cur,
                     aux=np.concatenate(aux), ctx=fb.ctx, out_len=fb.out_len)


def batch_a() -> FlatBatch:
    """six single-topic scenarios of 800 partitions on ~40 brokers, one replaced or some added: one solves, five strand"""
    return with_sparse_partition_ids(_batch(1234, 6, 800, 40, 8, 3, ("replace1", "add_k")))


def batch_b() -> FlatBatch:
    """three scenarios of three topics: topics that solve, topics that strand and the topics skipped behind those"""
    return with_sparse_partition_ids(_multi_topic_scenarios(77, 3, 3, 700, 40, 8, 3))


# name -> (builder, statuses the oracle's topic records must include)
BATCHES = {
    "A": (batch_a, (abi.KAS_OK, abi.KAS_FAIL_UNASSIGNABLE)),
    "B": (batch_b, (abi.KAS_OK, abi.KAS_FAIL_UNASSIGNABLE, abi.KAS_SKIPPED)),
}
_SOLVED = {}


def assert_strands_under_sparse_ids(fb: FlatBatch, want, statuses) -> None:
    """A condition on the batch, from the oracle's solve alone: it has every status in `statuses`, and every failed record
    names its partition by the id constructed above, not by a row index."""
    status = want.topic_results["status"][:fb.n_topics]
    for st in statuses:
        assert (status == st).any(), (st, status.tolist())
    for t in np.nonzero(status == abi.KAS_FAIL_UNASSIGNABLE)[0]:
        pid, P = int(want.topic_results["fail_partition"][t]), int(fb.topics["n_partitions"][t])
        assert pid >= 5 + t and (pid - 5 - t) % 3 == 0 and (pid - 5 - t) // 3 < P, (int(t), pid)
    for s in range(fb.n_scenarios):
        if int(want.scenario_results["status"][s]) != abi.KAS_FAIL_UNASSIGNABLE:
            continue
        t = int(fb.scen["topic_begin"][s]) + int(want.scenario_results["fail_topic"][s])
        assert int(want.scenario_results["fail_partition"][s]) == int(want.topic_results["fail_partition"][t]), s


def solved(name: str):
    """(fb, want) of a named batch: the oracle's solve, computed once and shared by the tests (which leave both as they
    are), with the batch's guard already passed"""
    if name not in _SOLVED:
        from oracle_lib import oracle_solve
        make, statuses = BATCHES[name]
        fb = make()
        want = oracle_solve(fb)
        assert_strands_under_sparse_ids(fb, want, statuses)
        _SOLVED[name] = (fb, want)
    return _SOLVED[name]

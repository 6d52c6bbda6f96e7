"""Batches for the round-7 forms of the fill's row pass and the order kernel's final lists on dword mid rows (p3_rows' SORTED_OUT /
DISTINCT, relax_pick3): shared by tests/test_sorted_rows_emu.py and tests/test_sorted_rows_gpu.py.  Test infrastructure.

Every batch has 512 scenarios — from there on the plan takes the slim fill, kas_p4_kernel and tiles of 64 rows by batch size — of
677 partitions: ten full tiles and a ragged one, two or three tiles to a fill wavefront."""
from __future__ import annotations

import numpy as np

from kafka_assigner_amd import abi
from kafka_assigner_amd import generator as G
from kafka_assigner_amd.flatten import FlatBatch

S = 512
P = 677


def batch_of(scs) -> FlatBatch:
    """scs: one (node ids ascending, node racks, [(cur int32 [rows, width], rf, name hash), ...]) per scenario"""
    n_topics = sum(len(t) for _, _, t in scs)
    scen = np.zeros(len(scs), dtype=abi.SCENARIO_DESC_DTYPE)
    topics = np.zeros(n_topics, dtype=abi.TOPIC_DESC_DTYPE)
    node_off = cur_off = out_off = ti = 0
    cur = []
    for s, (ids, racks, ts) in enumerate(scs):
        scen[s] = (len(ids), ti, len(ts), 0, node_off, -1)
        node_off += len(ids)
        for c, rf, name_hash in ts:
            rows, cw = c.shape
            ow = max(cw, rf, 1)
            topics[ti] = (name_hash, rows, cw, rf, ow, 0, cur_off, out_off, -1, -1, -1)
            cur.append(np.ascontiguousarray(c, dtype=np.int32).reshape(-1))
            cur_off += rows * cw
            out_off += rows * ow
            ti += 1
    return FlatBatch(scen=scen, topics=topics,
                     node_id=np.concatenate([np.asarray(i, dtype=np.int32) for i, _, _ in scs]),
                     node_rack=np.concatenate([np.asarray(r, dtype=np.int32) for _, r, _ in scs]),
                     cur=np.concatenate(cur), aux=np.zeros(0, np.int32), ctx=np.zeros(0, np.int32), out_len=out_off)


def _plain(seed, N, R, max_add=50):
    """512 single-topic scenarios over brokers 0..N-1 on R racks, every BENCH_ACTIONS action (up to 5 brokers leave, up to max_add join)"""
    scs = []
    for s in range(S):
        _, bs = G.scenario_action(seed, s, N, R, actions=G.BENCH_ACTIONS, max_remove=5, max_add=max_add)
        scs.append((bs.node_id, bs.node_rack, [(G.random_assignment(seed + s, P, N, R, 3), 3, 3644)]))
    return scs


HANDED_BACK_40 = (9, 300)          # scenarios of batch_40() whose rows name a KNOWN broker twice


def batch_40() -> FlatBatch:
    """40 brokers on 8 racks, RF 3, and the rows that can go wrong:
    scenario 1: brokers 0-3 and 20 leave; rows 0-3 keep 0, 1, 2 and 3 of their replicas; row 4 names the unknown broker 20 twice (inside the id
                table's range), row 5 the unknown broker 99 twice (outside it) — both stay on the slim path;
    scenario 2: 50 brokers join — the capacity drops to 23 of the ~50 replicas a broker holds: quotas run out inside the tiles;
    scenarios 9 and 300: a row names the known broker 11 twice — not rack-diverse, handed back to kas_fill_kernel;
    scenario 5: its topic is 2 wide (RF 2) in a batch 3 wide;  scenario 7: two topics, the second 300 rows of RF 2."""
    scs = _plain(4100, 40, 8)
    b1 = G.perturb_brokers(40, 8, remove=[0, 1, 2, 3, 20])
    c1 = G.random_assignment(4101, P, 40, 8, 3)
    c1[0] = (0, 1, 2); c1[1] = (0, 1, 10); c1[2] = (0, 9, 10); c1[3] = (8, 9, 10); c1[4] = (20, 20, 13); c1[5] = (99, 99, 14)
    scs[1] = (b1.node_id, b1.node_rack, [(c1, 3, 3644)])
    b2 = G.perturb_brokers(40, 8, add=50)
    scs[2] = (b2.node_id, b2.node_rack, scs[2][2])
    for s in HANDED_BACK_40:
        c = scs[s][2][0][0].copy()
        known = int(scs[s][0][11])
        c[333] = (known, int(scs[s][0][20]), known)
        scs[s] = (scs[s][0], scs[s][1], [(c, 3, 3644)])
    scs[5] = (scs[5][0], scs[5][1], [(G.random_assignment(4105, P, 40, 8, 2), 2, 3644)])
    scs[7] = (scs[7][0], scs[7][1], [scs[7][2][0], (G.random_assignment(4107, 300, 40, 8, 2), 2, 97)])
    return batch_of(scs)


def batch_wide(N: int) -> FlatBatch:
    """N brokers on 50 racks (1,100 and 2,046: node indices >= 1,024 set the flag bit of mid32_pack's middle field); at most 2,047
    brokers in a scenario, the most a dword mid row can name"""
    return batch_of(_plain(7000 + N, N, 50, max_add=min(50, 2047 - N)))


def kept_counts(fb: FlatBatch, s: int, rows) -> list:
    """how many of its current replicas each of `rows` of scenario s's first topic finds in the broker set"""
    sd, td = fb.scen[s], fb.topics[int(fb.scen[s]["topic_begin"])]
    ids = fb.node_id[int(sd["node_off"]):int(sd["node_off"]) + int(sd["n_nodes"])]
    cw = int(td["cur_width"])
    cur = fb.cur[int(td["cur_off"]):int(td["cur_off"]) + int(td["n_partitions"]) * cw].reshape(-1, cw)
    return [int(np.isin(cur[p], ids).sum()) for p in rows]

"""NumPy restatement of ranking and fronting by rack criteria (include/kas_abi.h: KAS_KEY_RACK_BASE and the *_racks entries).
The checker of tests/test_rack_choose_*.py, not a product path; written from the header's definitions.

A criterion is a name or a KAS_KEY_* number of either set: abi.KEY_NAMES (choose_ref.criterion over the scenario record and the
impact record) or abi.RACK_KEY_NAMES (a field of the scenario rack record, or one of the two spreads).  choose_ref and front_ref
compute every ranking and front from criterion columns looked up by key, so the references here hand them record arrays that
carry the rack columns under their own keys: one structured array whose fields are every criterion of both sets.
"""
from __future__ import annotations

import numpy as np

import choose_ref
import front_ref
from kafka_assigner_amd import abi

ALL_NAMES = abi.KEY_NAMES + abi.RACK_KEY_NAMES


def key_name(key) -> str:
    """the name of a criterion given by name or by KAS_KEY_* number (either range)"""
    if isinstance(key, str):
        assert key in abi.KEYS or key in abi.RACK_KEYS, key
        return key
    key = int(key)
    if 0 <= key < abi.KAS_KEY_COUNT:
        return abi.KEY_NAMES[key]
    assert abi.KAS_KEY_RACK_BASE <= key < abi.KAS_KEY_RACK_END, key
    return abi.RACK_KEY_NAMES[key - abi.KAS_KEY_RACK_BASE]


def criterion(sr, si, srk, key) -> np.ndarray:
    """int64 [S]: criterion `key` of every scenario; srk (SCENARIO_RACK_IMPACT_DTYPE [S]) may be None for a broker criterion"""
    name = key_name(key)
    if name in abi.KEYS:
        return choose_ref.criterion(sr, si, name)
    if name == "rack_replica_spread":
        return srk["max_rack_replicas_after"].astype(np.int64) - srk["min_rack_replicas_after"]
    if name == "rack_leader_spread":
        return srk["max_rack_leaders_after"].astype(np.int64) - srk["min_rack_leaders_after"]
    return srk[name].astype(np.int64)


class _Columns:
    """Stands in for the impact records in choose_ref / front_ref: column lookup by criterion name.  Their criterion() reads
    sr[name] for the two scenario-record criteria, computes the two broker spreads from the four extremes and else reads si[name]:
    here si[name] answers every other name of both sets."""

    def __init__(self, sr, si, srk):
        self.sr, self.si, self.srk = sr, si, srk

    def __getitem__(self, name):
        if isinstance(name, slice):
            return _Columns(self.sr[name], self.si[name], None if self.srk is None else self.srk[name])
        if name in abi.SCENARIO_IMPACT_FIELDS:
            return self.si[name]
        return criterion(self.sr, self.si, self.srk, name)


def _names(keys):
    """every key as a name (choose_ref.criterion resolves numbers through abi.KEY_NAMES alone)"""
    return [key_name(k) for k in keys]


def rank_ref(sr, si, srk, keys, k: int):
    """choose_ref.Ranking by criteria of either set"""
    return choose_ref.rank_ref(sr, _Columns(sr, si, srk), _names(keys), k)


def front_of(sr, si, srk, keys, k: int, within=()):
    """front_ref.FrontRef by criteria and bounds of either set"""
    pairs = list(within.items()) if isinstance(within, dict) else list(within)
    return front_ref.front_ref(sr, _Columns(sr, si, srk), _names(keys), k, [(key_name(n), v) for n, v in pairs])


def choose_of(fb, sr, out, imp, srk, keys, k: int):
    """choose_ref.ChoiceRef (rank, chosen, offsets, packed rows, node blocks) by criteria of either set"""
    nodes, si = imp
    S = fb.n_scenarios
    return choose_ref.choose_ref(fb, sr, out, (nodes, _Columns(sr[:S], si[:S], srk[:S])), _names(keys), k)


def front_choice_of(fb, sr, out, imp, srk, keys, k: int, within=()):
    """front_ref.front_choice_ref by criteria and bounds of either set"""
    nodes, si = imp
    S = fb.n_scenarios
    pairs = list(within.items()) if isinstance(within, dict) else list(within)
    return front_ref.front_choice_ref(fb, sr, out, (nodes, _Columns(sr[:S], si[:S], srk[:S])), _names(keys), k,
                                      [(key_name(n), v) for n, v in pairs])

"""NumPy restatement of ranking and fronting by topic criteria (include/kas_abi.h: KAS_KEY_TOPIC_BASE and the *_topics entries).
The checker of tests/test_topic_choose_*.py, not a product path; written from the header's definitions.

A criterion is a name or a KAS_KEY_* number of one of three sets: abi.KEY_NAMES (choose_ref.criterion over the scenario record
and the impact record), abi.RACK_KEY_NAMES (rack_choose_ref.criterion over the scenario rack record) or abi.TOPIC_KEY_NAMES: int32
word key - KAS_KEY_TOPIC_BASE of the scenario topic record, which is the field of that name (the record holds its spreads: no key
is derived, and the sixteenth word, `reserved`, is no criterion).  choose_ref and front_ref compute every ranking and front from
criterion columns looked up by name, so the references here hand them a column lookup over the four record arrays.
"""
from __future__ import annotations

import numpy as np

import choose_ref
import front_ref
import rack_choose_ref
from kafka_assigner_amd import abi

ALL_NAMES = abi.KEY_NAMES + abi.RACK_KEY_NAMES + abi.TOPIC_KEY_NAMES


def key_name(key) -> str:
    """the name of a criterion given by name or by KAS_KEY_* number (any of the three ranges)"""
    if isinstance(key, str):
        assert key in ALL_NAMES, key
        return key
    key = int(key)
    if abi.KAS_KEY_TOPIC_BASE <= key < abi.KAS_KEY_TOPIC_END:
        return abi.TOPIC_KEY_NAMES[key - abi.KAS_KEY_TOPIC_BASE]
    return rack_choose_ref.key_name(key)


def criterion(sr, si, srk, stp, key) -> np.ndarray:
    """int64 [S]: criterion `key` of every scenario; srk (SCENARIO_RACK_IMPACT_DTYPE [S]) and stp (SCENARIO_TOPIC_IMPACT_DTYPE [S])
    may be None when no criterion of their set is asked for"""
    name = key_name(key)
    if name in abi.TOPIC_KEYS:
        return stp[name].astype(np.int64)
    return rack_choose_ref.criterion(sr, si, srk, name)


class _Columns:
    """Stands in for the impact records in choose_ref / front_ref (as rack_choose_ref._Columns does): si[name] answers every
    criterion name of the three sets."""

    def __init__(self, sr, si, srk, stp):
        self.sr, self.si, self.srk, self.stp = sr, si, srk, stp

    def __getitem__(self, name):
        if isinstance(name, slice):
            return _Columns(self.sr[name], self.si[name], None if self.srk is None else self.srk[name],
                            None if self.stp is None else self.stp[name])
        if name in abi.SCENARIO_IMPACT_FIELDS:
            return self.si[name]
        return criterion(self.sr, self.si, self.srk, self.stp, name)


def _names(keys):
    return [key_name(k) for k in keys]


def _pairs(within):
    return [(key_name(n), v) for n, v in (list(within.items()) if isinstance(within, dict) else list(within))]


def rank_ref(sr, si, srk, stp, keys, k: int):
    """choose_ref.Ranking by criteria of the three sets"""
    return choose_ref.rank_ref(sr, _Columns(sr, si, srk, stp), _names(keys), k)


def front_of(sr, si, srk, stp, keys, k: int, within=()):
    """front_ref.FrontRef by criteria and bounds of the three sets"""
    return front_ref.front_ref(sr, _Columns(sr, si, srk, stp), _names(keys), k, _pairs(within))


def _cut(a, S):
    return None if a is None else a[:S]


def choose_of(fb, sr, out, imp, srk, stp, keys, k: int):
    """choose_ref.ChoiceRef (rank, chosen, offsets, packed rows, node blocks) by criteria of the three sets"""
    nodes, si = imp
    S = fb.n_scenarios
    return choose_ref.choose_ref(fb, sr, out, (nodes, _Columns(sr[:S], si[:S], _cut(srk, S), _cut(stp, S))), _names(keys), k)


def front_choice_of(fb, sr, out, imp, srk, stp, keys, k: int, within=()):
    """front_ref.front_choice_ref by criteria and bounds of the three sets"""
    nodes, si = imp
    S = fb.n_scenarios
    return front_ref.front_choice_ref(fb, sr, out, (nodes, _Columns(sr[:S], si[:S], _cut(srk, S), _cut(stp, S))), _names(keys), k,
                                      _pairs(within))

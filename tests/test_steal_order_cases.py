"""The slotted problems of tests/steal_order_cases.py on the CPU, with the oracle: what
tests/test_gpu_steal_order.py may conclude from them.

* Walked in the right order -- ``np.lexsort((task_arrival, task_prio))``, what
  ``dgp_steal_order`` asks of the device -- every case gives its expected result: for a
  reference fixture every array the fixture records, for the others the oracle's answer for
  the problem before it was put into slots.
* Every order in ``WRONG`` (a device sort with that mistake) changes the request list of a
  named case, so the GPU test of that case fails on such a device. The table is printed.
* The cases keep enough requests for the order to matter: 100 or more, except the ones whose
  original has fewer, which keep exactly theirs (``FEWER``).
"""
import numpy as np
import pytest

import steal_cases
import steal_order_cases as C
from conftest import steal_files
from oracle import oracle
from test_oracle_steal import STEAL_KEYS, assert_same

FLOOR = 100
# the originals with fewer requests than FLOOR: the fixture's recorded count / the oracle's
# count for the aimed problem or the cut, which the slotted case must keep exactly
FEWER = {"steal_busy_second.npz": 84, "fill_then_reject": 59, "topk_small": 40, "topk_ties": 97,
         1: 1, 2: 1, 63: 49, 64: 47, 65: 50}

# which mistakes each key scheme exposes (on every fixture tried below). Not exposed: a
# mistake that leaves the walk as it should be under that scheme's keys -- ``rank`` and
# ``packed`` have no negative key and no deciding arrival, ``wide`` decides above bit 32,
# only ``dupes`` has equal pairs.
EXPOSES = {
    "rank": {"slot_order", "high32_prio", "descending"},
    "wide": {"slot_order", "prio_only", "arrival_major", "unsigned_prio", "unsigned_arrival", "low32_prio",
             "low32_arrival", "descending"},
    "packed": {"slot_order", "arrival_major", "low32_prio", "high32_prio", "descending"},
    "extremes": {"slot_order", "prio_only", "arrival_major", "unsigned_prio", "unsigned_arrival", "low32_prio",
                 "low32_arrival", "high32_arrival", "descending"},
    "dupes": set(C.WRONG),
}
WIDE_FIXTURES = ("steal_busy_small.npz", "steal_restricted_small.npz", "steal_spread.npz", "steal_busy_second.npz")
TABLE_CASES = [(f, "wide") for f in WIDE_FIXTURES] + [(f, s) for f in C.SCHEME_FIXTURES for s in C.KEY_SCHEMES]


def _walked_right(q):
    perm = np.lexsort((q["task_arrival"], q["task_prio"]))
    return oracle.steal_balance(C.reorder(C.unkeyed(q), perm)), perm


def _floor(key, n):
    if key in FEWER:
        assert n == FEWER[key], (key, n)
    else:
        assert n >= FLOOR, (key, n)


@pytest.mark.parametrize("scheme", C.FIXTURE_SCHEMES)
@pytest.mark.parametrize("name", steal_files())
def test_fixture_in_slots_walked_right_is_the_fixture(name, scheme):
    q, pi, exp = C.fixture_case(name, scheme)
    assert not np.array_equal(pi, np.arange(len(pi)))
    out, perm = _walked_right(q)
    assert_same(out, exp)  # in the fixture's ids
    assert_same(C.map_back(out, None, perm), C.map_back(exp, pi), keys=STEAL_KEYS)  # and in slot ids
    _floor(name, len(exp["st_task"]))


@pytest.mark.parametrize("scheme", C.KEY_SCHEMES)
@pytest.mark.parametrize("name", C.SCHEME_FIXTURES)
def test_key_scheme_walked_right_is_the_fixture(name, scheme):
    q, pi, exp = C.fixture_case(name, scheme)
    out, perm = _walked_right(q)
    assert_same(out, exp)
    _floor(name, len(exp["st_task"]))
    pr, ar = q["task_prio"], q["task_arrival"]
    if scheme == "extremes":
        for k in (pr, ar):
            assert all(v in k for v in (C.I64.min, -1, 0, C.I64.max))
    if scheme == "packed":  # the whole range of what pack_priority holds, 27 deciding bits
        assert pr.min() == 0 and pr.max() >> 27 == (1 << 36) - 1 and (pr & ((1 << 27) - 1)).max() >= 1 << 26
    if scheme == "dupes":
        pairs = np.stack([pr, ar], 1)
        assert len(np.unique(pairs, axis=0)) == -(-len(pr) // C.DUPES)


@pytest.mark.parametrize("name", steal_cases.NAMES)
def test_aimed_problem_in_slots_walked_right_is_the_original(name):
    q, pi, ref = C.aimed_case(name)
    out, perm = _walked_right(q)
    assert_same(out, ref, keys=tuple(ref))
    _floor(name, len(ref["st_task"]))


@pytest.mark.parametrize("T", C.SIZES)
def test_cut_problem_in_slots_walked_right_is_the_original(T):
    q, pi, ref = C.size_case(T)
    assert len(q["victim"]) == T
    out, perm = _walked_right(q)
    assert_same(out, ref, keys=tuple(ref))
    _floor(T, len(ref["st_task"]))
    if T > 1:
        assert (ref["level"] < 0).any()  # rows in no bin: the last bin key is present


@pytest.mark.parametrize("variant", C.ROWS_VARIANTS)
def test_rows_state_has_requests_and_an_order_of_its_own(variant):
    p, _, ref = C.rows_case(variant)
    T = len(p["victim"])
    assert len(ref["st_task"]) >= FLOOR
    perm = np.lexsort((p["task_arrival"], p["task_prio"]))
    assert not np.array_equal(perm, np.arange(T))
    if variant == "pk_bad":  # the host's ranks
        assert np.array_equal(np.sort(p["task_prio"]), np.arange(T)) and not p["task_arrival"].any()
    else:  # packed priorities; the tasks put again arrived after every first arrival
        assert len(np.unique(p["task_prio"])) == T and p["task_arrival"].max() >= 2000
    # walked in slot order instead, the requests differ
    plain = oracle.steal_balance(C.unkeyed(p))
    assert not (np.array_equal(plain["st_task"], ref["st_task"]) and np.array_equal(plain["st_thief"], ref["st_thief"]))


def _caught(q, pi, exp, name):
    walk, perm = C.wrong_walk(q, name)
    out = oracle.steal_balance(walk)
    st = pi[perm[np.asarray(out["st_task"], np.int64)]]  # in the original's ids
    return not (np.array_equal(st, exp["st_task"]) and np.array_equal(out["st_thief"], exp["st_thief"]))


def test_every_wrong_order_changes_the_requests_of_a_named_case(capsys):
    catches = {w: [] for w in C.WRONG}
    for name, scheme in TABLE_CASES:
        q, pi, exp = C.fixture_case(name, scheme)
        got = {w for w in C.WRONG if _caught(q, pi, exp, w)}
        assert got == EXPOSES[scheme], (name, scheme, sorted(got ^ EXPOSES[scheme]))
        for w in got:
            catches[w].append(f"{name[6:-4]}/{scheme}")
    with capsys.disabled():
        print()
        for w, by in catches.items():
            print(f"  {w:17s} caught by {len(by):2d}: {' '.join(by)}")
    for w, by in catches.items():
        assert by, f"no case catches {w}"
    # the mistakes only one scheme is there for
    assert all("/packed" in c or "/dupes" in c for c in catches["high32_prio"])
    assert all("/extremes" in c or "/dupes" in c for c in catches["high32_arrival"])
    assert all("/dupes" in c for c in catches["unstable_ties"])


@pytest.mark.parametrize("scheme", C.FIXTURE_SCHEMES)
def test_slot_order_changes_the_requests_of_every_fixture(scheme):
    for name in steal_files():
        q, pi, exp = C.fixture_case(name, scheme)
        assert _caught(q, pi, exp, "slot_order"), name

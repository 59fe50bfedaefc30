"""The device's own ordering of the steal problem's rows (needs an MI355X): dgp_steal_order.

``GPUWorkStealing.balance()`` hands over its task rows in slot order with a (priority,
arrival) key each; dgp_steal_load sorts them on the device (two sign flips, two stable
64-bit radix passes, the permutation feeding the bin sort) and every later kernel reaches a
task's inputs through that permutation. The other GPU tests pass problems already in walk
order, where the permutation is the identity and position = task id. Here every problem
comes in slots (tests/steal_order_cases.py); tests/test_steal_order_cases.py shows on the
CPU that each mistake such a sort could make changes the requests of one of these cases.
All comparisons are bit-exact (``assert_same``).

* every reference fixture in slots, keys ``rank`` and ``wide``: the fixture's arrays with the
  task ids relabelled (fresh levels, restricted rows, the second balance() with ``level_in``);
* the key schemes ``packed``, ``extremes`` and ``dupes`` on three of them;
* every aimed problem of tests/steal_cases.py in slots: the chunk, window and run paths with
  task ids that do not ascend inside a bin;
* one problem cut to the sizes around the sort's and the kernels' block sizes;
* the sliced path (thief rows per engine, pack, unpack, run) under an order;
* ``StealRows.problem`` of a plugin state after puts, removals, slot reuse and re-puts, with
  packed keys and with the host's ranks (one priority that does not pack);
* the contract of the keys: they are for one load, which refuses another n_tasks and drops
  them however it ends.
"""
import numpy as np
import pytest

import steal_cases
import steal_order_cases as C
from conftest import steal_files
from distributed_amd.engine import PlacementEngine, _ptr
from oracle import oracle
from test_gpu_shard import _sliced
from test_oracle_steal import STEAL_KEYS, assert_same

pytestmark = pytest.mark.gpu

DGP_E_ARG = -1  # include/dgplace.h


@pytest.fixture(scope="module")
def eng():
    e = PlacementEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def pair():
    with PlacementEngine(0) as a, PlacementEngine(0) as b:
        yield [a, b]


@pytest.mark.parametrize("scheme", C.FIXTURE_SCHEMES)
@pytest.mark.parametrize("name", steal_files())
def test_fixture_in_slots(eng, name, scheme):
    q, pi, exp = C.fixture_case(name, scheme)
    assert_same(eng.steal_balance(q), C.map_back(exp, pi))


@pytest.mark.parametrize("scheme", C.KEY_SCHEMES)
@pytest.mark.parametrize("name", C.SCHEME_FIXTURES)
def test_key_schemes(eng, name, scheme):
    q, pi, exp = C.fixture_case(name, scheme)
    assert_same(eng.steal_balance(q), C.map_back(exp, pi))


@pytest.mark.parametrize("name", steal_cases.NAMES)
def test_aimed_problem_in_slots(eng, name):
    q, pi, ref = C.aimed_case(name)
    assert_same(eng.steal_balance(q), C.map_back(ref, pi), keys=tuple(ref))


@pytest.mark.parametrize("T", C.SIZES)
def test_sizes_of_the_sort(eng, T):
    q, pi, ref = C.size_case(T)
    assert_same(eng.steal_balance(q), C.map_back(ref, pi), keys=tuple(ref))


@pytest.mark.parametrize("variant", C.ROWS_VARIANTS)
def test_steal_rows_problem(eng, variant):
    """What the plugin sends: rows.problem(plugin) as it is, against the oracle on
    ordered_problem of it."""
    p, _, ref = C.rows_case(variant)
    assert_same(eng.steal_balance(p), ref, keys=tuple(ref))


def _sliced_cases():
    q, pi, exp = C.fixture_case("steal_busy_restricted.npz", "wide")
    yield q, C.map_back(exp, pi), STEAL_KEYS
    q, pi, ref = C.aimed_case("busy_runs")
    yield q, C.map_back(ref, pi), tuple(ref)
    p, _, ref = C.rows_case("packed")
    yield p, ref, tuple(ref)


@pytest.mark.parametrize("k", range(3), ids=["fixture", "aimed", "rows"])
def test_sliced_over_two_engines_under_an_order(pair, k):
    """Each engine gets the keys before its dgp_steal_load (``_steal_args``), computes its
    slice of the thief rows by sorted position and both walk."""
    q, want, keys = list(_sliced_cases())[k]
    for out in _sliced(pair, q):
        assert_same(out, want, keys=keys)


# ------------------------------------------------------------------ the contract of the keys
def _order(e, q):
    pr = np.ascontiguousarray(q["task_prio"], np.int64)
    ar = np.ascontiguousarray(q["task_arrival"], np.int64)
    return e.lib.dgp_steal_order(e.h, len(pr), _ptr(pr), _ptr(ar))


def _plain(e, p):
    """dgp_steal_balance of ``p`` with no dgp_steal_order before it -> (rc, outputs)."""
    assert p.get("task_prio") is None
    inputs, outputs, out, n, keep = e._steal_args(p)
    rc = e.lib.dgp_steal_balance(e.h, *inputs, *outputs)
    return rc, (e._steal_result(out, n) if rc == 0 else None)


@pytest.fixture(scope="module")
def stale():
    """A slotted fixture, the problem without its keys, and that problem's own answer (walked
    in slot order), which the keys would change."""
    q, pi, exp = C.fixture_case("steal_busy_small.npz", "wide")
    p = C.unkeyed(q)
    ref = oracle.steal_balance(p)
    keyed = C.map_back(exp, pi)
    assert not (np.array_equal(ref["st_task"], keyed["st_task"]) and np.array_equal(ref["st_thief"], keyed["st_thief"]))
    return q, p, ref, keyed


def test_keys_for_another_n_tasks_are_refused(eng, stale):
    q, p, ref, keyed = stale
    other = C.unkeyed(C.size_case(257)[0])
    assert len(other["victim"]) != len(p["victim"])
    assert _order(eng, q) == 0
    rc, _ = _plain(eng, other)
    assert rc == DGP_E_ARG
    assert b"dgp_steal_order" in eng.lib.dgp_last_error(eng.h)
    rc, out = _plain(eng, p)  # as many tasks as the refused keys: walked in input order all the same
    assert rc == 0
    assert_same(out, ref, keys=tuple(ref))


def test_a_refused_load_drops_the_keys(eng, stale):
    q, p, ref, keyed = stale
    bad = dict(p, occ=p["occ"].copy())
    bad["occ"][int(np.flatnonzero(p["idle"])[0])] = -1.0
    assert _order(eng, q) == 0
    rc, _ = _plain(eng, bad)
    assert rc == DGP_E_ARG
    assert b"occupancy" in eng.lib.dgp_last_error(eng.h)
    rc, out = _plain(eng, p)
    assert rc == 0
    assert_same(out, ref, keys=tuple(ref))


def test_keys_hold_for_one_balance(eng, stale):
    q, p, ref, keyed = stale
    assert_same(eng.steal_balance(q), keyed)
    rc, out = _plain(eng, p)
    assert rc == 0
    assert_same(out, ref, keys=tuple(ref))


def test_no_keys_for_no_tasks(eng, stale):
    q, p, ref, keyed = stale
    z = np.zeros(0)
    empty = dict(p, victim=z.astype(np.int32), duration=z, fast=z.astype(np.uint8), dep_ptr=np.zeros(1, np.int64),
                 dep_idx=z.astype(np.int32))
    assert eng.lib.dgp_steal_order(eng.h, 0, None, None) == 0
    rc, out = _plain(eng, empty)
    assert rc == 0
    want = oracle.steal_balance(empty)
    assert len(out["st_task"]) == 0
    assert_same(out, want, keys=tuple(want))
    assert eng.lib.dgp_steal_order(eng.h, 0, None, None) == 0  # keys for no task, then tasks: another n_tasks
    rc, _ = _plain(eng, p)
    assert rc == DGP_E_ARG
    rc, out = _plain(eng, p)
    assert rc == 0
    assert_same(out, ref, keys=tuple(ref))

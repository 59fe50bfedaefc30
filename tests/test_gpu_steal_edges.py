"""HIP WorkStealing.balance() at the edges of its own bookkeeping (needs an MI355X).

* Every aimed problem of tests/steal_cases.py -- busy thieves in many runs of equal stack
  time, rows of 0..4 and more than MAXH holders, rounding ties across runs, searches past
  the 64-run window, exact bin sizes, a rejection on the lane after a fill, the victim
  paths at 19 / 20 saturated and topk below 10 workers, the plugin's state as input -- is
  bit-exact against the oracle, ``checked`` included. tests/test_steal_census.py shows on
  the CPU which kernel paths each of them reaches.
* The run-heavy, many-holder and restricted ones also go through the sliced path (thief
  rows per engine, packed 128-byte records, unpack, run) on two engines.
* ABI edges of dgp_steal_load: nthreads 65535 / 65536, the largest W whose balance state
  fits the 160 KiB of LDS and the next one, negative / NaN occupancy refused, -0.0 taken
  as 0.0.
"""
import ctypes as C

import numpy as np
import pytest

import steal_cases
from distributed_amd import graphs
from distributed_amd.engine import PlacementEngine
from oracle import oracle
from test_gpu_shard import _sliced
from test_oracle_steal import assert_same

pytestmark = pytest.mark.gpu

NAMES = steal_cases.NAMES  # the problems are built at their first use, not at collection
DGP_E_ARG = -1  # include/dgplace.h


@pytest.fixture(scope="module")
def eng():
    e = PlacementEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def refs():
    cache = {}

    def ref(name):
        if name not in cache:
            cache[name] = oracle.steal_balance(steal_cases.problem(name))
        return cache[name]

    return ref


@pytest.mark.parametrize("name", NAMES)
def test_aimed_problem_matches_oracle(eng, refs, name):
    p, ref = steal_cases.problem(name), refs(name)
    assert len(ref["st_task"]) > 0
    assert_same(eng.steal_balance(p), ref, keys=tuple(ref))


@pytest.fixture(scope="module")
def pair():
    with PlacementEngine(0) as a, PlacementEngine(0) as b:
        yield [a, b]


@pytest.mark.parametrize("name", steal_cases.SLICED)
def test_aimed_problem_sliced_over_two_engines(pair, refs, name):
    """The 128-byte row carries nh, hw, hg, hr of 3-, 4- and more-than-MAXH-holder tasks and the
    thief of restricted ones from the engine that computed them to the one that walks."""
    ref = refs(name)
    for out in _sliced(pair, steal_cases.problem(name)):
        assert_same(out, ref, keys=tuple(ref))


def _rc(e, p):
    inputs, outputs, out, n, keep = e._steal_args(p)
    return e.lib.dgp_steal_balance(e.h, *inputs, *outputs)


def _four_workers(nthreads_thief):
    """Worker 0 loaded, 1..3 thieves; worker 3 with ``nthreads_thief`` threads."""
    p = graphs.steal_problem(4, 60, hot_frac=0.25, seed=7)
    v = int(p["victim"][0])
    th = [w for w in range(4) if w != v]
    p["nthreads"] = p["nthreads"].copy()
    p["nthreads"][th[-1]] = nthreads_thief
    p["total_nthreads"] = int(p["nthreads"].sum())
    return p


def test_nthreads_limit(eng):
    p = _four_workers(65535)
    ref = oracle.steal_balance(p)
    big = int(np.flatnonzero(p["nthreads"] == 65535)[0])
    assert big in ref["st_thief"]  # the 65535-thread worker is a thief that takes tasks
    assert_same(eng.steal_balance(p), ref, keys=tuple(ref))
    q = _four_workers(65536)
    assert _rc(eng, q) == DGP_E_ARG
    assert_same(eng.steal_balance(p), ref, keys=tuple(ref))  # the refusal left the engine usable


def _lds_bytes(W):  # balance_lds_bytes (dgp_steal.h, which points here): the layout restated
    return ((W * (8 + 8 + 4) + (6 * W + 2) * 2 + W * 4 + W) + 15) & ~15


def test_worker_limit_of_the_balance_state(eng):
    W = max(w for w in range(4000, 4600) if _lds_bytes(w) <= 160 * 1024)
    assert _lds_bytes(W + 1) > 160 * 1024
    p = graphs.steal_problem(W, 2000, seed=9, hot_frac=0.01)
    ref = oracle.steal_balance(p)
    assert len(ref["st_task"]) > 0
    assert_same(eng.steal_balance(p), ref, keys=tuple(ref))
    q = graphs.steal_problem(W + 1, 2000, seed=9, hot_frac=0.01)
    assert _rc(eng, q) == DGP_E_ARG


@pytest.mark.parametrize("bad", [-1e-300, -1.0, float("nan"), -float("inf")])
def test_negative_or_nan_occupancy_is_refused(eng, bad):
    p = steal_cases.problem(NAMES[0])
    q = dict(p, occ=p["occ"].copy())
    q["occ"][int(np.flatnonzero(p["idle"])[5])] = bad
    assert _rc(eng, q) == DGP_E_ARG
    with pytest.raises(Exception, match="occupancy"):
        eng.steal_balance(q)


def test_two_thieves_at_plus_and_minus_zero(eng):
    """Worker 0 loaded; the thieves 1 (+0.0) and 2 (-0.0) are one run: every task's thief is
    the one of less ws.nbytes, then index, whichever sign its zero has."""
    for wnb in ([0, 5, 3], [0, 3, 5], [0, 4, 4]):
        p = dict(nthreads=np.array([2, 2, 2], np.int32), occ=np.array([40.0, 0.0, -0.0]),
                 nproc=np.array([40, 0, 0], np.int32), wnbytes=np.array(wnb, np.int64),
                 idle=np.array([0, 1, 1], np.uint8), sat=np.array([1, 0, 0], np.uint8), total_occ=40.0,
                 total_nthreads=6, bandwidth=100_000_000, victim=np.zeros(40, np.int32), duration=np.ones(40),
                 fast=np.zeros(40, np.uint8), dep_ptr=np.zeros(41, np.int64), dep_idx=np.zeros(0, np.int32),
                 data_nbytes=np.zeros(1, np.int64), data_get_nbytes=np.zeros(1, np.int64),
                 data_holder=np.array([-1], np.int32))
        ref = oracle.steal_balance(p)
        assert set(ref["st_thief"].tolist()) == {1, 2}
        assert_same(eng.steal_balance(p), ref, keys=tuple(ref))


def test_minus_zero_among_busy_thieves(eng):
    """-0.0 beside +0.0 and positive stack times: as bits it would sort after every one of
    them and the search's early exit (a later run starts later) would skip it."""
    p = steal_cases.problem(NAMES[0])
    cold = np.flatnonzero(p["idle"])
    q = dict(p, occ=p["occ"].copy())
    q["occ"][cold[0:40:4]] = -0.0
    q["occ"][cold[1:40:4]] = 0.0
    ref = oracle.steal_balance(q)
    assert set(ref["st_thief"].tolist()) & set(cold[0:40:4].tolist())
    assert_same(eng.steal_balance(q), ref, keys=tuple(ref))

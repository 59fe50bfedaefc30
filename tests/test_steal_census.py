"""Which paths of the device balance() the steal problems reach (CPU; tests/steal_census.py).

* The census itself: its walk reproduces the request list of every steal fixture and every
  aimed problem (it asserts that before it counts), and it refuses a request list that is
  not the problem's.
* The gap it was written to close, pinned: every steal fixture from before the busy-thief
  family has exactly one run of equal stack time among its thieves (all idle at 0.0) and no
  search that saw more than 64 live runs; the reference's own unit scenarios have at most
  two runs.
* The aimed problems (tests/steal_cases.py, run on the device by test_gpu_steal_edges.py)
  meet their floors, and every site of ``steal_census.SITES`` is reached by one of them.
* The busy-thief reference fixtures (gen_steal.py ``warm=``): many runs, the zero run a
  minority, winners outside the first live run, emptied runs crossed, holders tying
  non-holders.
"""
import os

import numpy as np
import pytest

import steal_cases
import steal_census
from conftest import GOLDEN, STEAL_REFTESTS, steal_files
from oracle import oracle

BUSY = [f for f in steal_files() if f.startswith("steal_busy_")]
OLD = [f for f in steal_files() if not f.startswith("steal_busy_")]
NAMES = steal_cases.NAMES
# A floor of 1: the exact saturated counts and the topk below 10 workers, and the two sites that
# one balance() can reach only once (the thief set runs out; the topk path from 10 workers), for
# which ">= 3 in some problem" cannot be met. Every other site: >= 3.
ONCE = {"win.thieves_exhausted_midchunk", "vict.topk_w_lt10", "vict.topk_w_ge10", "vict.nsat19", "vict.nsat20"}


@pytest.fixture(scope="module")
def fixture_census():
    out = {}
    for name in steal_files():
        p, exp, meta = oracle.load_steal_fixture(os.path.join(GOLDEN, name))
        out[name] = (p, steal_census.census(p, exp))
    return out


@pytest.fixture(scope="module")
def case_census():
    return {n: steal_census.census(steal_cases.problem(n), oracle.steal_balance(steal_cases.problem(n))) for n in NAMES}


def test_busy_family_present():
    assert sorted(BUSY) == [f"steal_busy_{k}.npz" for k in ("restricted", "runs", "second", "small", "threads", "topk")]
    assert len(OLD) == 7


@pytest.mark.parametrize("name", OLD)
def test_old_fixtures_have_one_run(fixture_census, name):
    p, c = fixture_census[name]
    n, runs, zero = steal_census.thief_runs(p)
    assert runs == 1 and zero == n, (n, runs, zero)
    assert c["search.live_runs_gt64"] == 0 and c["search.winner_not_first_run"] == 0
    assert c["search.tie_across_runs"] == 0 and c["search.past_window"] == 0


def test_reference_unit_scenarios_have_two_runs_at_most():
    for name, p, exp in oracle.load_steal_problems(os.path.join(GOLDEN, STEAL_REFTESTS)):
        assert len(p["nthreads"]) <= 5 and steal_census.thief_runs(p)[1] <= 2, name
        steal_census.census(p, exp)  # the walk holds on them too


def test_census_refuses_a_foreign_request_list():
    p = steal_cases.problem(NAMES[0])
    ref = oracle.steal_balance(p)
    bad = dict(ref, st_thief=ref["st_thief"].copy())
    bad["st_thief"][len(bad["st_thief"]) // 2] ^= 1
    with pytest.raises(AssertionError, match="census walk"):
        steal_census.census(p, bad)
    with pytest.raises(AssertionError, match="census walk"):
        steal_census.census(p, {k: (v[:-1] if k.startswith("st_") else v) for k, v in ref.items()})


@pytest.mark.parametrize("name", NAMES)
def test_aimed_problem_meets_its_floors(case_census, name):
    p, floors, c = steal_cases.problem(name), steal_cases.floors(name), case_census[name]
    assert len(p["nthreads"]) <= 256 and len(p["victim"]) <= 4000
    assert steal_census.byte_sum_bound(p) < 2 ** 53
    assert set(floors) <= set(steal_census.SITES)
    short = {s: (c[s], need) for s, need in floors.items() if c[s] < need}
    assert not short, short


def test_every_site_has_an_aimed_problem():
    """Each site is a floor of some aimed problem: >= 3 there (>= 1 for ``ONCE``), and the
    figures the issue sets."""
    best = {}
    for name in NAMES:
        for s, need in steal_cases.floors(name).items():
            best[s] = max(best.get(s, 0), need)
    assert not [s for s in steal_census.SITES if best.get(s, 0) < (1 if s in ONCE else 3)]
    for s, need in {"search.live_runs_gt64": 100, "search.tie_across_runs": 10, "rows.nh3": 20, "rows.nh4": 20,
                    "rows.many": 20, "search.holder_at_min_start": 20, "bin.size64": 1, "bin.size65": 1,
                    "bin.size1": 3, "bin.size63": 3, "bin.size128": 3, "bin.size129": 3}.items():
        assert best[s] >= need, (s, best[s])


def test_sliced_cases_carry_every_row_kind(case_census):
    tot = sum((case_census[name] for name in steal_cases.SLICED), steal_census.Counter())
    for s in ("rows.nh0", "rows.nh1", "rows.nh2", "rows.nh3", "rows.nh4", "rows.many", "restr.valid",
              "restr.none_strict", "search.live_runs_gt64"):
        assert tot[s] >= 3, s


@pytest.mark.parametrize("name", BUSY)
def test_busy_fixture_thieves_fall_into_many_runs(name):
    p, exp, meta = oracle.load_steal_fixture(os.path.join(GOLDEN, name))
    n, runs, zero = steal_census.thief_runs(p)
    assert runs >= 20 and 2 * zero < n, (n, runs, zero)
    if name == "steal_busy_runs.npz":
        assert runs > 64
    assert os.path.getsize(os.path.join(GOLDEN, name)) < max(os.path.getsize(os.path.join(GOLDEN, f)) for f in OLD)


def test_busy_fixtures_reach_the_run_search(fixture_census):
    tot = sum((fixture_census[f][1] for f in BUSY), steal_census.Counter())
    assert tot["search.winner_not_first_run"] >= 30
    assert tot["search.crossed_empty_run"] >= 30 and tot["search.first_run_changed"] >= 30
    assert fixture_census["steal_busy_runs.npz"][1]["search.live_runs_gt64"] >= 100
    assert tot["search.holder_tie_wins"] + tot["search.holder_tie_loses"] >= 3
    assert tot["search.holder_wins"] >= 30 and tot["search.again"] >= 30


def test_busy_fixtures_cover_their_inputs(fixture_census):
    p, c = fixture_census["steal_busy_second.npz"]
    assert c["in.level_in_neg"] >= 3 and c["in.inflight_in"] >= 3 and len(p["level_in"]) == len(p["victim"])
    p, c = fixture_census["steal_busy_threads.npz"]
    assert set(np.unique(p["nthreads"]).tolist()) == {1, 2, 4, 64} and c["in.nthreads_mixed"]
    p, c = fixture_census["steal_busy_topk.npz"]
    assert int(p["sat"].sum()) == 0 and c["vict.topk_w_ge10"] == 1
    p, c = fixture_census["steal_busy_restricted.npz"]
    assert c["restr.valid"] >= 3 and c["restr.none_loose"] >= 3 and c["restr.none_strict"] >= 3

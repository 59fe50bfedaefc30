"""The ``edge_*`` fixtures reach the edges they were made for (CPU only).

Each fixture (tests/golden/gen_golden.py ``edge_fixtures``) pins the engines at a shape
where they change path: the stream engine's local / global classification of a stimulus
(csrc/dgp_stream.h ``build_desc``: KT_MAX = 24, KX_MAX = 8, NE = 64, TMAX = 32, PLC = 64,
RC_MAX = 8) and the hand-over to the round-kernel engine past PX = 32 task prefixes. A
fixture that never produced a stimulus next to a limit would pass on a kernel that is wrong
there, so the conditions below are asserted on the inputs themselves: the graph and the
reference's placement log, walked by ``stimulus_census`` (tests/stimulus_census.py) in the
order the prefetcher applies its tests. A limit counts as reached only by a stimulus the
walk has not already made global for another reason: the mixed fan-in graphs reach 64
entries and 32 workers only on stimuli that are global by their dependency counts, so those
two limits are bound by the layered fixtures. Nothing here measures the code under test.
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from oracle import oracle
from stimulus_census import REASONS, max_worker_prefixes, scan_mode_refills, stimulus_census

MIXED = ["edge_mixed_w48_sat1.1", "edge_mixed_w48_satinf", "edge_mixed_w200_sat1.1", "edge_p40_mixed_sat1.1"]
ROUND_ENGINE = ["edge_p33_sat1.1", "edge_p40_sat1.1", "edge_p40_satinf", "edge_p64_sat1.1", "edge_p40_w1100_sat1.1",
                "edge_p40_restr_sat1.1", "edge_p40_mixed_sat1.1"]
LOCAL, BY_KT, BY_KX, BY_NE, BY_TMAX, BY_PLC = (REASONS.index(k) for k in ("local", "kt", "kx", "ne", "tmax", "plc"))

_cache = {}


def census(name):
    """(graph, config, expected outputs, census) of a fixture, computed once."""
    if name not in _cache:
        g, cfg, exp, meta = oracle.load_fixture(os.path.join(GOLDEN, name + ".npz"))
        _cache[name] = (g, cfg, exp, stimulus_census(g, exp, cfg["saturation"]))
    return _cache[name]


def count(a, v):
    return int((np.asarray(a) == v).sum())


def both(mask, a, v):
    return int((mask & (np.asarray(a) == v)).sum())


def test_every_edge_fixture_is_covered_here():
    have = sorted(f[:-4] for f in os.listdir(GOLDEN) if f.startswith("edge_") and f.endswith(".npz"))
    assert have == sorted(set(MIXED + ROUND_ENGINE + ["edge_p32_sat1.1", "edge_threads_sat1.1", "edge_layers_ne_sat1.1",
                                                       "edge_layers_tmax_sat1.1", "edge_restr_wide_sat1.1", "edge_scan_refill_sat1.1",
                                                       "edge_w1_sat1.1"]))


def test_census_on_a_graph_counted_by_hand():
    """Tasks 0..3 are roots on workers 0, 1, 2, 0; 4 needs {0, 1, 2}, 5 needs {3}, 6 needs
    {3, 4}; 5 and 6 are wanted. Completing 3 readies 5; completing 2 (last of 0, 1, 2) readies
    4; completing 4 releases 0, 1, 2 (three entries, their holders touched) and readies 6,
    whose dependencies are held by workers 0 and 1; completing 6 releases 3 and 4."""
    g = dict(n_tasks=7, dep_ptr=np.array([0, 0, 0, 0, 0, 3, 4, 6]), dep_idx=np.array([0, 1, 2, 3, 3, 4]),
             nthreads=np.array([2, 57, 1]), prio=np.arange(7), wanted=np.array([0, 0, 0, 0, 0, 1, 1]))
    out = dict(pl_task=np.array([3, 0, 1, 2, 5, 4, 6]), pl_worker=np.array([0, 0, 1, 2, 2, 1, 0]))
    c = stimulus_census(g, out, 1.1)
    assert c["kt"].tolist() == [0, 0, 0, 0, 1, 3, 2]
    assert c["nf"].tolist() == [1, 0, 0, 1, 0, 1, 0]
    assert c["kx"].tolist() == [1, 3, 2] and c["kx_local"].tolist() == [1, 3]
    # worker 1 has 57 threads: ceil(57 * 1.1) = 63 refill rows + 1 ready task + 1 > 64
    assert c["reason"].tolist() == [LOCAL] * 5 + [BY_PLC, LOCAL]
    assert c["n"].tolist() == [9, 7, 7, 11, 8, 7 + 3 + 3 + 3, 7 + 2 + 2]
    assert c["nt"].tolist() == [1, 1, 1, 3, 1, 3, 2]
    assert c["entries_all"].tolist() == [9, 7, 7, 11, 8, 13, 9]
    assert c["nt_all"].tolist() == [1, 1, 1, 3, 1, 2, 1]
    # ceil(2 * 1.1) = 3, ceil(57 * 1.1) = 63, ceil(1.1) = 2
    assert c["staging"].tolist() == [1 + 3 + 1, 3 + 1, 63 + 1, 1 + 2 + 1, 2 + 1, 1 + 63 + 1, 3 + 1]
    assert stimulus_census(g, out, "inf")["staging"].tolist() == [2, 1, 1, 2, 1, 2, 1]
    out["round_nplaced"] = np.array([4, 2, 1, 0])
    g["prefix_id"] = np.array([0, 1, 2, 3, 4, 5, 6])
    # worker 0 is given tasks 3, 0 (round 0) and 6 (round 2); worker 2 tasks 2 and 5 in rounds 0, 1
    assert max_worker_prefixes(g, out) == 2


def test_census_stops_where_the_prefetcher_stops():
    """Nine roots, task 9 needs all of them, task 10 only root 8, which completes last: the
    walk meets task 9 first (9 dependencies: global) and counts nothing after it."""
    g = dict(n_tasks=11, dep_ptr=np.array([0] * 10 + [9, 10]), dep_idx=np.array(list(range(9)) + [8]),
             nthreads=np.array([1, 1]), prio=np.arange(11), wanted=np.array([0] * 9 + [1, 1]))
    out = dict(pl_task=np.arange(11), pl_worker=np.array([0, 1] * 5 + [0]))
    c = stimulus_census(g, out, 1.1)
    assert c["reason"].tolist() == [LOCAL] * 8 + [BY_KX, LOCAL, LOCAL]
    assert c["nf"][8] == 2 and c["n"][8] == 7 and c["nt"][8] == 1
    assert c["entries_all"][8] == 7 + 10 + 2 and c["nt_all"][8] == 2
    assert c["kx"].tolist() == [9, 1] and c["kx_local"].tolist() == []


@pytest.mark.parametrize("name", MIXED)
def test_mixed_fixtures_sit_on_both_sides_of_the_dependency_limits(name):
    """KT_MAX and KX_MAX, counted jointly: stimuli the walk leaves local at kt = 24 and with a
    ready task at kx = 8, next to stimuli made global by kt = 25 and by kx = 9. The marginal
    counts of 64 / 65 entries and 32 / 33 workers are conditions on the graphs too, but every
    such stimulus is global by kt or kx before the device counts that far: they bind nothing
    (see the layered fixtures)."""
    g, cfg, exp, c = census(name)
    loc = c["reason"] == LOCAL
    print(name, "reasons", dict(zip(REASONS, np.bincount(c["reason"], minlength=len(REASONS)).tolist())),
          {f"kt={v}": (both(loc, c["kt"], v), count(c["kt"], v)) for v in (23, 24, 25, 26)},
          {f"kx={v}": (count(c["kx_local"], v), count(c["kx"], v)) for v in (7, 8, 9, 10)},
          "largest local n", int(c["n"][loc].max()), "nt", int(c["nt"][loc].max()))
    assert len(c["kt"]) == g["n_tasks"]
    assert both(loc, c["kt"], 24) >= 20 and both(c["reason"] == BY_KT, c["kt"], 25) >= 20
    assert count(c["kx_local"], 8) >= 20 and count(c["kx"], 9) >= 20 and count(c["reason"], BY_KX) >= 20
    for v in (24, 25):
        assert count(c["kt"], v) >= 20, (v, count(c["kt"], v))
    for v in (8, 9):
        assert count(c["kx"], v) >= 20, (v, count(c["kx"], v))
    for v in (64, 65):
        assert count(c["entries_all"], v) >= 1, v
    if name in ("edge_mixed_w48_sat1.1", "edge_mixed_w200_sat1.1"):
        for v in (32, 33):
            assert count(c["nt_all"], v) >= 1, v


def test_layers_fixture_fills_the_descriptor_and_trips_at_65():
    """NE: stimuli the walk leaves local with 63 and with exactly 64 entries (release
    entries included), and stimuli global only because the next ready task would make 65."""
    g, cfg, exp, c = census("edge_layers_ne_sat1.1")
    loc = c["reason"] == LOCAL
    print({f"local n={v}": both(loc, c["n"], v) for v in (62, 63, 64)},
          {f"trip at {v}": count(c["trip_n"], v) for v in (65, 66, 67)},
          "reasons", dict(zip(REASONS, np.bincount(c["reason"], minlength=len(REASONS)).tolist())))
    assert int(c["kt"].max()) <= 8 and int(c["kx"].max()) <= 8  # nothing is global by kt or kx
    assert both(loc, c["n"], 63) >= 3 and both(loc, c["n"], 64) >= 3
    assert both(c["reason"] == BY_NE, c["trip_n"], 65) >= 3
    assert int(c["n"][loc].max()) == 64


def test_layers_fixture_touches_32_workers_local_and_33_global():
    """TMAX: stimuli the walk leaves local with exactly 32 workers touched, and stimuli whose
    descriptor fits (at most 64 entries) that are global only by touching 33."""
    g, cfg, exp, c = census("edge_layers_tmax_sat1.1")
    loc = c["reason"] == LOCAL
    print({f"local nt={v}": both(loc, c["nt"], v) for v in (30, 31, 32)},
          {f"global by nt={v}": both(c["reason"] == BY_TMAX, c["nt"], v) for v in (33, 34, 35)},
          "reasons", dict(zip(REASONS, np.bincount(c["reason"], minlength=len(REASONS)).tolist())))
    assert int(c["kt"].max()) <= 8 and int(c["kx"].max()) <= 8
    assert both(loc, c["nt"], 32) >= 2 and both(c["reason"] == BY_TMAX, c["nt"], 33) >= 2
    assert int(c["nt"][loc].max()) == 32


def test_threads_fixture_sits_on_both_sides_of_the_staging_limit():
    g, cfg, exp, c = census("edge_threads_sat1.1")
    print({f"staging={v}": count(c["staging"], v) for v in (62, 63, 64, 65, 66)},
          "local at 64", both(c["reason"] == LOCAL, c["staging"], 64), "global only by 65",
          both(c["reason"] == BY_PLC, c["staging"], 65))
    for v in (64, 65):  # PLC
        assert count(c["staging"], v) >= 100, (v, count(c["staging"], v))
    assert both(c["reason"] == LOCAL, c["staging"], 64) >= 100 and both(c["reason"] == BY_PLC, c["staging"], 65) >= 100


def test_restr_wide_fixture_has_rows_on_both_sides_of_the_candidate_limit():
    g, cfg, exp, c = census("edge_restr_wide_sat1.1")
    width = np.diff(g["restr_ptr"])[(g["restr_flags"] & 1) != 0]
    print({f"width={v}": count(width, v) for v in (7, 8, 9, 10)}, "max", int(width.max()))
    for v in (8, 9):  # RC_MAX
        assert count(width, v) >= 20, (v, count(width, v))


@pytest.mark.parametrize("name", ROUND_ENGINE)
def test_round_engine_fixtures_pass_the_prefix_limit_within_the_worker_cap(name):
    g, cfg, exp, c = census(name)
    P = len(g["prefix_default_dur"])
    used = len(np.unique(g["prefix_id"]))
    held = max_worker_prefixes(g, exp)
    print(name, "prefixes", P, "used", used, "most per worker over two rounds", held, "max nt", int(c["nt_all"].max()))
    assert P > 32 and used == P
    assert held <= 8  # PMAX, the engines' documented per-worker cap: not under test
    if name == "edge_p64_sat1.1":
        assert P == 64  # PMAX_G
    if name == "edge_p40_mixed_sat1.1":
        assert int(c["nt_all"].max()) > 24  # TOUCH_MAX
    if name == "edge_p40_w1100_sat1.1":
        assert len(g["nthreads"]) > 1024  # LDS_WORKERS_MAX
    if name == "edge_p40_restr_sat1.1":
        assert int(np.diff(g["restr_ptr"]).max()) == 12


def test_p40_mixed_refills_a_worker_past_its_needs_line():
    """The stimulus shape that found a wrong network occupancy in the round engine's local
    commit: a completion on worker w readies a task that goes to w itself, needs more remote
    dependencies than a needs_what line holds (31, so w turns to exact scans while the
    completing task still counts as processing there) and shares remote dependencies with
    the completing task. The fixture must keep having such stimuli."""
    g, cfg, exp, c = census("edge_p40_mixed_sat1.1")
    ptr, idx = g["dep_ptr"], g["dep_idx"]
    pt, pw = exp["pl_task"], exp["pl_worker"]
    run = np.empty(g["n_tasks"], np.int64)
    run[pt] = np.arange(len(pt))
    holder = np.empty(g["n_tasks"], np.int64)
    holder[pt] = pw
    hits = 0
    for x, w in zip(pt.tolist(), pw.tolist()):
        deps = idx[ptr[x]:ptr[x + 1]]
        if len(deps) < 32:
            continue
        t = int(pt[run[deps].max()])  # the completion that readied x
        remote = set(deps[holder[deps] != w].tolist())
        if holder[t] == w and len(remote) > 31 and remote & set(idx[ptr[t]:ptr[t + 1]].tolist()):
            hits += 1
    print("refills past the needs line with shared dependencies:", hits)
    assert hits >= 5


def test_scan_refill_fixture_refills_scanning_workers_in_local_mode():
    """The same shape on the stream engine, whose needs_what tables hold 63 entries: local
    stimuli on workers that have passed them, among them ones that place a ready task back on
    the completing worker with a dependency it shares with the completing task alone."""
    g, cfg, exp, meta = oracle.load_fixture(os.path.join(GOLDEN, "edge_scan_refill_sat1.1.npz"))
    refills, scanning = scan_mode_refills(g, exp, cfg["saturation"], 63)
    print("refills", refills, "local stimuli on a scanning worker", scanning)
    assert len(g["prefix_default_dur"]) <= 32
    assert refills >= 10 and scanning >= 1000


def test_p32_is_the_last_stream_engine_count():
    g, cfg, exp, c = census("edge_p32_sat1.1")
    assert len(g["prefix_default_dur"]) == 32 == len(np.unique(g["prefix_id"]))
    assert max_worker_prefixes(g, exp) <= 8

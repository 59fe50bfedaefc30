"""Aimed WorkStealing.balance() problems, each with the kernel paths it must reach.

``CASES`` maps a name to a builder of a problem dict for ``PlacementEngine.steal_balance`` /
``oracle.steal_balance`` (W <= 256, T <= 4000; ``problem(name)`` builds it at its first use),
a dict ``site -> minimum count`` over ``steal_census.SITES`` (tests/test_steal_census.py
checks it on the CPU), and whether the GPU test also runs the sliced path on it. The floors are
conditions on the inputs, stated before anything runs on the device: a case that misses
one is changed, not its floor.

No import of the census here: tests/test_gpu_steal_edges.py uses the problems alone.
"""
from __future__ import annotations

import functools

import numpy as np

from distributed_amd import graphs
from oracle import oracle


def _flags(p):
    """total_occ and the idle / saturated sets from the per-worker arrays
    (check_idle_saturated, scheduler.py:2949-2995), as graphs.steal_problem states them."""
    occ, nth, nproc = p["occ"], p["nthreads"], p["nproc"]
    p["total_occ"] = float(occ.sum())
    p["total_nthreads"] = int(nth.sum())
    avg = p["total_occ"] / p["total_nthreads"]
    p["idle"] = ((nproc < nth) | (occ < nth * avg / 2)).astype(np.uint8)
    pend = np.where(nproc > nth, occ * (nproc - nth) / np.maximum(nproc * nth, 1), 0.0)
    p["sat"] = ((p["idle"] == 0) & (nproc > nth) & (pend > 0.4) & (pend > 1.9 * avg)).astype(np.uint8)
    return p


def warm_cold_workers(p, step, kmax, seed):
    """Every worker without a task gets one (not stealable: a fast prefix, no dependency) and
    the occupancy k * step, k uniform in 1..kmax: the thieves of ``p`` then fall into many
    runs of equal stack time, ``step`` apart."""
    rng = np.random.default_rng(seed)
    cold = np.flatnonzero(p["nproc"] == 0)
    k = rng.integers(1, kmax + 1, len(cold))
    p = dict(p)
    p["occ"] = p["occ"].copy()
    p["occ"][cold] = k * step
    p["nproc"] = p["nproc"].copy()
    p["nproc"][cold] = 1
    p["victim"] = np.concatenate([p["victim"], cold.astype(np.int32)])
    p["duration"] = np.concatenate([p["duration"], k * step])
    p["fast"] = np.concatenate([p["fast"], np.ones(len(cold), np.uint8)])
    p["dep_ptr"] = np.concatenate([p["dep_ptr"], np.full(len(cold), p["dep_ptr"][-1], np.int64)])
    if p.get("restr_flags") is not None:
        p["restr_flags"] = np.concatenate([p["restr_flags"], np.zeros(len(cold), np.uint8)])
        p["restr_ptr"] = np.concatenate([p["restr_ptr"], np.full(len(cold), p["restr_ptr"][-1], np.int64)])
    return _flags(p)


def busy_runs():
    """More than 64 runs among the thieves, dependencies on up to 5 workers: the run-ordered
    search far from "first live thief of the zero run", rows of every holder count."""
    p = graphs.steal_problem(200, 3800, seed=101, replicas=5)
    return warm_cold_workers(p, 0.01, 400, 102)


def busy_restricted():
    p = graphs.steal_problem(160, 3500, seed=111, restrict=0.8, replicas=2, hot_frac=0.3)
    return warm_cold_workers(p, 0.01, 300, 112)


def shared_runs():
    """Few stack times shared by many thieves and half of the data empty (0 bytes): a
    holder of an empty dependency starts when the non-holders of its run do, and
    (ws.nbytes, index) decides between them."""
    p = graphs.steal_problem(128, 3000, seed=121, replicas=3)
    p["data_nbytes"] = p["data_nbytes"].copy()
    p["data_nbytes"][np.random.default_rng(122).random(len(p["data_nbytes"])) < 0.5] = 0
    p["data_get_nbytes"] = p["data_nbytes"]
    p["wnbytes"] = np.bincount(p["holder_idx"], weights=np.repeat(p["data_nbytes"], np.diff(p["holder_ptr"])),
                               minlength=128).astype(np.int64)
    return warm_cold_workers(p, 0.01, 4, 123)


def rounding(W, T, step, seed, thieves_hold_nothing=False):
    """Starts that tie across runs only because ``ra + x`` rounds: 1.28 s tasks, every seventh
    datum 3e10 bytes (x = 300 s at 1e8 B/s, half an ulp is 2.8e-14 s; two of them put a task
    past the last level), stack times ``step / 2`` apart. With ``step`` 1e-14 a handful of
    runs tie; with 2.4e-16 on 200 workers more than half of some 140 do, and a search walks
    past the 64 runs whose stack times it keeps in registers. ``thieves_hold_nothing``: every
    datum lies on a worker with tasks, so all thieves have ws.nbytes 0 and a tie of starts
    across runs falls to the worker index, which a later run may win."""
    p = graphs.steal_problem(W, T, seed=seed)
    if thieves_hold_nothing:
        hot = np.unique(p["victim"])
        p["data_holder"] = hot[p["data_holder"] % len(hot)].astype(np.int32)
    p["duration"] = np.full_like(p["duration"], 1.28)
    nb = p["data_nbytes"].copy()
    nb[::7] = 30_000_000_000
    p["data_nbytes"] = p["data_get_nbytes"] = nb
    p["wnbytes"] = np.bincount(p["data_holder"], weights=nb, minlength=W).astype(np.int64)
    occ = np.zeros(W)  # as graphs.steal_problem: durations + each remote dependency once per worker
    np.add.at(occ, p["victim"], p["duration"])
    seen = set()
    for t in range(len(p["victim"])):
        v = int(p["victim"][t])
        for d in p["dep_idx"][p["dep_ptr"][t]:p["dep_ptr"][t + 1]]:
            if p["data_holder"][d] != v and (v, int(d)) not in seen:
                seen.add((v, int(d)))
                occ[v] += nb[d] / p["bandwidth"]
    p["occ"] = occ
    return warm_cold_workers(_flags(p), step, 400, seed + 1)


def saturated_exactly(n):
    """Exactly ``n`` saturated workers (19: the sorted list; 20: the live set), busy thieves."""
    p = graphs.steal_problem(200, 3800, seed=151, hot_frac=0.2, zipf_a=1.1)
    p = warm_cold_workers(p, 0.01, 200, 152)
    # the n most loaded workers that are not idle (the set is the scheduler's as it stood at
    # their last check, so any such subset is a legal input)
    busy = np.flatnonzero((p["idle"] == 0) & (p["nproc"] > p["nthreads"]))
    assert len(busy) >= n, len(busy)
    p["sat"] = np.zeros_like(p["sat"])
    p["sat"][busy[np.argsort(-p["occ"][busy], kind="stable")[:n]]] = 1
    return p


def plugin_state():
    """The plugin's own state as input: bins with tasks taken out, in-flight accounts of both
    signs, three victims whose combined occupancy is below zero at their check."""
    p = graphs.steal_problem(160, 3500, seed=161, restrict=0.1)
    p = warm_cold_workers(p, 0.01, 300, 162)
    rng = np.random.default_rng(163)
    W, T = 160, len(p["victim"])
    lv = oracle.steal_balance(p)["level"].copy()  # the bins as the plugin would hold them
    lv[rng.random(T) < 0.2] = -1
    p["level_in"] = lv
    p["inflight_occ_in"] = np.where(rng.random(W) < 0.3, rng.normal(0, 0.5, W), 0.0)
    p["inflight_tasks_in"] = rng.integers(-2, 3, W).astype(np.int32)
    for v in np.flatnonzero(p["sat"])[:3]:
        p["inflight_occ_in"][v] = -p["occ"][v] - 1.0
    return p


def _hand(W, nth, occ, nproc, idle, sat, tasks, avg, data=(), level_in=True):
    """A problem from explicit rows. ``tasks``: (victim, level, duration, [data ids]);
    ``data``: (nbytes, holder). The bins are given as ``level_in``."""
    T = len(tasks)
    dep_ptr = np.zeros(T + 1, np.int64)
    dep_ptr[1:] = np.cumsum([len(t[3]) for t in tasks])
    data = list(data) or [(0, 0)]
    nb = np.array([d[0] for d in data], np.int64)
    hold = np.array([d[1] for d in data], np.int32)
    nth = np.asarray(nth, np.int32)
    return dict(nthreads=nth, occ=np.asarray(occ, np.float64), nproc=np.asarray(nproc, np.int32),
                wnbytes=np.bincount(hold, weights=nb, minlength=W).astype(np.int64),
                idle=np.asarray(idle, np.uint8), sat=np.asarray(sat, np.uint8),
                total_occ=float(avg) * int(nth.sum()), total_nthreads=int(nth.sum()), bandwidth=100_000_000,
                victim=np.array([t[0] for t in tasks], np.int32), duration=np.array([t[2] for t in tasks], np.float64),
                fast=np.zeros(T, np.uint8), dep_ptr=dep_ptr,
                dep_idx=np.array([d for t in tasks for d in t[3]], np.int32), data_nbytes=nb, data_get_nbytes=nb,
                data_holder=hold, level_in=np.array([t[1] for t in tasks], np.int8))


def exact_bins():
    """Bins of exactly 1, 63, 64, 65, 128 and 129 tasks, each size on six victims of equal
    occupancy (at another level on each); thieves of 65 threads with one task each: a chunk's
    64 tasks all go to one thief, whose 64th fills it at lane 63 (the accepted prefix reaches
    the chunk's end while the thief repeats)."""
    V, N = 6, 50
    W = V + N + 2
    nth = [2] * V + [65] * N + [1, 65535]
    occ = [5000.0] * V + [0.001 * k for k in range(1, N + 1)] + [0.5, 6553.5]
    nproc = [2000] * V + [1] * (N + 2)
    idle = [0] * V + [1] * (N + 2)
    sat = [1] * V + [0] * (N + 2)
    sizes = (1, 63, 64, 65, 128, 129)
    tasks = []
    for v in range(V):
        for lv in range(len(sizes)):
            tasks += [(v, lv, 0.5, [])] * sizes[(lv + v) % len(sizes)]
    return _hand(W, nth, occ, nproc, idle, sat, tasks, avg=0.01)


def fill_then_reject():
    """One-thread thieves that one task fills, each followed by a task too long to move: the
    rejection falls on the lane right after the fill, first with the filled thief as that
    lane's own (no dependency: every task's first choice is the least stack time), then
    with another thief (a dependency that thief holds)."""
    W = 60
    nth = [2] + [1] * 59
    occ = [400.0] + [0.01 * k for k in range(1, 60)]
    nproc = [300] + [0] * 59
    idle = [0] + [1] * 59
    sat = [1] + [0] * 59
    data = [(5_000_000_000, 50 + k) for k in range(10)]  # held by the thieves 50..59
    tasks = []
    for k in range(10):
        tasks += [(0, 0, 1.0, []), (0, 0, 1000.0, []), (0, 0, 1.0, []), (0, 0, 1000.0, [k])]
    tasks += [(0, 1, 1.0, [])] * 45  # a second bin: the last thieves fill in mid-chunk
    return _hand(W, nth, occ, nproc, idle, sat, tasks, avg=1.0, data=data)


def topk_small():
    """None saturated on 8 workers: topk(10) of fewer than 10, seven victims of one combined
    occupancy (ties in the topk and in the stable sort)."""
    W = 8
    occ = [50.0] * 7 + [0.01]
    tasks = []
    for v in range(7):
        tasks += [(v, 0, 0.5, [])] * 10 + [(v, 2, 0.5, [v])] * 5
    data = [(1000, 7) for v in range(7)]
    return _hand(W, [2] * W, occ, [15] * 7 + [1], [0] * 7 + [1], [0] * W, tasks, avg=20.0, data=data)


def topk_ties():
    """None saturated on 16 workers: pairs of equal combined occupancy in the topk and in the
    stable sort of the victims; nthreads from 1 to 65535."""
    W = 16
    occ = [50.0] * 4 + [40.0] * 4 + [0.01 * (k % 4) for k in range(8)]
    nth = [1, 2, 2, 4, 2, 2, 1, 2] + [1, 64, 4, 64, 65535, 1, 128, 2]
    tasks = []
    for v in range(8):
        tasks += [(v, 0, 0.5, [])] * 12 + [(v, 3, 0.25, [v])] * 6
    data = [(4096, 8 + v) for v in range(8)]
    return _hand(W, nth, occ, [18] * 8 + [1] * 8, [0] * 8 + [1] * 8, [0] * W, tasks, avg=0.5, data=data)


ANY3 = 3  # "reached" for a site the issue sets no figure for

# name -> (builder, floors, also through the sliced path)
CASES = {
    "busy_runs": (busy_runs, {
        "search.live_runs_gt64": 100, "rows.nh3": 20, "rows.nh4": 20, "rows.many": 20, "rows.nh0": ANY3,
        "rows.nh1": ANY3, "rows.nh2": ANY3, "search.holder_at_min_start": 20, "search.holder_wins": ANY3,
        "search.winner_not_first_run": ANY3, "search.crossed_empty_run": ANY3, "search.first_run_changed": ANY3,
        "search.batched": ANY3, "search.again": ANY3, "search.holder_first_of_run": ANY3, "win.repeat": ANY3,
        "win.prefix_splits_repeat": ANY3, "win.fill_repeats_later": ANY3}, True),
    "busy_restricted": (busy_restricted, {
        "restr.valid": ANY3, "restr.none_loose": ANY3, "restr.none_strict": ANY3, "search.live_runs_gt64": 100}, True),
    "shared_runs": (shared_runs, {
        "search.tie_in_run": ANY3, "search.holder_tie_wins": ANY3, "search.holder_tie_loses": ANY3,
        "search.holder_at_min_start": 20}, True),
    "rounding": (lambda: rounding(96, 3000, 1e-14, 131), {"search.tie_across_runs": 10, "win.reject_lane0": ANY3},
                 False),
    "deep_ties": (lambda: rounding(200, 3800, 2.4e-16, 141), {"search.past_window": ANY3,
                                                             "search.tie_across_runs": 10}, False),
    "index_ties": (lambda: rounding(96, 3000, 1e-14, 171, thieves_hold_nothing=True),
                   {"search.tie_across_runs_by_index": ANY3, "search.tie_across_runs": 10}, False),
    "sat19": (lambda: saturated_exactly(19), {"vict.nsat19": 1, "search.live_runs_gt64": 100}, False),
    "sat20": (lambda: saturated_exactly(20), {"vict.nsat20": 1, "vict.live_left_sat": ANY3}, False),
    "plugin_state": (plugin_state, {"in.level_in_neg": ANY3, "in.inflight_in": ANY3, "vict.occ_negative": ANY3},
                     False),
    "exact_bins": (exact_bins, {
        "bin.size1": ANY3, "bin.size63": ANY3, "bin.size64": ANY3, "bin.size65": ANY3, "bin.size128": ANY3,
        "bin.size129": ANY3, "chunk.prefix_to_lane63_with_repeat": ANY3, "vict.sort_tie": ANY3,
        "in.nthreads_mixed": ANY3}, False),
    "fill_then_reject": (fill_then_reject, {
        "win.reject_after_fill_same": ANY3, "win.reject_after_fill_other": ANY3, "win.reject_lane0": ANY3,
        "win.thieves_exhausted_midchunk": 1}, False),
    "topk_small": (topk_small, {"vict.topk_w_lt10": 1, "vict.topk_tie": ANY3, "vict.sort_tie": ANY3}, False),
    "topk_ties": (topk_ties, {"vict.topk_w_ge10": 1, "vict.topk_tie": ANY3, "vict.sort_tie": ANY3,
                              "in.nthreads_mixed": ANY3}, False),
}
NAMES = tuple(CASES)
SLICED = tuple(n for n in NAMES if CASES[n][2])


def floors(name):
    return CASES[name][1]


@functools.lru_cache(maxsize=None)
def problem(name):
    """The problem of one case, built at its first use (nothing is built at import)."""
    return CASES[name][0]()

"""The bulk path of dgp_release_tasks (needs an MI355X): the parallel kernels of
distributed_amd/csrc/dgp_release.h against the serial kernel they stand in for and against
the reference.

* every ``svcbulk_*`` stream (tests/golden/bulk/, gen_bulk_release.py: the reference's own
  client_releases_keys with many keys per call) on either path, and every ``svcrel_*`` /
  ``svccan_*`` stream (plans of one to a few tasks: the degenerate grids): bit-exact with the
  reference, the state audit clean after each release; the ``svcbulk_skew_*`` streams also
  carry every worker's idle / saturated flags after each call, from plans whose workers'
  flags depend on the place in the plan at which check_idle_saturated reads the total;
* twins: two engines advanced alike on small random graphs, the same synthetic plan applied by
  the serial kernel on one and the bulk kernels on the other; everything the state audit can
  see, the refill's placements and the rest of the replay are equal;
* twins on plans made so that the flags depend on that place (counted from the engines' own
  snapshot), and on graphs of up to 32 prefixes;
* a worker in needs_what scan mode: the bulk path runs when no result is listed before a
  cancelled dependent, and leaves the plan to the serial kernel when one is;
* one cancelled graph of 120k tasks on 256 workers, bulk only (the serial kernel would search
  the queue once per queued task).
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN, svc_release_files
from oracle import oracle
from test_gpu_events import EV_RELEASE_KEYS, drive_events
from test_gpu_parity import PL_KEYS, ROUND_KEYS, assert_same

pytestmark = pytest.mark.gpu

SERIAL, BULK = 1, 2
CFG = {"bandwidth": 100_000_000, "default_data_size": 1024, "unknown_duration": 0.5}
S_RELEASED, S_WAITING, S_PROCESSING, S_QUEUED, S_NO_WORKER, S_MEMORY = range(6)


def worker_flags(eng):
    """(idle, saturated) of every worker: a dry run of sync_workers with all-zero rows reports
    each flags byte that is not a running worker's with neither flag set."""
    W, z = eng.n_workers, np.zeros
    rows = eng.audit_rows(workers=dict(
        status=z(W, np.int8), nproc=z(W, np.int32), n_long_running=z(W, np.int32), plen=z(W, np.int32),
        prefix=z(W * 8, np.int32), count=z(W * 8, np.int32), netocc=z(W, np.int64), nbytes=z(W, np.int64),
        idle=z(W, np.uint8), saturated=z(W, np.uint8), needs_ptr=z(W + 1, np.int64), needs_task=z(1, np.int32),
        needs_count=z(1, np.int32)), cap=80 * W + 4096)
    assert len(rows) == rows.total
    fl = np.zeros(W, np.uint8)
    for v in rows:
        if v.field == "flags":
            fl[v.index] = v.device_value
    return fl & 1, (fl >> 1) & 1


class Watched:
    """An engine whose release_tasks notes the path each plan took and audits the state;
    with ``flags`` (per call: every worker's idle and saturated flag in the reference after
    it) it compares the engine's flags after each call as well."""

    def __init__(self, eng, flags=None):
        self._e = eng
        self.paths = []
        self.flags = flags

    def __getattr__(self, k):
        return getattr(self._e, k)

    def release_tasks(self, task, forget):
        r = self._e.release_tasks(task, forget)
        if r is not None and len(task):
            self.paths.append((len(task), self._e.last_release_path))
            v, _ = self._e.audit_state()
            assert not v, (len(self.paths), v[:5])
            if self.flags is not None:
                k = len(self.paths) - 1
                idle, sat = worker_flags(self._e)
                assert np.array_equal(idle, self.flags[0][k]), ("idle after call", k, idle, self.flags[0][k])
                assert np.array_equal(sat, self.flags[1][k]), ("saturated after call", k, sat, self.flags[1][k])
        return r


@pytest.mark.parametrize("mode", [SERIAL, BULK], ids=["serial", "bulk"])
@pytest.mark.parametrize("name", svc_release_files())
def test_release_streams_on_either_path(name, mode):
    """svcrel_* / svccan_*: every client release on the device by the path asked for. Every
    placement, snapshot and final state equals the reference's; each plan ran on that path."""
    from distributed_amd.engine import PlacementEngine

    path = os.path.join(GOLDEN, name)
    g, cfg, exp, meta = oracle.load_fixture(path)
    z = np.load(path, allow_pickle=False)
    R = len(exp["round_nplaced"]) + 2
    with PlacementEngine(0) as eng:
        assert eng.last_release_path == 0
        eng.load(g, cfg, snapshots=R, results=False)
        eng.set_release_mode(mode)
        eng.update_graph()
        w = Watched(eng)
        stim = drive_events(w, g, z, exp, device_release=True)
        out = eng.placements()
        out.update(eng.snapshots(R))
        out["final_state"] = eng.task_states()
    assert len(w.paths) == int((z["ev_kind"] == EV_RELEASE_KEYS).sum())
    assert {p for _, p in w.paths} == {mode}, w.paths[:10]
    assert np.array_equal(stim, exp["stim_nplaced"]), np.nonzero(stim != exp["stim_nplaced"])[0][:5]
    assert_same(out, exp, PL_KEYS + ROUND_KEYS)
    assert np.array_equal(out["final_state"], np.where(exp["final_state"] == 7, 0, exp["final_state"]))


def svc_bulk_files():
    """Streams whose client-releases-keys calls name many keys (gen_bulk_release.py)."""
    return sorted(f for f in os.listdir(os.path.join(GOLDEN, "bulk"))
                  if f.startswith("svcbulk_") and f.endswith(".npz"))


def bulk_stream_cases():
    out = [pytest.param(f, mode, "auto", id=f"{f[:-4]}-{'serial' if mode == SERIAL else 'bulk'}")
           for f in svc_bulk_files() for mode in (SERIAL, BULK)]
    # one stream on each stream-window build, forced
    return out + [pytest.param("svcbulk_queue_sat1.1.npz", BULK, 32, id="svcbulk_queue_sat1.1-bulk-w32"),
                  pytest.param("svcbulk_half_c2var_sat1.1.npz", BULK, 64, id="svcbulk_half_c2var_sat1.1-bulk-w64"),
                  pytest.param("svcbulk_skew_wide_satinf.npz", BULK, 64, id="svcbulk_skew_wide_satinf-bulk-w64")]


@pytest.mark.parametrize("name,mode,window", bulk_stream_cases())
def test_bulk_streams_match_reference(name, mode, window):
    """svcbulk_*: the reference's own Scheduler.client_releases_keys with many keys per call
    (half the wanted keys mid-run, every key, a group's keys; 70 workers; restrictions; the
    queue's head, tail, inside and all of it). stim_nplaced, the placement columns, the
    per-round snapshots and the final states equal the reference's on either path (mode 1: a
    wrong fixture shows as such); the audit is clean after each release and, with mode 2,
    every call ran the bulk kernels. One stream also runs on each stream-window build.

    svcbulk_skew_*: the first long call lists a few workers' exits before most of what the
    others process, so those workers' flags are right only with the total as of their last
    exit's place in the plan (tests/test_bulk_release_census.py counts them by flag and by
    term of the total; the wide stream's sums pass 2^32). Their fixtures hold every worker's
    flags after each call (bk_idle / bk_sat), compared here."""
    from distributed_amd.engine import PlacementEngine

    path = os.path.join(GOLDEN, "bulk", name)
    g, cfg, exp, meta = oracle.load_fixture(path)
    z = np.load(path, allow_pickle=False)
    R = len(exp["round_nplaced"]) + 2
    with PlacementEngine(0, window=window) as eng:
        eng.load(g, cfg, snapshots=R, results=False)
        assert window == "auto" or eng.get_window() == window
        eng.set_release_mode(mode)
        eng.update_graph()
        w = Watched(eng, (z["bk_idle"], z["bk_sat"]) if "bk_idle" in z.files else None)
        assert w.flags is not None or "_skew_" not in name
        stim = drive_events(w, g, z, exp, device_release=True)
        out = eng.placements()
        out.update(eng.snapshots(R))
        out["final_state"] = eng.task_states()
    assert [n for n, _ in w.paths] == z["bk_n"].tolist() and max(z["bk_n"]) > 64
    assert {p for _, p in w.paths} == {mode}, w.paths[:10]
    assert np.array_equal(stim, exp["stim_nplaced"]), np.nonzero(stim != exp["stim_nplaced"])[0][:5]
    assert_same(out, exp, PL_KEYS + ROUND_KEYS)
    assert np.array_equal(out["final_state"], np.where(exp["final_state"] == 7, 0, exp["final_state"]))


# ------------------------------------------------------------------------------ twins
def finish_round(engs, g, done, skip=()):
    """Complete, on every engine alike, the placements from ``done`` on whose task still runs."""
    n = engs[0].num_placements()
    assert all(e.num_placements() == n for e in engs)
    if n == done:
        return n
    p = engs[0].placements(done, n - done, columns=("pl_task", "pl_worker"))
    st = engs[0].task_states()
    t, w, r = p["pl_task"], p["pl_worker"], np.arange(done, n, dtype=np.int32)
    keep = st[t] == S_PROCESSING
    if len(skip):
        keep &= ~np.isin(t, skip)
    t, w, r = t[keep], w[keep], r[keep]
    for e in engs:
        if len(t):
            s, _ = e.tasks_finished(t, w, r, g["nbytes"][t], g["start"][t], g["stop"][t])
            assert (s == 0).all()
        e.snapshot()
    return n


def state_dump(eng, g):
    """Everything the row audits compare, as the differences from an all-zero state."""
    N, W, P, G = g["n_tasks"], eng.n_workers, len(g["prefix_default_dur"]), len(g["group_prefix"])
    z = np.zeros
    tasks = dict(task=np.arange(N, dtype=np.int32), state=z(N, np.uint8), remaining=z(N, np.int32),
                 waiters=z(N, np.int32), processing_on=z(N, np.int32), nbytes=z(N, np.int64),
                 long_running=z(N, np.uint8), wanted=z(N, np.uint8), holder_ptr=z(N + 1, np.int64),
                 holder_idx=z(1, np.int32))
    workers = dict(status=z(W, np.int8), nproc=z(W, np.int32), n_long_running=z(W, np.int32), plen=z(W, np.int32),
                   prefix=z(W * 8, np.int32), count=z(W * 8, np.int32), netocc=z(W, np.int64), nbytes=z(W, np.int64),
                   idle=z(W, np.uint8), saturated=z(W, np.uint8), needs_ptr=z(W + 1, np.int64),
                   needs_task=z(1, np.int32), needs_count=z(1, np.int32))
    glob = dict(n_tasks=0, network_occ_global=0.0, g_prefix=z(0, np.int32), g_count=z(0, np.int64),
                queued=z(0, np.int32), duration_average=z(P), max_exec_time=z(P), bandwidth=1.0,
                group_released_waiting=z(G, np.int64), group_left=z(G, np.int64), group_last_worker=z(G, np.int32))
    return [tuple(v) for v in eng.audit_rows(tasks, workers, glob, cap=40 * N + 64 * W + 4096)]


def synthetic_plan(g, rng, frac):
    """A dependents-closed subset in reverse topological order with shuffled ties, forget flags
    on an upward-closed part of it (the sink side)."""
    N = g["n_tasks"]
    dp, di = g["dep_ptr"], g["dep_idx"]
    inplan = rng.random(N) < frac
    forget = inplan & (rng.random(N) < 0.3)
    level = np.zeros(N, np.int64)
    for t in range(N):  # dependencies have lower indices
        d = di[dp[t]:dp[t + 1]]
        if len(d):
            inplan[t] |= inplan[d].any()
            level[t] = level[d].max() + 1
    for t in range(N):  # forgotten: every dependent forgotten too
        d = di[dp[t]:dp[t + 1]]
        if len(d) and forget[d].any():
            forget[t] = True
    forget &= inplan
    ts = np.flatnonzero(inplan)
    order = np.lexsort((rng.random(len(ts)), -level[ts]))
    ts = ts[order].astype(np.int32)
    return ts, forget[ts].astype(np.uint8)


def twin_cases():
    rng = np.random.default_rng(2024)
    out = []
    for i in range(30):
        n = int(rng.integers(300, 2001))
        w = [5, 17, 64, 65, 70, 33][i % 6]
        sat = 1.1 if i % 3 else float("inf")
        k = 1 + i % 8
        rounds = [0, 1, 2, 4, 8][i % 5]
        frac = [0.02, 0.2, 1.0][i % 3 if i % 7 else 2]
        out.append(pytest.param(n, w, sat, k, rounds, frac, i, id=f"n{n}-w{w}-sat{sat}-p{k}-r{rounds}-f{frac}"))
    # past the 8 prefixes a worker's own dict holds, up to the stream engine's 32: k_rb_flags'
    # and k_rb_globals' per-prefix tables and the duration rows at prefix ids above 8. At
    # saturation 1.1 a worker of 1-4 threads runs at most 5 tasks, so at most 5 prefixes
    out.append(pytest.param(1200, 17, 1.1, 20, 4, 1.0, 31, id="n1200-w17-sat1.1-p20-r4-f1.0"))
    out.append(pytest.param(900, 33, 1.1, 31, 2, 0.2, 33, id="n900-w33-sat1.1-p31-r2-f0.2"))
    return out


def flags_with_total(occ, nproc, nthreads, total):
    """check_idle_saturated's idle / saturated (scheduler.py:2949-3004) of running workers
    with ``total`` for SchedulerState.total_occupancy."""
    avg = total / nthreads.sum()
    idle = (nproc < nthreads) | (occ < nthreads * avg / 2)
    pending = occ * (nproc - nthreads) / np.maximum(nproc * nthreads, 1)
    sat = ~idle & (nproc > nthreads) & (pending > 0.4) & (pending > 1.9 * avg)
    return idle, sat


def place_sensitive(eng, g, exits, R):
    """Of the workers in ``exits`` (each lost a processing task to the release just made, no
    worker is paused), those whose flags differ from check_idle_saturated restated with the
    total occupancy the call left: the engine's last snapshot has every worker's occupancy,
    whose sum is that total up to rounding, so a worker counts only when a total 1e-9 to
    either side gives the same restated flags."""
    s = eng.snapshots(R)
    occ, nproc = s["round_occ"][-1], s["round_nproc"][-1].astype(np.int64)
    have = s["round_idle"][-1].astype(bool), s["round_sat"][-1].astype(bool)
    nth = np.asarray(g["nthreads"], np.int64)
    differs = np.ones(len(nth), bool)
    for total in (occ.sum() * (1 - 1e-9), occ.sum() * (1 + 1e-9)):
        idle, sat = flags_with_total(occ, nproc, nth, total)
        differs &= (idle != have[0]) | (sat != have[1])
    return np.flatnonzero(differs & np.isin(np.arange(len(nth)), exits))


def run_twins(g, cfg, rounds, plan, forget, expect_path=BULK, until_scan=False, audit=True, info=None):
    """``info``: a dict that receives ``sensitive``, per engine the workers that lost a
    processing task and whose flags depend on where in the plan the total is read."""
    from distributed_amd.engine import PlacementEngine

    R = 400
    with PlacementEngine(0) as a, PlacementEngine(0) as b:
        engs = (a, b)
        for e, mode in ((a, SERIAL), (b, BULK)):
            e.load(g, cfg, snapshots=R, results=False)
            e.set_release_mode(mode)
            e.update_graph()
        done = 0
        for k in range(rounds):
            done = finish_round(engs, g, done)
            if until_scan and a.audit_state()[1] > 0:
                break
        if until_scan:  # a worker past its needs_what line (scan mode) is what the case is about
            assert a.audit_state()[1] > 0
        if callable(plan):
            plan, forget = plan(a.task_states(), a)
        kinds = np.bincount(a.task_states()[plan], minlength=6)
        if info is not None:  # the workers the plan's processing tasks run on
            p = a.placements(columns=("pl_task", "pl_worker"))
            on = np.full(g["n_tasks"], -1, np.int64)
            on[p["pl_task"]] = p["pl_worker"]  # a task placed again: its last placement
            exits = np.unique(on[plan[a.task_states()[plan] == S_PROCESSING]])
        pa, pb = a.release_tasks(plan, forget), b.release_tasks(plan, forget)
        assert pa is not None and pb is not None, (a.refusal, b.refusal)
        assert (a.last_release_path, b.last_release_path) == (SERIAL, expect_path)
        assert pa == pb
        for e in engs if audit else ():
            v, _ = e.audit_state()
            assert not v, v[:5]
        assert np.array_equal(a.task_states(), b.task_states())
        assert a.num_unrunnable() == b.num_unrunnable()
        da, db = state_dump(a, g), state_dump(b, g)
        assert da == db, [x for x in zip(da, db) if x[0] != x[1]][:5]
        for e in engs:
            e.snapshot()
        if info is not None:
            info["sensitive"] = [place_sensitive(e, g, exits, R).tolist() for e in engs]
        for k in range(R - rounds - 3):  # the rest of the replay, from the state the release left
            n = finish_round(engs, g, done, skip=plan)
            if n == done:
                break
            done = n
        oa, ob = a.placements(), b.placements()
        oa.update(a.snapshots(R))
        ob.update(b.snapshots(R))
        assert_same(ob, oa, PL_KEYS + ROUND_KEYS)
        assert np.array_equal(a.task_states(), b.task_states())
    return kinds


@pytest.mark.parametrize("n,w,sat,k,rounds,frac,seed", twin_cases())
def test_twin_engines_serial_and_bulk(n, w, sat, k, rounds, frac, seed):
    from distributed_amd import graphs

    # every other graph is mostly roots, so that at saturation 1.1 a long queue stands
    g = graphs.random_dag(n, w, seed=100 + seed, n_inner_prefixes=k, random_durations=True,
                          nthreads="random" if seed % 2 else 1, root_frac=0.1 if seed % 2 else 0.6)
    if seed % 5 == 0:  # worker restrictions, some with no valid worker: no-worker tasks, the 64-slot build
        g = graphs.restrict(g, 0.2, seed=seed)
    plan, forget = synthetic_plan(g, np.random.default_rng(seed), frac)
    info = {}
    kinds = run_twins(g, dict(CFG, saturation=sat), rounds, plan, forget, info=info)
    print("plan", len(plan), "entry states (released, waiting, processing, queued, no-worker, memory)", kinds.tolist(),
          "workers whose flags depend on the place of the total", [len(x) for x in info["sensitive"]])
    assert info["sensitive"][0] == info["sensitive"][1]


def skewed_plan(g, rng, st, eng, n_spare=3, share=0.8):
    """The svcbulk_skew_* plan on a synthetic state: one processing task of each of a few
    workers first, then most of the other workers' processing tasks, then every result in
    memory all of whose dependents the plan cancels (released when its last waiter left)."""
    p = eng.placements(columns=("pl_task", "pl_worker"))
    on = np.full(g["n_tasks"], -1, np.int64)
    on[p["pl_task"]] = p["pl_worker"]
    proc = np.flatnonzero(st == S_PROCESSING)
    spare = rng.choice(np.unique(on[proc]), n_spare, replace=False)
    first = [rng.choice(proc[on[proc] == w]) for w in spare]
    rest = proc[~np.isin(on[proc], spare) & (rng.random(len(proc)) < share)]
    rng.shuffle(rest)
    cancelled = np.zeros(g["n_tasks"], bool)
    cancelled[first] = cancelled[rest] = True
    left = np.zeros(g["n_tasks"], np.int64)  # dependents the plan leaves
    dp, di = g["dep_ptr"], g["dep_idx"]
    for t in np.flatnonzero(~cancelled & (st != S_RELEASED) & (st != S_MEMORY)):
        left[di[dp[t]:dp[t + 1]]] += 1
    mem = np.flatnonzero((st == S_MEMORY) & (left == 0) & (np.bincount(di, minlength=g["n_tasks"]) > 0))
    plan = np.concatenate([first, rest, mem]).astype(np.int32)
    return plan, (rng.random(len(plan)) < 0.3).astype(np.uint8) & cancelled[plan]


@pytest.mark.parametrize("fetches", [False, True], ids=["counts", "fetches"])
def test_twins_on_a_plan_whose_flags_depend_on_the_place_of_the_total(fetches):
    """Saturation inf, every task of the plan processing. ``counts``: 600 tasks without
    dependencies on 10 workers right after update_graph, so no exit frees a byte and only the
    prefix counts move the total. ``fetches``: two layers of 300, the first in memory, the
    second processing on 24 workers with dependencies of several GB on other workers, so the freed bytes
    (sums past 2^32) move it, and the results nobody waits for any more go with the plan.
    Some exiting worker's flags differ, on both engines, from check_idle_saturated restated
    with the total the call left (so a kernel that read the total there would fail here),
    and the twins agree on everything run_twins compares."""
    from distributed_amd import graphs

    if fetches:
        # 24 workers, 2 or 3 dependencies: no worker needs more results than its needs_what line holds
        g = graphs.widen(graphs.layered_dag(2, 300, 24, seed=71, fanins=(2, 3), n_inner_prefixes=3,
                                            random_durations=True, nthreads="random"), 71)
    else:
        g = graphs.random_dag(600, 10, seed=70, root_frac=1.0, random_durations=True, nthreads="random")
    rng = np.random.default_rng(70)
    info = {}
    kinds = run_twins(g, dict(CFG, saturation=float("inf")), 1 if fetches else 0,
                      lambda st, eng: skewed_plan(g, rng, st, eng), None, info=info)
    print("entry states", kinds.tolist(), "workers whose flags depend on the place of the total", info["sensitive"])
    assert kinds[S_PROCESSING] > 64 and (kinds[S_MEMORY] > 0) == fetches
    assert info["sensitive"][0] == info["sensitive"][1] and len(info["sensitive"][0]) >= 1


def mixed_graph():
    from distributed_amd import graphs

    # three workers, layers of 200 tasks with 7 or 8 dependencies: each worker needs more
    # dependencies at once than its needs_what line and overflow hold
    return graphs.layered_dag(15, 200, 3, seed=400, fanins=(7, 8), span=2, n_inner_prefixes=3,
                              random_durations=True, nthreads="random")


def test_scan_mode_worker_on_the_bulk_path():
    """A worker whose needs_what left its line (scan mode), every task released in reverse
    topological order: no result is listed before a dependent, so the bulk path runs and its
    scan-mode exits read replicas that are still there, as the serial kernel's do."""
    g = mixed_graph()

    def plan(st, eng):
        ts = np.arange(g["n_tasks"] - 1, -1, -1, dtype=np.int32)
        return ts, np.zeros(len(ts), np.uint8)

    kinds = run_twins(g, dict(CFG, saturation=1.1), 200, plan, None, expect_path=BULK, until_scan=True)
    assert kinds[S_PROCESSING] > 0 and kinds[S_MEMORY] > 0, kinds


def test_result_listed_before_its_scan_mode_dependent_takes_the_serial_path():
    """The same state with the results listed first: a memory release precedes a cancelled
    dependent processing on a scan-mode worker, which the bulk path does not cover. Mode 2
    runs the serial kernel and the twins stay equal. No scheduler lists a plan so (a result is
    released after its last waiter left): the serial kernel then frees bytes the worker never
    counted, so the state audit is not asked here, only that both engines did the same."""
    g = mixed_graph()

    def plan(st, eng):
        ts = np.arange(g["n_tasks"], dtype=np.int32)
        return ts, np.zeros(len(ts), np.uint8)

    run_twins(g, dict(CFG, saturation=1.1), 200, plan, None, expect_path=SERIAL, until_scan=True, audit=False)


def test_cancel_a_large_graph():
    """120k tasks on 256 workers at saturation 1.1, every key released right after
    update_graph: about 12k root tasks queued, the workers full. Bulk only: the serial kernel
    would search the queue once per queued task."""
    from distributed_amd import graphs
    from distributed_amd.engine import PlacementEngine

    g = graphs.random_dag(120_000, 256, seed=9)
    N = g["n_tasks"]
    with PlacementEngine(0) as eng:
        eng.load(g, dict(CFG, saturation=1.1), snapshots=4, results=False)
        eng.update_graph()
        eng.snapshot()
        st = eng.task_states()
        assert (st == S_QUEUED).sum() > 10_000 and (st == S_PROCESSING).sum() >= 256
        plan = np.arange(N - 1, -1, -1, dtype=np.int32)
        assert eng.release_tasks(plan, np.zeros(N, np.uint8)) == 0  # auto: a plan this long is bulk
        assert eng.last_release_path == BULK
        eng.snapshot()
        snap = eng.snapshots(4)
        assert (eng.task_states() == S_RELEASED).all()
        # the last two snapshots: before the release, after it
        assert snap["round_nqueued"][-2] > 10_000 and snap["round_nqueued"][-1] == 0
        assert (snap["round_nproc"][-2] > 0).all() and (snap["round_nproc"][-1] == 0).all()
        assert (snap["round_occ"][-1] == 0).all()
        assert (snap["round_idle"][-1] == 1).all() and (snap["round_sat"][-1] == 0).all()
        assert eng.num_unrunnable() == 0
        v, skipped = eng.audit_state()
        assert not v and skipped == 0, v[:5]

"""The state audit (needs an MI355X): ``dgp_audit_state`` recounts every aggregate of the
engine's resident state on the device and reports where the kept value disagrees
(include/dgplace.h lists the rules; distributed_amd/csrc/dgp_audit.h has the kernels).

* the state the engine reaches by itself is consistent at every round boundary of every
  stimulus family, after every stimulus it decided on the device (reschedule, release, worker
  loss) and after every resync, in launch and resident mode;
* every rule fires on a state with exactly that field altered, with the engine's value and
  the recount's, and nothing else fires except what provably follows;
* after every reschedule the device decides on the svcrs streams, its state equals the dump
  the reference made of its own state, field for field (``audit_rows``: a dry run of the
  resync), and ``audit_rows`` reports exactly the field altered in a row;
* the audit changes nothing: the stream finishes bit-exact around it;
* the round-kernel engine (more than 32 prefixes) refuses it and carries on.

The altered states come in through ``dgp_sync_*`` (the one way to set the engine's state from
outside), so what the resync itself refuses -- an idle or saturated bit on a worker that is
not running, more than 8 prefixes in a dict -- cannot be planted and is asserted as refused.
After a resync the needs_what rule is one-sided (include/dgplace.h: an entry may count fewer
tasks than need it once a replica event or resync was seen, as in the reference), so a count
raised by one fires and a dropped entry shows as the network occupancy it no longer covers.
The order of a dict is history, not state: a self-audit cannot see two entries swapped (the
test says so); ``audit_rows`` against the scheduler's rows does, and is tested on it.
"""
import collections
import os

import numpy as np
import pytest

from conftest import (GOLDEN, svc_add_worker_files, svc_event_files, svc_loss_files, svc_p2p_files, svc_release_files,
                      svc_resync_files, svc_retry_files)
from oracle import oracle
from test_gpu_events import EV_RELEASE_KEYS, EV_RESCHEDULE, drive_events, sync_dump
from test_gpu_parity import PL_KEYS, ROUND_KEYS, assert_same
from test_gpu_service import drive, fixture_messages

pytestmark = pytest.mark.gpu


class Audited:
    """A proxy around the engine that forwards every call and audits the state after each
    round (``snapshot``), each stimulus the device decided and each resync."""

    def __init__(self, eng, scan_ok=False):
        self._e = eng
        self.scan_ok = scan_ok
        self.n = {"snapshot": 0, "reschedule": 0, "release_tasks": 0, "lose_worker": 0, "sync": 0}
        self.skipped = 0

    def __getattr__(self, k):
        return getattr(self._e, k)

    def check(self, where):
        found, skipped = self._e.audit_state()
        assert found == [] and found.total == 0, (where, self.n, found.total, found[:6])
        if not self.scan_ok:
            assert skipped == 0, (where, skipped)
        self.skipped += skipped
        self.n[where] += 1

    def snapshot(self):
        self._e.snapshot()
        self.check("snapshot")

    def reschedule(self, t):
        r = self._e.reschedule(t)
        if r is not None:
            self.check("reschedule")
        return r

    def release_tasks(self, task, forget):
        r = self._e.release_tasks(task, forget)
        if r is not None and len(task):
            self.check("release_tasks")
        return r

    def lose_worker(self, *a):
        r = self._e.lose_worker(*a)
        if r is not None:
            self.check("lose_worker")
        return r

    def sync(self, *a):
        self._e.sync(*a)
        self.check("sync")


def smallest(files):
    """The smallest stream of a family at the default values; the ``*_wide_*`` streams
    (multi-GB sizes, a config of their own) are named where a test runs them besides."""
    return min((f for f in files if "_wide_" not in f), key=lambda f: os.path.getsize(os.path.join(GOLDEN, f)))


def run_events(name, **kw):
    from distributed_amd.engine import PlacementEngine

    path = os.path.join(GOLDEN, name)
    g, cfg, exp, meta = oracle.load_fixture(path)
    z = np.load(path, allow_pickle=False)
    R = len(exp["round_nplaced"]) + 2
    with PlacementEngine(0) as eng:
        eng.load(g, cfg, snapshots=R, results=False)
        eng.update_graph()
        p = Audited(eng, scan_ok=name.startswith("svcp2p_"))  # the shuffle's barrier fills a needs table
        p.check("snapshot")  # right after update_graph
        stim = drive_events(p, g, z, exp, **kw)
        out = eng.placements()
        out.update(eng.snapshots(R))
        out["final_state"] = eng.task_states()
    assert np.array_equal(stim, exp["stim_nplaced"])
    assert_same(out, exp, PL_KEYS + ROUND_KEYS)
    assert np.array_equal(out["final_state"], np.where(exp["final_state"] == 7, 0, exp["final_state"]))
    return p, z


# ------------------------------------------------------------- 1. device-decided state
def compared(d, counts, sat_inf=False):
    """How many values of each field one audit_rows(dump) call compares, from the rows and the
    conditions of include/dgplace.h (remaining for waiting / queued / processing / no-worker
    rows, cur_nbytes for rows in memory, holder_of for processing rows and single-holder
    results, TD_MULTI for rows with several holders)."""
    t, w, g = d["tasks"], d["workers"], d["globals"]
    st = np.where(t["state"] == 7, 0, t["state"])
    hn = np.diff(t["holder_ptr"])
    n = len(st)
    for f in ("state", "waiters", "proc_on", "res_nbytes", "who_has", "lr", "wanted", "forgotten"):
        counts[f] += n
    counts["remaining"] += int(np.isin(st, (1, 2, 3, 4)).sum())
    counts["cur_nbytes"] += int((st == 5).sum())
    counts["holder_of"] += int(((st == 2) | ((st == 5) & (hn == 1))).sum())
    counts["multi"] += int((hn > 1).sum())
    W_ = len(w["status"])
    # cap / slots: not compared under worker-saturation inf (include/dgplace.h: nothing decides by them there)
    for f in ("nproc", "dict_len", "netocc", "nbytes", "flags") + (() if sat_inf else ("cap", "itcslots", "itc_slots")):
        counts[f] += W_
    counts["dict_prefix"] += int(w["plen"].sum()) + len(g["g_prefix"])
    counts["dict_count"] += int(w["plen"].sum()) + len(g["g_prefix"])
    nl = np.diff(w["needs_ptr"])
    counts["needs_count"] += int(nl[nl <= 63].sum())
    for f in ("n_idle", "n_sat", "n_itc", "n_tasks", "g_netocc", "queue_len", "bandwidth"):
        counts[f] += 1
    counts["queue_entry"] += len(g["queued"])
    counts["duration"] += 3 * len(g["duration_average"])
    counts["max_exec"] += len(g["max_exec_time"])
    for f in ("relwait", "group_left", "group_lastw"):
        counts[f] += len(g["group_left"])


class Pinned(Audited):
    """Audited, and after each stimulus the device decided where the reference dumped its own
    state (a reschedule, a release) the engine's state against that dump, field for field
    (audit_rows: a dry run of the resync). The dump index is counted as drive_events does:
    one per successful reschedule, one per release, one per resync."""

    def __init__(self, eng, z, sat_inf):
        super().__init__(eng)
        self.z, self.j, self.sat_inf = z, 0, sat_inf
        self.counts = {"device": collections.Counter(), "sync": collections.Counter()}

    def pin(self, where):
        d = sync_dump(self.z, self.j)
        found = self._e.audit_rows(d["tasks"], d["workers"], d["globals"])
        assert found == [] and found.total == 0, (where, self.j, found.total, found[:6])
        compared(d, self.counts["sync" if where == "sync" else "device"], self.sat_inf)
        self.j += 1

    def reschedule(self, t):
        r = super().reschedule(t)
        if r is not None:
            self.pin("reschedule")
        return r

    def release_tasks(self, task, forget):
        r = super().release_tasks(task, forget)
        if r is not None and len(task):
            self.pin("release_tasks")
        return r

    def sync(self, *a):
        super().sync(*a)
        self.pin("sync")  # a round trip: what the resync wrote, the audit reads back


@pytest.mark.parametrize("name", svc_resync_files())
def test_reference_dumps_pin_device_decided_state(name):
    """svcrs_*: after every reschedule decided on the device (dgp_reschedule) the engine's
    state equals the dump the reference made of its own state after that stimulus, field for
    field (audit_rows), and is self-consistent (audit_state); after every resync both hold
    too (there the dump check is a round trip). The placements, snapshots and final states
    equal the reference's as before. The svcrs fixtures carry no release plans (``rk_*``), so
    their releases resync; device-decided releases are audited on svcrel / svccan below,
    which have no dumps. Every field is compared at least once after a device-decided
    stimulus in each fixture, except, under worker-saturation inf, what the fixture's
    reference state never has (queue entries: nothing queues there) and the three fields no
    kernel decides by there (cap, itcslots, itc_slots: include/dgplace.h); the sat 1.1 fixture
    compares all of them."""
    from distributed_amd.engine import PlacementEngine

    path = os.path.join(GOLDEN, name)
    g, cfg, exp, meta = oracle.load_fixture(path)
    z = np.load(path, allow_pickle=False)
    R = len(exp["round_nplaced"]) + 2
    with PlacementEngine(0) as eng:
        eng.load(g, cfg, snapshots=R, results=False)
        eng.update_graph()
        p = Pinned(eng, z, cfg["saturation"] == "inf")
        stim = drive_events(p, g, z, exp, device_resched=True)
        out = eng.placements()
        out.update(eng.snapshots(R))
        out["final_state"] = eng.task_states()
    assert np.array_equal(stim, exp["stim_nplaced"])
    assert_same(out, exp, PL_KEYS + ROUND_KEYS)
    assert np.array_equal(out["final_state"], np.where(exp["final_state"] == 7, 0, exp["final_state"]))
    assert p.n["reschedule"] > 0 and p.n["sync"] > 0, p.n
    assert p.n["reschedule"] + p.n["sync"] == p.j == int(np.isin(z["ev_kind"], (8, EV_RESCHEDULE, EV_RELEASE_KEYS)).sum())
    empty = [f for f, c in p.counts["device"].items() if c == 0]
    inf = cfg["saturation"] == "inf"
    assert empty == (["queue_entry"] if inf else []), p.counts["device"]
    assert {"cap", "itcslots", "itc_slots"}.isdisjoint(p.counts["device"]) == inf


@pytest.mark.parametrize("name", svc_release_files())
def test_device_decided_releases_leave_a_consistent_state(name):
    """svcrel_* / svccan_*: every client release decided on the device (dgp_release_tasks:
    results in memory and cancelled work, released or forgotten) is followed by a clean audit.
    Fails on the parent of this change: a forgotten task stayed in its group's released count."""
    p, z = run_events(name, device_release=True)
    assert p.n["release_tasks"] > 0 and p.n["release_tasks"] == int((z["ev_kind"] == EV_RELEASE_KEYS).sum()), p.n


# --------------------------------------------------------- 2. clean at every round boundary
FAMILIES = [smallest(svc_event_files()), smallest([f for f in svc_loss_files() if f.startswith("svcwl_chain_")]),
            smallest([f for f in svc_loss_files() if f.startswith("svcwl_killed_")]), smallest(svc_retry_files()),
            smallest(svc_p2p_files())]
# ... and the recounts at byte counts past 2^32 (w_nbytes, w_netocc, g_netocc)
FAMILIES += ["svcev_wide_sat1.1.npz", "svcwl_chain_wide_sat1.1.npz"]


@pytest.mark.parametrize("name", FAMILIES)
def test_clean_at_every_round_boundary_of_an_event_stream(name):
    p, z = run_events(name, device_resched=True)
    assert p.n["snapshot"] == len(z["ev_round_ptr"]) > 1, p.n  # after update_graph and after every round
    if name.startswith("svcwl_"):
        assert p.n["lose_worker"] > 0, p.n
    if name.startswith("svcretry_"):
        assert p.n["reschedule"] > 0, p.n


SERVICE = ["c2var_sat1.1.npz", "c2p12_sat1.1.npz", "restr_sat1.1.npz", "c3mini_sat1.1.npz",
           "edge_scan_refill_sat1.1.npz", "edge_threads_sat1.1.npz", "edge_w1_sat1.1.npz", "edge_p32_sat1.1.npz"]
SCAN = {"edge_scan_refill_sat1.1.npz", "c3mini_sat1.1.npz"}  # a worker reaches scan mode (c3mini: the barrier's)


@pytest.mark.parametrize("resident", [False, True], ids=["launch", "resident"])
@pytest.mark.parametrize("name", SERVICE)
def test_clean_at_every_round_boundary_in_service_mode(name, resident):
    from distributed_amd.engine import PlacementEngine

    g, cfg, exp, meta = oracle.load_fixture(os.path.join(GOLDEN, name))
    msgs, ptr = fixture_messages(g, exp)
    R = len(exp["round_nplaced"]) + 2
    with PlacementEngine(0) as eng:
        eng.load(g, cfg, snapshots=R, results=False)
        eng.set_resident(resident)
        eng.update_graph()
        p = Audited(eng, scan_ok=name in SCAN)
        p.check("snapshot")
        status = drive(p, msgs, ptr, per_message=False)
        out = eng.placements()
        out.update(eng.snapshots(R))
        out["final_state"] = eng.task_states()
    assert (status == 0).all()
    assert_same(out, exp, PL_KEYS + ROUND_KEYS)
    assert np.array_equal(out["final_state"], exp["final_state"])
    if name in SCAN:  # needs tables past the line and the overflow: scan mode, skipped and said so
        assert p.skipped > 0
    else:
        assert p.skipped == 0


def device_caps(eng, n_workers):
    """w_cap of every worker, read through ``audit_rows``: against worker rows that claim 1,000
    long-running tasks each, every cap differs, and each ``cap`` record carries the engine's
    value."""
    z = np.zeros(n_workers, np.int32)
    rows = dict(status=z, nproc=z, n_long_running=z + 1000, plen=z, prefix=np.zeros(n_workers * PD, np.int32),
                count=np.zeros(n_workers * PD, np.int32), netocc=z, nbytes=z, idle=z, saturated=z,
                needs_ptr=np.zeros(n_workers + 1, np.int64), needs_task=z[:0], needs_count=z[:0])
    found = eng.audit_rows(workers=rows, cap=128 * n_workers)
    assert found.total == len(found)
    caps = {v.index: v.device_value for v in found if v.rule == "ROW_WORKERS" and v.field == "cap"}
    return [caps[w] for w in range(n_workers)]


@pytest.mark.parametrize("name", [smallest([f for f in svc_add_worker_files() if f.startswith("svcaddw_order_")]),
                                  "svcaddw_order_sat1.1.npz", "svcaddw_w1000_sat1.1.npz",
                                  "svcaddw_insrestr_sat1.1.npz", "svcaddw_ins64_sat1.1.npz"])
def test_clean_at_every_round_boundary_with_workers_joining(name):
    """Workers joining (dgp_add_worker_at: every later worker's index moves up on the device)
    and, with 1,000 workers, worker state outside LDS and who_has rows of several words;
    svcaddw_insrestr / svcaddw_ins64: insertions into a restricted graph, the second across
    the 64-worker word of the who_has rows (tests/test_join_census.py).
    After the last join every worker's slot cap is the cap rule of its own threads,
    max(ceil(saturation * nthreads), 1), computed here and not by the engine (audit_state's cap
    rule compares against the engine's own formula). The smallest svcaddw_order stream runs
    under worker-saturation inf, where the cap is 0, nothing decides by it and no audit compares
    it, so the cap is checked on the family's sat 1.1 stream and on the 1,000 workers."""
    import math

    from distributed_amd.engine import PlacementEngine

    path = os.path.join(GOLDEN, name)
    g, cfg, exp, meta = oracle.load_fixture(path)
    z = np.load(path, allow_pickle=False)
    cols = [z[k].tolist() for k in ("msg_task", "msg_worker", "msg_runid", "msg_nbytes", "msg_start", "msg_stop")]
    msgs = list(zip(*cols))
    ptr = z["msg_round_ptr"].tolist()
    n_add = len(z["add_nthreads"])
    pos = z["add_pos"].tolist() if "add_pos" in z else [None] * n_add
    run = z["add_running"].tolist() if "add_running" in z else [1] * n_add
    add_at = {}
    for i, nt, p_, r_ in zip(z["add_msg"].tolist(), z["add_nthreads"].tolist(), pos, run):
        add_at.setdefault(i, []).append((nt, p_, r_))
    for i, w in zip(*((z["res_msg"].tolist(), z["res_worker"].tolist()) if "res_msg" in z else ((), ()))):
        add_at.setdefault(i, []).append((0, w, 2))
    R = len(exp["round_nplaced"]) + 2
    nthreads, joined = g["nthreads"].tolist(), 0
    sat = float(cfg["saturation"])
    assert math.isfinite(sat) == ("satinf" not in name)
    with PlacementEngine(0) as eng:
        eng.load(g, cfg, snapshots=R, results=False)
        eng.update_graph()
        p = Audited(eng)
        p.check("snapshot")
        for k in range(len(ptr) - 1):
            i, e = ptr[k], ptr[k + 1]
            while i < e:
                for nt, p_, r_ in add_at.get(i, ()):
                    if r_ == 2:
                        eng.set_worker_status(p_, 1)
                    else:
                        eng.add_worker(nt, running=bool(r_), position=p_)
                        nthreads.insert(len(nthreads) if p_ is None else p_, nt)
                        joined += 1
                        if joined == n_add and math.isfinite(sat):  # the last join
                            assert device_caps(eng, len(nthreads)) == [max(math.ceil(sat * t), 1) for t in nthreads]
                    p.check("snapshot")  # right after the join
                j = i + 1
                while j < e and j not in add_at:
                    j += 1
                st, _ = eng.tasks_finished(*(np.array(c) for c in zip(*msgs[i:j])))
                assert (st == 0).all()
                i = j
            if e > ptr[k]:
                p.snapshot()
        out = eng.placements()
        out.update(eng.snapshots(R))
    assert_same(out, exp, PL_KEYS + ROUND_KEYS)
    assert p.n["snapshot"] > n_add


# ------------------------------------------------------------- 3. every rule fires
W = 128
CFG = {"bandwidth": 100_000_000, "default_data_size": 1024, "unknown_duration": 0.5, "saturation": 1.1}
PD = 8


def planted_state(g):
    """A consistent scheduler state over graph ``g`` as dgp_sync_* rows, small enough to
    reason about: tasks X1 processing on worker 1 with 12..63 distinct dependencies it does
    not hold (needs_what in overflow form), X2 on worker 2 with a few (line form), their
    dependencies D in memory on worker 0 (the first one also on worker 3), one waiting task,
    four queued roots, worker 5 paused, everything else released."""
    N = int(g["n_tasks"])
    dp, di = g["dep_ptr"], g["dep_idx"]
    deps = [di[dp[t]:dp[t + 1]].tolist() for t in range(N)]
    nb = 1000 + np.arange(N, dtype=np.int64)
    X, D = {}, set()

    def grow(w, lo):
        got = set()
        for t in range(N):
            if len(got) >= lo:
                break
            if not deps[t] or t in X or t in D or any(d in X for d in deps[t]):
                continue
            X[t] = w
            got.update(deps[t])
            D.update(deps[t])
        return got

    n1, n2 = grow(1, 14), grow(2, 4)
    assert 12 <= len(n1) <= 63 and 2 <= len(n2) <= 11
    y = next(t for t in range(N) if t not in X and t not in D and len(deps[t]) >= 2
             and not any(d in X for d in deps[t]) and any(d not in D for d in deps[t]))
    Q = [t for t in range(N) if not deps[t] and t not in D][:4]
    active = set(X) | {y} | set(Q)
    state = np.zeros(N, np.uint8)
    state[list(D)] = 5
    state[list(X)] = 2
    state[y] = 1
    state[Q] = 3
    remaining = np.zeros(N, np.int32)
    remaining[y] = sum(1 for d in deps[y] if d not in D)
    waiters = np.zeros(N, np.int32)
    for t in active:
        for d in deps[t]:
            if d in D:
                waiters[d] += 1
    proc = np.full(N, -1, np.int32)
    for t, w in X.items():
        proc[t] = w
    d0 = min(D)
    hold = [([0, 3] if t == d0 else [0]) if t in D else [] for t in range(N)]
    hp = np.zeros(N + 1, np.int64)
    hp[1:] = np.cumsum([len(h) for h in hold])
    tasks = dict(task=np.arange(N, dtype=np.int32), state=state, remaining=remaining, waiters=waiters,
                 processing_on=proc, nbytes=np.where(state == 5, nb, -1), long_running=np.zeros(N, np.uint8),
                 wanted=g["wanted"].copy(), holder_ptr=hp, holder_idx=np.array(sum(hold, []), np.int32))
    status = np.zeros(W, np.int8)
    status[5] = 1
    nproc = np.zeros(W, np.int32)
    plen, pfx, pcn = np.zeros(W, np.int32), np.zeros(W * PD, np.int32), np.zeros(W * PD, np.int32)
    netocc, wnb = np.zeros(W, np.int64), np.zeros(W, np.int64)
    needs = {w: {} for w in range(W)}
    gd = {}
    for t in sorted(X):
        w, p = X[t], int(g["prefix_id"][t])
        nproc[w] += 1
        row = pfx[w * PD:w * PD + plen[w]].tolist()
        if p not in row:
            pfx[w * PD + plen[w]] = p
            plen[w] += 1
            row.append(p)
        pcn[w * PD + row.index(p)] += 1
        gd[p] = gd.get(p, 0) + 1
        for d in deps[t]:
            needs[w][d] = needs[w].get(d, 0) + 1
    for w in range(W):
        netocc[w] = sum(int(nb[d]) for d in needs[w])
    wnb[0] = sum(int(nb[d]) for d in D)
    wnb[3] = int(nb[d0])
    idle = ((status == 0) & (nproc == 0)).astype(np.uint8)
    nptr = np.zeros(W + 1, np.int64)
    nptr[1:] = np.cumsum([len(needs[w]) for w in range(W)])
    workers = dict(status=status, nproc=nproc, n_long_running=np.zeros(W, np.int32), plen=plen, prefix=pfx, count=pcn,
                   netocc=netocc, nbytes=wnb, idle=idle, saturated=np.zeros(W, np.uint8), needs_ptr=nptr,
                   needs_task=np.array([d for w in range(W) for d in needs[w]], np.int32),
                   needs_count=np.array([c for w in range(W) for c in needs[w].values()], np.int32))
    P, G = len(g["prefix_default_dur"]), len(g["group_prefix"])
    relw = np.bincount(g["group_id"][(state <= 1)], minlength=G).astype(np.int64)
    glob = dict(n_tasks=0, network_occ_global=float(netocc.sum()), g_prefix=np.array(list(gd), np.int32),
                g_count=np.array(list(gd.values()), np.int64), queued=np.array(sorted(Q, key=lambda t: g["prio"][t]), np.int32),
                duration_average=np.full(P, -1.0), max_exec_time=np.full(P, -1.0), bandwidth=1e8,
                group_released_waiting=relw, group_left=np.zeros(G, np.int64), group_last_worker=np.full(G, -1, np.int32))
    info = dict(X=X, D=D, y=y, Q=glob["queued"].tolist(), d0=d0, nb=nb, deps=deps, needs=needs)
    return dict(tasks=tasks, workers=workers, globals=glob), info


def altered(base, part, **changes):
    out = {k: dict(v) for k, v in base.items()}
    for k, v in changes.items():
        out[part][k] = v
    return out


def bump(a, i, by=1):
    a = np.array(a).copy()
    a[i] += by
    return a


@pytest.fixture(scope="module")
def planted():
    from distributed_amd import graphs
    from distributed_amd.engine import PlacementEngine

    g = graphs.random_dag(600, W, seed=9, n_inner_prefixes=3)
    base, info = planted_state(g)
    with PlacementEngine(0) as eng:
        eng.load(g, CFG, results=False)
        eng.update_graph()
        assert eng.audit_state() == ([], 0)  # the engine's own state after update_graph
        eng.sync(None, base["tasks"], base["workers"], base["globals"])
        yield eng, g, base, info


def audit_after(eng, base, st, cap=64):
    eng.sync(None, st["tasks"], st["workers"], st["globals"])
    found, skipped = eng.audit_state(cap)
    eng.sync(None, base["tasks"], base["workers"], base["globals"])
    assert eng.audit_state() == ([], 0)  # and the planted state is clean again
    return found


def drop_need(wk, w, k):
    """worker w's k-th needs entry removed from the CSR (its network occupancy kept)."""
    p = wk["needs_ptr"]
    at = int(p[w]) + k
    ptr = p.copy()
    ptr[w + 1:] -= 1
    return dict(needs_ptr=ptr, needs_task=np.delete(wk["needs_task"], at), needs_count=np.delete(wk["needs_count"], at))


def test_the_planted_state_is_clean_and_in_the_forms_it_claims(planted):
    eng, g, base, info = planted
    assert eng.audit_state() == ([], 0)
    n = np.diff(base["workers"]["needs_ptr"])
    assert 12 <= n[1] <= 63 and 2 <= n[2] <= 11 and n.sum() == n[1] + n[2]  # overflow form, line form
    assert base["workers"]["plen"].max() >= 2 and len(info["Q"]) == 4


def test_each_altered_field_fires_its_rule_and_only_it(planted):
    from distributed_amd.engine import Violation as V

    eng, g, base, info = planted
    tk, wk, gl = base["tasks"], base["workers"], base["globals"]
    nb, needs = info["nb"], info["needs"]

    def one(st):
        return list(audit_after(eng, base, st))

    # WORKER_NPROC: nproc + 1 on one worker
    n2 = int(wk["nproc"][2])
    assert one(altered(base, "workers", nproc=bump(wk["nproc"], 2))) == [V("WORKER_NPROC", "nproc", 2, -1, n2 + 1, n2)]
    # WORKER_DICT: a dict count off by one; the global dict's sum follows (GLOBAL_DICT)
    p0, c0 = int(wk["prefix"][1 * PD]), int(wk["count"][1 * PD])
    gi = gl["g_prefix"].tolist().index(p0)
    gc = int(gl["g_count"][gi])
    assert one(altered(base, "workers", count=bump(wk["count"], 1 * PD))) == [
        V("WORKER_DICT", "dict_count", 1, p0, c0 + 1, c0), V("GLOBAL_DICT", "dict_count", -1, p0, gc, gc + 1)]
    # ... and a prefix nothing processes there
    free = next(p for p in range(len(g["prefix_default_dur"])) if p not in wk["prefix"][2 * PD:2 * PD + wk["plen"][2]])
    pf, pc = wk["prefix"].copy(), wk["count"].copy()
    pf[2 * PD + wk["plen"][2]], pc[2 * PD + wk["plen"][2]] = free, 1
    found = one(altered(base, "workers", plen=bump(wk["plen"], 2), prefix=pf, count=pc))
    assert found[0] == V("WORKER_DICT", "dict_count", 2, free, 1, 0) and {v.rule for v in found[1:]} == {"GLOBAL_DICT"}
    # two dict entries swapped: the order is insertion history, which no recount can see
    assert wk["plen"][1] >= 2
    pf, pc = wk["prefix"].copy(), wk["count"].copy()
    pf[[PD, PD + 1]], pc[[PD, PD + 1]] = pf[[PD + 1, PD]], pc[[PD + 1, PD]]
    assert one(altered(base, "workers", prefix=pf, count=pc)) == []
    # WORKER_NBYTES
    b0 = int(wk["nbytes"][0])
    assert one(altered(base, "workers", nbytes=bump(wk["nbytes"], 0))) == [V("WORKER_NBYTES", "nbytes", 0, -1, b0 + 1, b0)]
    # WORKER_NEEDS, line form (worker 2) and overflow form (worker 1): a count one too high ...
    for w in (2, 1):
        at = int(wk["needs_ptr"][w])
        d, c = int(wk["needs_task"][at]), int(wk["needs_count"][at])
        assert one(altered(base, "workers", needs_count=bump(wk["needs_count"], at))) == [
            V("WORKER_NEEDS", "needs_count", w, d, c + 1, c)]
        # ... an entry dropped: the network occupancy it no longer covers
        k = len(needs[w]) - 1
        dk = int(wk["needs_task"][at + k])
        no = int(wk["netocc"][w])
        assert one(altered(base, "workers", **drop_need(wk, w, k))) == [
            V("WORKER_NEEDS", "netocc", w, -1, no, no - int(nb[dk]))]
        # ... an entry for a dependency the worker holds (who_has gains w, and w its bytes)
        held = min(needs[w])
        hp = tk["holder_ptr"].copy()
        hi = np.insert(tk["holder_idx"], int(hp[held + 1]), w)
        hp[held + 1:] += 1
        found = one(altered(altered(base, "tasks", holder_ptr=hp, holder_idx=hi), "workers",
                            nbytes=bump(wk["nbytes"], w, int(nb[held]))))
        assert found == [V("WORKER_NEEDS", "needs_count", w, held, needs[w][held], 0)]
    # TASK_HOLDERS: a task in memory with no holders; its holder's nbytes and the tasks that
    # depend on it follow (WORKER_NBYTES, TASK_REMAINING)
    d1 = max(info["D"])
    hp = tk["holder_ptr"].copy()
    at = int(hp[d1])
    hp[d1 + 1:] -= 1
    found = one(altered(base, "tasks", holder_ptr=hp, holder_idx=np.delete(tk["holder_idx"], at)))
    assert found[0] == V("TASK_HOLDERS", "holders", d1, -1, 0, 1)
    assert V("WORKER_NBYTES", "nbytes", 0, -1, b0, b0 - int(nb[d1])) in found
    assert {v.rule for v in found[1:]} == {"WORKER_NBYTES", "TASK_REMAINING"}
    assert all(d1 in info["deps"][v.index] for v in found if v.rule == "TASK_REMAINING")
    # TD_MULTI: two holders on a row the flag does not cover cannot come through the resync
    # (it derives the flag); a bit on a removed or out-of-range worker is refused by it too
    # TASK_REMAINING: a waiting task with remaining - 1
    y, r = info["y"], int(tk["remaining"][info["y"]])
    assert one(altered(base, "tasks", remaining=bump(tk["remaining"], y, -1))) == [
        V("TASK_REMAINING", "remaining", y, -1, r - 1, r)]
    # TASK_WAITERS: a task in memory with waiters + 1
    wv = int(tk["waiters"][d1])
    assert one(altered(base, "tasks", waiters=bump(tk["waiters"], d1))) == [V("TASK_WAITERS", "waiters", d1, -1, wv + 1, wv)]
    # TASK_PROC: a released task that names a worker cannot come through the resync
    # (proc_on = -1 unless processing); a processing task on another worker shows in both counts
    x = min(info["X"])
    found = one(altered(base, "tasks", processing_on=bump(tk["processing_on"], x, 20)))
    assert {v.rule for v in found} == {"WORKER_NPROC", "WORKER_DICT", "WORKER_NEEDS"}
    # WORKER_FLAGS: a running worker with nothing processing that is not idle; idle and saturated
    idle = wk["idle"].copy()
    idle[7] = 0
    assert one(altered(base, "workers", idle=idle)) == [V("WORKER_FLAGS", "flags", 7, -1, 4, 5)]
    sat = wk["saturated"].copy()
    sat[8] = 1
    assert one(altered(base, "workers", saturated=sat)) == [V("WORKER_FLAGS", "flags", 8, -1, 7, 5)]
    # QUEUE: two entries swapped; one missing
    q = gl["queued"]
    assert one(altered(base, "globals", queued=q[[0, 2, 1, 3]])) == [V("QUEUE", "queue_entry", 2, -1, int(q[1]), -1)]
    assert one(altered(base, "globals", queued=np.delete(q, 1))) == [V("QUEUE", "queue_member", int(q[1]), -1, 0, 1)]
    assert one(altered(base, "globals", queued=np.append(q, q[0]))) == [
        V("QUEUE", "queue_entry", 4, -1, int(q[0]), -1), V("QUEUE", "queue_member", int(q[0]), -1, 2, 1)]
    # GLOBAL_DICT: a global count off by one
    p, c = int(gl["g_prefix"][0]), int(gl["g_count"][0])
    assert one(altered(base, "globals", g_count=bump(gl["g_count"], 0))) == [V("GLOBAL_DICT", "dict_count", -1, p, c + 1, c)]
    # GROUP_COUNT
    rw = int(gl["group_released_waiting"][0])
    assert one(altered(base, "globals", group_released_waiting=bump(gl["group_released_waiting"], 0))) == [
        V("GROUP_COUNT", "relwait", 0, -1, rw + 1, rw)]


def test_what_the_resync_refuses_cannot_be_planted(planted):
    """An idle or saturated bit on a worker that is not running never reaches the device:
    dgp_sync_workers and dgp_set_worker_flags both refuse it."""
    from distributed_amd import _lib

    eng, g, base, info = planted
    idle = base["workers"]["idle"].copy()
    idle[5] = 1  # worker 5 is paused
    with pytest.raises(_lib.DgpError, match="not running"):
        eng.sync_workers(dict(base["workers"], idle=idle))
    with pytest.raises(_lib.DgpError, match="paused"):
        eng.set_worker_flags([5], [1], [0])
    assert eng.audit_state() == ([], 0)


def test_more_violations_than_cap(planted):
    eng, g, base, info = planted
    nproc = base["workers"]["nproc"].copy()
    who = np.arange(W)[10:80]
    nproc[who] += 1
    found = audit_after(eng, base, altered(base, "workers", nproc=nproc), cap=64)
    assert found.total == 70 and len(found) == 64
    assert all(v.rule == "WORKER_NPROC" and v.field == "nproc" and v.device_value == v.expected_value + 1 for v in found)
    idx = [v.index for v in found]
    assert idx == sorted(idx) and len(set(idx)) == 64 and set(idx) <= set(who.tolist())
    everything = audit_after(eng, base, altered(base, "workers", nproc=nproc), cap=128)
    assert everything.total == 70 and [v.index for v in everything] == who.tolist()
    nothing = audit_after(eng, base, altered(base, "workers", nproc=nproc), cap=0)
    assert nothing.total == 70 and len(nothing) == 0


# ------------------------------------------------- 4. audit_rows reports the altered field
@pytest.fixture(scope="module")
def dumped():
    """An engine whose state is dump 24 of svcrs_c2var (queued tasks, needs tables, dicts of
    three prefixes, paused and removed workers, replicas), handed over by a resync."""
    from distributed_amd.engine import PlacementEngine

    path = os.path.join(GOLDEN, "svcrs_c2var_sat1.1.npz")
    g, cfg, exp, meta = oracle.load_fixture(path)
    d = sync_dump(np.load(path, allow_pickle=False), 24)
    d["globals"] = dict(d["globals"], n_tasks=int(d["globals"]["n_tasks"]),
                        network_occ_global=float(d["globals"]["network_occ_global"]),
                        bandwidth=float(d["globals"]["bandwidth"]))
    with PlacementEngine(0) as eng:
        eng.load(g, cfg, results=False)
        eng.update_graph()
        eng.sync(None, d["tasks"], d["workers"], d["globals"])
        yield eng, d


def test_audit_rows_reports_exactly_the_altered_field(dumped):
    """One value altered per column of each row kind: the record carries that field, the row,
    the engine's value and the altered one. Where the resync derives other fields from the
    column (holder_of from who_has and processing_on, cur_nbytes from nbytes, cap / flags /
    slots from status, nproc and n_long_running, the Ctl counters), those follow and are
    named; nothing else is reported, and the unaltered rows give nothing."""
    from distributed_amd.engine import Violation as V

    eng, d = dumped
    tk, wk, gl = d["tasks"], d["workers"], d["globals"]
    assert eng.audit_rows(tk, wk, gl) == [] and eng.audit_state()[0] == []
    task, st = tk["task"], tk["state"]
    hn = np.diff(tk["holder_ptr"])
    W_ = len(wk["status"])

    def check(part, must, may=(), **changes):
        rows = altered(d, part, **changes)
        found = eng.audit_rows(rows["tasks"], rows["workers"], rows["globals"], cap=256)
        assert found.total == len(found)
        for m in must:
            assert m in found, (m, found[:8])
        extra = {v.field for v in found if v not in must}
        assert extra <= set(may), (changes.keys(), extra, found[:8])
        assert eng.audit_rows(tk, wk, gl) == []  # nothing changed

    def row(cond):
        return int(np.nonzero(cond)[0][0])

    T, WK, G = "ROW_TASKS", "ROW_WORKERS", "ROW_GLOBALS"
    # ---- task rows
    i = row(st == 1)
    t = int(task[i])
    check("tasks", [V(T, "state", t, -1, 1, 4)], state=bump(st, i, 3))  # waiting -> no-worker
    r = int(tk["remaining"][i])
    check("tasks", [V(T, "remaining", t, -1, r, r + 1)], remaining=bump(tk["remaining"], i))
    wv = int(tk["waiters"][i])
    check("tasks", [V(T, "waiters", t, -1, wv, wv + 1)], waiters=bump(tk["waiters"], i))
    nb = int(tk["nbytes"][i])
    check("tasks", [V(T, "res_nbytes", t, -1, nb, nb + 1)], nbytes=bump(tk["nbytes"], i))
    wa = int(tk["wanted"][i])
    check("tasks", [V(T, "wanted", t, -1, wa, 1 - wa)], wanted=bump(tk["wanted"], i, 1 - 2 * wa))
    i = row(st == 0)
    check("tasks", [V(T, "forgotten", int(task[i]), -1, 0, 4)], state=bump(st, i, 7))  # released -> forgotten
    i = row((st == 2) & (tk["long_running"] == 0))
    t, po = int(task[i]), int(tk["processing_on"][i])
    check("tasks", [V(T, "lr", t, -1, 0, 1)], long_running=bump(tk["long_running"], i))
    other = (po + 1) % W_
    check("tasks", [V(T, "proc_on", t, -1, po, other), V(T, "holder_of", t, -1, po, other)],
          processing_on=bump(tk["processing_on"], i, other - po))
    i = row((st == 5) & (hn == 1))  # a result with one holder: the holder list names another worker
    t, k = int(task[i]), int(tk["holder_ptr"][i])
    h = int(tk["holder_idx"][k])
    h2 = (h + 1) % W_
    check("tasks", [V(T, "who_has", t, 0, 1 << h, 1 << h2), V(T, "holder_of", t, -1, h, h2)],
          holder_idx=bump(tk["holder_idx"], k, h2 - h))
    nb = int(tk["nbytes"][i])
    check("tasks", [V(T, "res_nbytes", t, -1, nb, nb + 1), V(T, "cur_nbytes", t, -1, nb, nb + 1)],
          nbytes=bump(tk["nbytes"], i))
    # a second holder on that result: the who_has word gains its bit and TD_MULTI must be set
    hp = tk["holder_ptr"].copy()
    hp[i + 1:] += 1
    check("tasks", [V(T, "who_has", t, 0, 1 << h, (1 << h) | (1 << h2)), V(T, "multi", t, -1, 0, 2)],
          holder_ptr=hp, holder_idx=np.insert(tk["holder_idx"], k + 1, h2))
    # ---- worker rows
    run = (wk["status"] == 0)
    w = row(run & (wk["nproc"] > 0) & (wk["plen"] >= 2))
    derived = ("flags", "itcslots", "n_itc", "itc_slots")
    n0 = int(wk["nproc"][w])
    check("workers", [V(WK, "nproc", w, -1, n0, n0 + 1)], may=derived, nproc=bump(wk["nproc"], w))
    check("workers", [], may=("cap",) + derived, n_long_running=bump(wk["n_long_running"], w))
    PDs = 8
    p0, p1 = int(wk["prefix"][w * PDs]), int(wk["prefix"][w * PDs + 1])
    c0 = int(wk["count"][w * PDs])
    check("workers", [V(WK, "dict_count", w, 0, c0, c0 + 1)], count=bump(wk["count"], w * PDs))
    pf, pc = wk["prefix"].copy(), wk["count"].copy()  # the dict's order: insertion order decides the fp64 sum
    pf[[w * PDs, w * PDs + 1]], pc[[w * PDs, w * PDs + 1]] = pf[[w * PDs + 1, w * PDs]], pc[[w * PDs + 1, w * PDs]]
    check("workers", [V(WK, "dict_prefix", w, 0, p0, p1), V(WK, "dict_prefix", w, 1, p1, p0)], may=("dict_count",),
          prefix=pf, count=pc)
    pl = int(wk["plen"][w])
    check("workers", [V(WK, "dict_len", w, -1, pl, pl - 1)], may=("dict_prefix", "dict_count"), plen=bump(wk["plen"], w, -1))
    v0 = int(wk["netocc"][w])
    check("workers", [V(WK, "netocc", w, -1, v0, v0 + 1)], netocc=bump(wk["netocc"], w))
    v0 = int(wk["nbytes"][w])
    check("workers", [V(WK, "nbytes", w, -1, v0, v0 + 1)], nbytes=bump(wk["nbytes"], w))
    i0 = int(wk["idle"][w])
    check("workers", [], may=("flags", "n_idle"), idle=bump(wk["idle"], w, 1 - 2 * i0))
    s0 = int(wk["saturated"][w])
    check("workers", [], may=("flags", "n_sat"), saturated=bump(wk["saturated"], w, 1 - 2 * s0))
    ws = row(run & (wk["idle"] == 0) & (wk["saturated"] == 0))
    check("workers", [V(WK, "state", ws, -1, 0, 1)], may=derived, status=bump(wk["status"], ws))  # paused
    wn = row(np.diff(wk["needs_ptr"]) >= 2)
    k = int(wk["needs_ptr"][wn])
    dn, cn = int(wk["needs_task"][k]), int(wk["needs_count"][k])
    check("workers", [V(WK, "needs_count", wn, dn, cn, cn + 1)], needs_count=bump(wk["needs_count"], k))
    spare = next(x for x in range(len(task)) if x not in set(wk["needs_task"][k:int(wk["needs_ptr"][wn + 1])].tolist()))
    check("workers", [V(WK, "needs_count", wn, dn, cn, 0), V(WK, "needs_count", wn, spare, 0, cn)],
          needs_task=bump(wk["needs_task"], k, spare - dn))
    # ---- global rows
    check("globals", [V(G, "n_tasks", 0, -1, gl["n_tasks"], gl["n_tasks"] + 1)], n_tasks=gl["n_tasks"] + 1)
    x = gl["network_occ_global"]
    check("globals", [V(G, "g_netocc", 0, -1, x, float(np.nextafter(x, np.inf)))],
          network_occ_global=float(np.nextafter(x, np.inf)))  # one ulp
    x = gl["bandwidth"]
    check("globals", [V(G, "bandwidth", -1, -1, x, float(np.nextafter(x, np.inf)))], bandwidth=float(np.nextafter(x, np.inf)))
    gp, gc = gl["g_prefix"], gl["g_count"]
    check("globals", [V(G, "dict_count", 0, -1, int(gc[0]), int(gc[0]) + 1)], g_count=bump(gc, 0))
    sw = np.arange(len(gp))
    sw[[0, 1]] = [1, 0]
    check("globals", [V(G, "dict_prefix", 0, -1, int(gp[0]), int(gp[1])), V(G, "dict_prefix", 1, -1, int(gp[1]), int(gp[0]))],
          may=("dict_count",), g_prefix=gp[sw], g_count=gc[sw])
    q = gl["queued"]
    sw = np.arange(len(q))
    sw[[1, 2]] = [2, 1]
    check("globals", [V(G, "queue_entry", 1, -1, int(q[1]), int(q[2])), V(G, "queue_entry", 2, -1, int(q[2]), int(q[1]))],
          queued=q[sw])
    check("globals", [V(G, "queue_len", -1, -1, len(q), len(q) - 1)], queued=q[:-1])
    da = gl["duration_average"]
    up = da.copy()
    up[1] = np.nextafter(da[1], np.inf)
    check("globals", [V(G, "duration", 1, k_, float(da[1]), float(up[1])) for k_ in range(3)], duration_average=up)
    mx = gl["max_exec_time"]
    up = mx.copy()
    up[0] = np.nextafter(mx[0], np.inf)
    check("globals", [V(G, "max_exec", 0, -1, float(mx[0]), float(up[0]))], max_exec_time=up)
    for col, f in (("group_released_waiting", "relwait"), ("group_left", "group_left")):
        v0 = int(gl[col][1])
        check("globals", [V(G, f, 1, -1, v0, v0 + 1)], **{col: bump(gl[col], 1)})
    lw = int(gl["group_last_worker"][1])
    lw2 = (lw + 2) % W_
    check("globals", [V(G, "group_lastw", 1, -1, lw, lw2)], group_last_worker=bump(gl["group_last_worker"], 1, lw2 - lw))


# ------------------------------------- 4b. the resync and its dry run share one set of rules
def with_holder(tk, i, w):
    """Task rows with worker ``w`` appended to row i's holder list."""
    hp = tk["holder_ptr"].copy()
    hp[i + 1:] += 1
    return dict(tk, holder_ptr=hp, holder_idx=np.insert(tk["holder_idx"], int(tk["holder_ptr"][i + 1]), w))


def test_a_refused_resync_changes_nothing(dumped):
    """A resync call that is refused at its last row leaves the engine as it was: the rows
    before it, valid and different from the engine's state, are not applied in part.

    Workers: worker 0 goes running -> paused (idle and saturated cleared) and the last row
    carries nine prefixes. On the parent of this change dgp_sync_workers had moved the host's
    status column for worker 0 before it refused, and ``audit_rows`` reports it (ROW_WORKERS
    ``state``, row 0). Tasks: row 0's ``wanted`` is flipped and the last row names a holder out
    of range. On the parent dgp_sync_tasks had put the flag into the host's copy of the task
    flags, which the next dgp_sync_workers uploads; so the original worker rows are resynced
    before the audit, and the parent then reports ROW_TASKS ``wanted`` for row 0."""
    from distributed_amd import _lib

    eng, d = dumped
    tk, wk, gl = d["tasks"], d["workers"], d["globals"]
    W_ = len(wk["status"])
    assert wk["status"][0] == 0 and W_ > 1
    status, idle, sat, plen = wk["status"].copy(), wk["idle"].copy(), wk["saturated"].copy(), wk["plen"].copy()
    status[0], idle[0], sat[0], plen[-1] = 1, 0, 0, 9
    with pytest.raises(_lib.DgpError, match="more than 8 prefixes"):
        eng.sync_workers(dict(wk, status=status, idle=idle, saturated=sat, plen=plen))
    assert eng.audit_rows(tk, wk, gl) == [] and eng.audit_state() == ([], 0)
    wanted = tk["wanted"].copy()
    wanted[0] = 1 - wanted[0]
    with pytest.raises(_lib.DgpError, match="holder out of range"):
        eng.sync_tasks(dict(with_holder(tk, len(tk["task"]) - 1, W_), wanted=wanted))
    eng.sync_workers(wk)  # uploads the host's copy of the task flags
    assert eng.audit_rows(tk, wk, gl) == [] and eng.audit_state() == ([], 0)


def malformed(d, N):
    """(row kind, what is wrong, rows) for every input the resync refuses, over dump ``d`` of an
    engine with N tasks."""
    tk, wk, gl = d["tasks"], d["workers"], d["globals"]
    W_, P_ = len(wk["status"]), len(gl["duration_average"])
    PDs = 8

    def at(a, i, v):
        a = np.array(a).copy()
        a[i] = v
        return a

    proc = int(np.nonzero(tk["state"] == 2)[0][0])
    yield "tasks", "task id out of range", dict(tk, task=at(tk["task"], 0, N))
    yield "tasks", "state 8", dict(tk, state=at(tk["state"], 0, 8))
    yield "tasks", "descending holder_ptr", dict(tk, holder_ptr=at(tk["holder_ptr"], 1, -1))
    yield "tasks", "holder out of range", with_holder(tk, len(tk["task"]) - 1, W_)
    yield "tasks", "processing without a worker", dict(tk, processing_on=at(tk["processing_on"], proc, -1))
    run, paused, removed = (int(np.nonzero(wk["status"] == s)[0][0]) for s in (0, 1, 2))
    dicted = int(np.nonzero(wk["plen"] >= 1)[0][0])
    nl = np.diff(wk["needs_ptr"])
    k = int(wk["needs_ptr"][int(np.nonzero((nl >= 1) & (nl <= 63))[0][0])])  # a table the resync reads entry by entry
    yield "workers", "status 3", dict(wk, status=at(wk["status"], run, 3))
    yield "workers", "plen 9", dict(wk, plen=at(wk["plen"], run, 9))
    yield "workers", "prefix id = P", dict(wk, prefix=at(wk["prefix"], dicted * PDs, P_))
    yield "workers", "idle on a paused worker", dict(wk, idle=at(wk["idle"], paused, 1))
    yield "workers", "a removed worker returns", dict(wk, status=at(wk["status"], removed, 1))
    yield "workers", "needs count 0", dict(wk, needs_count=at(wk["needs_count"], k, 0))
    yield "workers", "needs count 256", dict(wk, needs_count=at(wk["needs_count"], k, 256))
    yield "workers", "needs task = N", dict(wk, needs_task=at(wk["needs_task"], k, N))
    yield "workers", "descending needs_ptr", dict(wk, needs_ptr=at(wk["needs_ptr"], 1, -1))
    many = 64 + 1  # PMAX_G (csrc/dgp_device.h): the prefixes the global dict holds
    yield "globals", "g_plen = PMAX_G + 1", dict(gl, g_prefix=np.zeros(many, np.int32), g_count=np.ones(many, np.int64))
    yield "globals", "prefix id = P", dict(gl, g_prefix=at(gl["g_prefix"], 0, P_))
    yield "globals", "queued task = N", dict(gl, queued=at(gl["queued"], 0, N))
    yield "globals", "last worker = W", dict(gl, group_last_worker=at(gl["group_last_worker"], 0, W_))
    yield "globals", "bandwidth 0", dict(gl, bandwidth=0.0)


def test_the_dry_run_refuses_what_the_resync_refuses_in_the_same_words(dumped):
    """Every malformed input: dgp_sync_* and dgp_audit_* both refuse it, with the same message
    once the function's name is taken out, and neither has changed anything (``audit_rows`` of
    the dump is clean after each)."""
    from distributed_amd import _lib

    eng, d = dumped
    tk, wk, gl = d["tasks"], d["workers"], d["globals"]
    N = len(eng.task_states())
    seen = 0
    for kind, what, rows in malformed(d, N):
        with pytest.raises(_lib.DgpError) as synced:
            getattr(eng, f"sync_{kind}")(rows)
        with pytest.raises(_lib.DgpError) as audited:
            eng.audit_rows(**{"globals_" if kind == "globals" else kind: rows})
        said = str(synced.value)
        assert f"dgp_sync_{kind} failed (-1): dgp_sync_{kind}: " in said, (what, said)
        assert str(audited.value) == said.replace(f"dgp_sync_{kind}", f"dgp_audit_{kind}"), (what, said, str(audited.value))
        assert eng.audit_rows(tk, wk, gl) == [], what
        seen += 1
    assert seen == 19 and eng.audit_state() == ([], 0)


# ----------------------------------------------------------------------- 5. read-only
@pytest.mark.parametrize("resident", [False, True], ids=["launch", "resident"])
def test_the_audit_changes_nothing(resident):
    from distributed_amd.engine import PlacementEngine

    name = smallest(svc_event_files())
    path = os.path.join(GOLDEN, name)
    g, cfg, exp, meta = oracle.load_fixture(path)
    z = np.load(path, allow_pickle=False)
    R = len(exp["round_nplaced"]) + 2
    seen = []

    class Mid(Audited):
        def snapshot(self):
            e = self._e
            e.snapshot()
            before = (e.task_states(), e.num_placements(), e.get_window(), e.snapshots(R))
            self.check("snapshot")
            after = (e.task_states(), e.num_placements(), e.get_window(), e.snapshots(R))
            assert np.array_equal(before[0], after[0]) and before[1:3] == after[1:3]
            assert before[3].keys() == after[3].keys()
            for k in before[3]:
                assert np.array_equal(before[3][k], after[3][k]), k
            seen.append(before[1])

    with PlacementEngine(0) as eng:
        eng.load(g, cfg, snapshots=R, results=False)
        eng.set_resident(resident)
        eng.update_graph()
        stim = drive_events(Mid(eng), g, z, exp)
        out = eng.placements()
        out.update(eng.snapshots(R))
        out["final_state"] = eng.task_states()
    assert len(seen) > 10
    assert np.array_equal(stim, exp["stim_nplaced"])
    assert_same(out, exp, PL_KEYS + ROUND_KEYS)
    assert np.array_equal(out["final_state"], exp["final_state"])


def test_the_round_kernel_engine_refuses_and_carries_on():
    from distributed_amd import _lib
    from distributed_amd.engine import PlacementEngine

    g, cfg, exp, meta = oracle.load_fixture(os.path.join(GOLDEN, "edge_p40_sat1.1.npz"))
    assert len(g["prefix_default_dur"]) > 32
    msgs, ptr = fixture_messages(g, exp)
    R = len(exp["round_nplaced"]) + 2
    with PlacementEngine(0) as eng:
        eng.load(g, cfg, snapshots=R, results=False)
        eng.update_graph()
        z0, G_, P_ = np.zeros(0, np.int32), len(g["group_prefix"]), len(g["prefix_default_dur"])
        rows = dict(
            tasks=dict(task=z0, state=z0, remaining=z0, waiters=z0, processing_on=z0, nbytes=z0, long_running=z0,
                       wanted=z0, holder_ptr=np.zeros(1, np.int64), holder_idx=z0),
            workers=dict(status=z0, nproc=z0, n_long_running=z0, plen=z0, prefix=z0, count=z0, netocc=z0, nbytes=z0,
                         idle=z0, saturated=z0, needs_ptr=np.zeros(1, np.int64), needs_task=z0, needs_count=z0),
            globals_=dict(n_tasks=0, network_occ_global=0.0, g_prefix=z0, g_count=z0, queued=z0,
                          duration_average=np.zeros(P_), max_exec_time=np.zeros(P_), bandwidth=1e8,
                          group_released_waiting=np.zeros(G_, np.int64), group_left=np.zeros(G_, np.int64),
                          group_last_worker=np.full(G_, -1, np.int32)))
        with pytest.raises(_lib.DgpError, match=r"\(-3\)"):
            eng.audit_state()
        for kind, r in rows.items():  # the four calls
            with pytest.raises(_lib.DgpError, match=r"dgp_audit_.* failed \(-3\)"):
                eng.audit_rows(**{kind: r})
        half = len(ptr) // 2
        st1 = drive(eng, msgs, ptr[:half + 1], per_message=False)
        with pytest.raises(_lib.DgpError, match=r"\(-3\)"):
            eng.audit_state()
        st2 = drive(eng, msgs, ptr[half:], per_message=False)
        out = eng.placements()
        out.update(eng.snapshots(R))
        out["final_state"] = eng.task_states()
    assert (st1 == 0).all() and (st2 == 0).all()
    assert_same(out, exp, PL_KEYS + ROUND_KEYS)
    assert np.array_equal(out["final_state"], exp["final_state"])


def test_refused_after_a_replay_and_while_a_batch_is_posted():
    from distributed_amd import _lib, graphs
    from distributed_amd.engine import PlacementEngine

    g = graphs.random_dag(600, 16, seed=9)
    with PlacementEngine(0) as eng:
        eng.load(g, CFG)
        eng.update_graph()
        assert eng.audit_state() == ([], 0)
        pl = eng.placements(0, 1)
        eng.tasks_finished_post([int(pl["pl_task"][0])], [int(pl["pl_worker"][0])], [0], [100], [0.0], [0.01])
        with pytest.raises(_lib.DgpError, match=r"\(-3\)"):
            eng.audit_state()
        eng.tasks_finished_wait()
        assert eng.audit_state() == ([], 0)
    with PlacementEngine(0) as eng:
        eng.load(g, CFG)
        eng.update_graph()
        eng.run_rounds(2)
        with pytest.raises(_lib.DgpError, match="replay"):
            eng.audit_state()

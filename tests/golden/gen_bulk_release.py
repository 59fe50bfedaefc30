"""svcbulk_*: client-releases-keys calls that name many keys at once (a cancelled
computation, a closing client), through the reference's own ``Scheduler.client_releases_keys``
(distributed/scheduler.py:5417-5430), in the event streams of ``gen_service.py``. The fixtures go
to ``tests/golden/bulk/``: the replay tests take every file of ``tests/golden/`` itself whose
family they do not know for a plain replay.

Run (from the repo root, build container: python3.9 + ``_refshim``)::

    PYTHONHASHSEED=0 /opt/conda/bin/python3.9 tests/golden/gen_bulk_release.py [name ...]

``gen_service.replay_events`` runs unchanged, as for ``svccan_*`` (release_cancel: every plan
from ``distributed_amd.loss.release_plan`` is recorded in ``rk_*`` and checked to name exactly
the tasks the transitions changed). What this file adds sits on the two calls it makes per
release: the plan and the reference's handler both get the keys a policy widened the one key
to --

* ``half``   the first call, once a case's share of the graph has finished: a random half of the wanted
             keys; the rest of the graph then runs on, with smaller calls (a twentieth)
* ``all``    that first call: every wanted key
* ``group``  every wanted key of one TaskGroup per call
* ``tail``   that first call: the wanted keys that descend from the last task in the queue, so
             that it (and whatever else they alone needed) leaves the queue; then as ``half``
* ``skew``   that first call: one processing key of each of three workers, four fifths of the
             processing keys of every other worker and the wanted results in memory, ordered so
             that the plan (the keys reversed: release_plan pops LIFO) lists the three workers'
             exits first and the results last; then as ``half``. The three workers'
             check_idle_saturated sees about the entry total, the others' last exits lie
             somewhere inside the plan
* ``thin_skew``  a first call that leaves three workers 2 x nthreads + 4 processing keys, then
             the ``skew`` call with those three listed first

Per multi-key call the fixture also records (``bk_*``, one row per call): the event index, the
plan's length, the queue's length before it and the places in the queue of the queued tasks
it removes (CSR), how many workers were paused, how many cancelled tasks were long-running,
how many released results had several replicas, the call's keys in the order they were sent
(``bk_key_ptr`` / ``bk_key_row``: each as the row of its task in the call's plan), and
``bk_sens``: how many workers that lost a
processing task would end with other idle / saturated flags had check_idle_saturated read
the end-of-call total occupancy instead of the total at the worker's last exit (computed on
the reference state between the transitions and the queue refill). ``rk_state``: each plan
row's state when the call began. A bounded search over seeds (``SEARCH``) looks for a
svcbulk_half_c2mini_satinf stream with bk_sens > 0; ``bk_search`` records how many seeds were
tried and what was found (none: the ``skew`` policy is what reaches such workers).

The ``skew`` / ``thin_skew`` streams record more per call (the earlier streams keep the arrays
they were committed with). check_idle_saturated is wrapped during the call to keep, per worker,
the global prefix counts and ``_network_occ_global`` as of its last check, so that the total can
be put together from either term at either time: ``bk_sens_idle`` / ``bk_sens_sat`` (which
flag the end-of-call total would change), ``bk_sens_cnt`` (workers whose flags would differ
with only the prefix counts read at the end of the call, the network bytes as of the exit),
``bk_sens_net`` (the converse), ``bk_freed`` (``_network_occ_global`` before the call less
after its transitions: the bytes its exits freed) and ``bk_idle`` / ``bk_sat`` (calls x
workers: every worker's flags when the handler returns, the refill included).
"""
from __future__ import annotations

import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gen_service as S  # noqa: E402  (re-executes under PYTHONHASHSEED=0, installs the shim)

import numpy as np  # noqa: E402

G = S.G
BULK = os.path.join(HERE, "bulk")  # tests/golden/bulk/svcbulk_*.npz
EV_RELEASE_KEYS = 10
SEARCH = 200  # seeds tried for a stream with an order-sensitive worker


class Widen:
    """The policy between replay_events and the reference: one key in, many keys out."""

    def __init__(self, mode, seed, early):
        self.mode, self.rng, self.early = mode, np.random.default_rng(seed), early
        self.spare = None  # skew: the workers whose exits the plan lists first
        self.loss = S_load("loss")
        self.pending = None
        self.first_done = False
        self.calls = []
        self.rk_state = []

    # --- replay_events' LR.release_plan(s, client, [key])
    def release_plan(self, s, client, keys):
        tss = list(s.tasks.values())
        n_done = sum(ts.state in ("memory", "released", "forgotten") for ts in tss)
        wanted = [ts for ts in tss if ts.who_wants and ts.state != "erred"]
        if not self.first_done and n_done < self.early * len(tss):
            self.pending = None
            return None  # too early: replay_events skips the event
        if self.mode == "group":
            grp = s.tasks[keys[0]].group
            pick = [ts for ts in wanted if ts.group is grp]
        elif not self.first_done and self.mode == "tail":
            if not len(s.queued):
                self.pending = None
                return None
            seen, stack = set(), [list(s.queued.sorted())[-1]]
            while stack:  # everything that descends from the last queued task
                ts = stack.pop()
                if ts not in seen:
                    seen.add(ts)
                    stack.extend(ts.dependents)
            pick = [ts for ts in wanted if ts in seen]
        elif self.mode == "thin_skew" and self.spare is None:
            pick = self.thin(wanted)
        elif self.mode in ("skew", "thin_skew") and (not self.first_done or self.spare):
            pick = self.skew(wanted)
        elif not self.first_done:
            pick = wanted if self.mode == "all" else [ts for ts in wanted if self.rng.random() < 0.5]
        else:
            pick = [ts for ts in wanted if self.rng.random() < 0.05]
        if pick is None:
            self.pending = None
            return None
        ks = [ts.key for ts in pick]
        if keys[0] not in ks:
            if self.mode in ("skew", "thin_skew"):
                ks.insert(0, keys[0])  # the last place of the plan: the order of the exits stays
            else:
                ks.append(keys[0])
        plan = self.loss.release_plan(s, client, ks)
        self.pending = ks if plan is not None else None
        if plan is not None:
            self.plan = plan
        return plan

    N_SPARE = 3

    @staticmethod
    def by_worker(wanted):
        by = {}
        for ts in wanted:
            if ts.state == "processing" and ts not in ts.processing_on.long_running:
                by.setdefault(ts.processing_on, []).append(ts)
        return by

    def thin(self, wanted):
        """thin_skew's first call: the spare workers keep a few more tasks than threads."""
        by = self.by_worker(wanted)
        ws = [w for w in by if len(by[w]) > 4 * w.nthreads + 8]
        if len(by) < 2 * self.N_SPARE or len(ws) < self.N_SPARE:
            return None
        self.spare = [ws[i] for i in sorted(self.rng.choice(len(ws), self.N_SPARE, replace=False).tolist())]
        return [ts for w in self.spare for ts in by[w][:len(by[w]) - (2 * w.nthreads + 4)]]

    def skew(self, wanted):
        """One processing key of each spare worker and four fifths of the other workers'; the
        plan is the keys reversed, so the spare workers' keys go last. With them, first in the
        keys, the wanted results in memory: they leave after every exit."""
        by = self.by_worker(wanted)
        if self.spare is None:
            if len(by) < 2 * self.N_SPARE:
                return None
            ws = list(by)
            self.spare = [ws[i] for i in sorted(self.rng.choice(len(ws), self.N_SPARE, replace=False).tolist())]
        spare = [w for w in self.spare if w in by]
        if not spare or len(by) < 2 * self.N_SPARE:
            return None
        self.spare = []  # the skew call is this one; later calls as ``half``
        mem = [ts for ts in wanted if ts.state == "memory"]
        rest = [ts for w, l in by.items() if w not in spare for ts in l if self.rng.random() < 0.8]
        return mem + rest + [by[w][int(self.rng.integers(0, len(by[w])))] for w in spare]

    # --- the reference's handler, with the widened keys
    def handler(self, orig):
        me = self

        def client_releases_keys(self, keys, client, stimulus_id=None):
            ks = me.pending
            assert ks is not None and keys[0] in ks
            me.pending = None
            me.first_done = True
            plan = me.plan
            q = {ts: i for i, ts in enumerate(self.queued.sorted())}
            proc = [ts for ts, _ in plan if ts.state == "processing"]
            row = dict(n=len(plan), qlen=len(q), qpos=sorted(q[ts] for ts, _ in plan if ts.state == "queued"),
                       npaused=sum(ws not in self.running for ws in self.workers.values()),
                       nlr=sum(ts in ts.processing_on.long_running for ts in proc),
                       nmulti=sum(ts.state == "memory" and len(ts.who_has) > 1 for ts, _ in plan))
            me.rk_state.extend(G.STATE_CODES[ts.state] for ts, _ in plan)
            at = {ts.key: i for i, (ts, _) in enumerate(plan)}
            row["keys"] = [at[k] for k in ks]  # every key is a row of its plan (one client: all transition)
            exits = {ts.processing_on for ts in proc}
            cls = type(self)
            refill = cls.stimulus_queue_slots_maybe_opened
            check = cls.check_idle_saturated
            at_check = {}  # per worker: the two terms of the total as of its last check
            net0 = self._network_occ_global

            def checked(self2, ws, occ=-1.0):
                at_check[ws] = (dict(self2._task_prefix_count_global), self2._network_occ_global)
                return check(self2, ws, occ)

            def before_refill(self2, stimulus_id):
                cnt1, net1 = self2._task_prefix_count_global, self2._network_occ_global
                sens = idle = sat = by_cnt = by_net = 0
                for ws in exits:
                    now = (ws.address in self2.idle, ws in self2.saturated)
                    end = me.flags_at_end(self2, ws)
                    sens += end != now
                    idle += end[0] != now[0]
                    sat += end[1] != now[1]
                    cnt0, netx = at_check[ws]
                    assert me.flags_with(self2, ws, self2._calc_occupancy(cnt0, netx)) == now
                    by_cnt += me.flags_with(self2, ws, self2._calc_occupancy(cnt1, netx)) != now
                    by_net += me.flags_with(self2, ws, self2._calc_occupancy(cnt0, net1)) != now
                assert net0 - net1 == int(net0 - net1) >= 0
                row.update(sens=sens, sens_idle=idle, sens_sat=sat, sens_cnt=by_cnt, sens_net=by_net,
                           freed=int(net0 - net1))
                return refill(self2, stimulus_id=stimulus_id)

            cls.stimulus_queue_slots_maybe_opened = before_refill
            cls.check_idle_saturated = checked
            try:
                r = orig(self, keys=ks, client=client, stimulus_id=stimulus_id)
            finally:
                cls.stimulus_queue_slots_maybe_opened = refill
                cls.check_idle_saturated = check
            # what the call leaves, the refill included: the flags of every worker, by index
            # (Scheduler.workers is sorted by address, and the addresses sort by index)
            row["idle"] = [ws.address in self.idle for ws in self.workers.values()]
            row["sat"] = [ws in self.saturated for ws in self.workers.values()]
            me.calls.append(row)
            return r

        return client_releases_keys

    @staticmethod
    def flags_at_end(s, ws):
        """check_idle_saturated's idle / saturated (:2949-2991) with the total occupancy as it
        is now, all transitions done."""
        return Widen.flags_with(s, ws, s.total_occupancy)

    @staticmethod
    def flags_with(s, ws, total):
        """... with ``total`` for SchedulerState.total_occupancy."""
        from distributed.core import Status

        occ, p, nc = ws.occupancy, len(ws.processing), ws.nthreads
        if ws.status != Status.running:
            return False, False
        if p < nc or occ < nc * (total / s.total_nthreads) / 2:  # is_unoccupied :2997-3004
            return True, False
        sat = False
        if p > nc:
            pending = occ * (p - nc) / (p * nc)
            sat = 0.4 < pending > 1.9 * (total / s.total_nthreads)
        return False, sat


S_load = S._load_repo_module


def generate(name, mk, sat, seed, p_event, mode, early=0.3):
    from distributed.scheduler import Scheduler

    g = mk()
    G.graphs.check_graph(g)
    cfg = S.own_config(name, sat)
    w = Widen(mode, seed, early)
    orig = Scheduler.client_releases_keys
    proxy = type("LossProxy", (), {"release_plan": staticmethod(w.release_plan)})
    S._load_repo_module = lambda nm: proxy if nm == "loss" else S_load(nm)
    Scheduler.client_releases_keys = w.handler(orig)
    try:
        with G.reference_config(cfg):
            rec, rounds, nplaced, states, ev, hb, round_ptr = S.replay_events(
                g, cfg, seed, p_event, (1, 2, 3, 4, 5, 6, 7, EV_RELEASE_KEYS, EV_RELEASE_KEYS), dumps=[],
                release_cancel=True)
    finally:
        Scheduler.client_releases_keys = orig
        S._load_repo_module = S_load
    return g, cfg, rec, rounds, nplaced, states, ev, hb, round_ptr, w


def save(name, out, search):
    g, cfg, rec, rounds, nplaced, states, ev, hb, round_ptr, w = out
    G.save(name, g, cfg, rec, rounds, nplaced, states, 0.0,
           generator=f"PYTHONHASHSEED=0 python3.9 tests/golden/gen_bulk_release.py {name}")
    os.makedirs(BULK, exist_ok=True)
    path = os.path.join(BULK, f"{name}.npz")
    os.replace(os.path.join(HERE, f"{name}.npz"), path)  # out of the folder the replay tests list
    z = dict(np.load(path, allow_pickle=False))
    lo = hb["lo"]
    rel = [i for i, k in enumerate(ev["kind"]) if k == EV_RELEASE_KEYS]
    assert len(rel) == len(w.calls) and len(w.rk_state) == len(lo["rtask"])
    assert [c["n"] for c in w.calls] == [lo["rptr"][i + 1] - lo["rptr"][i] for i in rel]
    qptr = np.cumsum([0] + [len(c["qpos"]) for c in w.calls])
    z.update(ev_kind=np.array(ev["kind"], np.int8), ev_task=np.array(ev["task"], np.int32),
             ev_worker=np.array(ev["worker"], np.int32), ev_x=np.array(ev["x"], np.float64),
             ev_nbytes=np.array(ev["nbytes"], np.int64), ev_start=np.array(ev["start"]),
             ev_stop=np.array(ev["stop"]), ev_runid=np.array(ev["runid"], np.int64),
             hb_ptr=np.array(hb["ptr"], np.int64), hb_task=np.array(hb["task"], np.int32),
             hb_dur=np.array(hb["dur"], np.float64), ev_round_ptr=np.array(round_ptr, np.int64),
             rk_evptr=np.array(lo["rptr"], np.int64), rk_task=np.array(lo["rtask"], np.int32),
             rk_forget=np.array(lo["rforget"], np.uint8), rk_state=np.array(w.rk_state, np.uint8),
             bk_event=np.array(rel, np.int64), bk_n=np.array([c["n"] for c in w.calls], np.int64),
             bk_qlen=np.array([c["qlen"] for c in w.calls], np.int64), bk_qpos_ptr=qptr.astype(np.int64),
             bk_qpos=np.array([p for c in w.calls for p in c["qpos"]], np.int64),
             bk_npaused=np.array([c["npaused"] for c in w.calls], np.int64),
             bk_nlr=np.array([c["nlr"] for c in w.calls], np.int64),
             bk_nmulti=np.array([c["nmulti"] for c in w.calls], np.int64),
             bk_sens=np.array([c["sens"] for c in w.calls], np.int64), bk_search=np.array(search, np.int64),
             bk_key_ptr=np.cumsum([0] + [len(c["keys"]) for c in w.calls]).astype(np.int64),
             bk_key_row=np.array([r for c in w.calls for r in c["keys"]], np.int64))
    if w.mode in ("skew", "thin_skew"):  # the earlier streams keep the arrays they were committed with
        z.update({f"bk_{k}": np.array([c[k] for c in w.calls], np.int64)
                  for k in ("sens_idle", "sens_sat", "sens_cnt", "sens_net", "freed")})
        z.update(bk_idle=np.array([c["idle"] for c in w.calls], np.uint8),
                 bk_sat=np.array([c["sat"] for c in w.calls], np.uint8))
    np.savez_compressed(path, **z)
    print(f"{name}: {len(ev['kind'])} events, {len(w.calls)} release calls, plans {[c['n'] for c in w.calls][:12]}, "
          f"entry states {np.bincount(np.array(w.rk_state, np.int64), minlength=6).tolist()}, "
          f"sens {[c['sens'] for c in w.calls][:12]}, search {search}, {os.path.getsize(path) / 1e3:.0f} kB", flush=True)
    if w.mode in ("skew", "thin_skew"):
        print("   (sens, idle, sat, by count, by network, bytes freed) of the calls with a worker that depends on the place: "
              f"{[tuple(c[k] for k in ('sens', 'sens_idle', 'sens_sat', 'sens_cnt', 'sens_net', 'freed')) for c in w.calls if c['sens']]}",
              flush=True)


def c2var(n, w, seed):
    return lambda: G.graphs.random_dag(n, w, seed=seed, n_inner_prefixes=3, random_durations=True, nthreads="random")


CASES = {
    # name: (graph, saturation, seed, p_event, policy)
    "svcbulk_half_c2var_sat1.1": (c2var(3000, 48, 81), 1.1, 81, 0.04, "half"),
    "svcbulk_half_c2mini_satinf": (lambda: G.graphs.random_dag(2500, 40, seed=82), float("inf"), 82, 0.04, "half"),
    # early, while root tasks still queue: every queued task leaves the queue
    "svcbulk_all_c2var_sat1.1": (c2var(2500, 24, 83), 1.1, 83, 0.04, "all", 0.02),
    # mostly roots with few dependents each, early: queued tasks leave at the head, inside, at the tail
    "svcbulk_queue_sat1.1": (lambda: G.graphs.random_dag(2500, 24, seed=92, n_inner_prefixes=3, random_durations=True,
                                                         nthreads="random", root_frac=0.6), 1.1, 92, 0.04, "half", 0.02),
    "svcbulk_tail_sat1.1": (lambda: G.graphs.random_dag(2500, 24, seed=93, n_inner_prefixes=3, random_durations=True,
                                                        nthreads="random", root_frac=0.6), 1.1, 93, 0.04, "tail", 0.02),
    # events often enough that the call meets paused workers, a long-running task, replicas
    "svcbulk_all_c2mini_satinf": (lambda: G.graphs.random_dag(2000, 32, seed=84), float("inf"), 84, 0.15, "all"),
    "svcbulk_group_c2var_sat1.1": (c2var(3000, 48, 85), 1.1, 85, 0.04, "group"),
    # 70 workers: two words per who_has row
    "svcbulk_w70_sat1.1": (c2var(3000, 70, 86), 1.1, 86, 0.04, "half"),
    # worker restrictions, some tasks with no valid worker (no-worker)
    "svcbulk_restr_sat1.1": (lambda: G.graphs.restrict(c2var(2500, 24, 87)(), 0.2, seed=87), 1.1, 87, 0.04, "half", 0.05),
    # skew: the plan lists a few workers' exits first and then most of what the others process,
    # so check_idle_saturated of the first sees a total the end of the call no longer has.
    # Every task a sink, all processing after update_graph: nothing is fetched, the counts move it
    "svcbulk_skew_satinf": (lambda: G.graphs.random_dag(1200, 12, seed=94, root_frac=1.0, random_durations=True,
                                                        nthreads="random"), float("inf"), 94, 0.04, "skew", 0.0),
    # three layers, results of several GB (WIDE_CONFIG by the name): once the second layer is
    # done the third is processing and waits for fetches, which are most of the total. 48
    # workers: none needs more results at once than the engine's needs_what line holds
    "svcbulk_skew_wide_satinf": (lambda: G.graphs.widen(G.graphs.layered_dag(
        3, 500, 48, seed=95, fanins=(2, 3), n_inner_prefixes=3, random_durations=True, nthreads="random"), 95),
        float("inf"), 95, 0.15, "skew", 0.64),
    # a first call leaves three workers few tasks (still no fewer than threads); the skew call
    # after it lists them first: idle by half the average at their exit, not by the end's
    "svcbulk_skew_thin_satinf": (lambda: G.graphs.random_dag(1200, 12, seed=96, root_frac=1.0, nthreads="random"),
                                 float("inf"), 96, 0.04, "thin_skew", 0.0),
}


def main():
    only = set(sys.argv[1:])
    for name, (mk, sat, seed, p_event, mode, *early) in CASES.items():
        if only and name not in only:
            continue
        out = generate(name, mk, sat, seed, p_event, mode, *early)
        search = [0, 0]
        if name == "svcbulk_half_c2mini_satinf":
            # the stream the order-sensitivity search runs on: the first seed whose calls hold a
            # worker that check_idle_saturated would flag otherwise with the end-of-call total
            for k in range(SEARCH):
                sens = sum(c["sens"] for c in out[-1].calls)
                search = [k + 1, sens]
                if sens > 0:
                    break
                if k + 1 < SEARCH:
                    out = generate(name, mk, sat, seed + 1000 * (k + 1), p_event, mode)
        save(name, out, search)


if __name__ == "__main__":
    main()

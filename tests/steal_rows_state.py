"""A plugin state for ``StealRows`` on plain stand-ins of the reference's objects (no dask
needed), and the put / remove / re-put sequence that brings it to every shape of row the
plugin keeps: dependency rows longer than the slot row (KD), removals and slot reuse from
the free list, tasks put again (a recalculated cost: a later arrival), dependencies shared
and dropped, more holders than a dependency row keeps inline (HM), who_has cleared, unknown
task durations, restrictions. tests/test_steal_rows.py checks the rows against the full
rebuild after every phase; tests/test_gpu_steal_order.py hands the final state's problem to
the device.

CPU only; nothing here imports the engine."""
import numpy as np

from distributed_amd.stealing import StealRows


class NS:  # a plain stand-in, hashed by identity like TaskState / WorkerState
    def __init__(self, **kw):
        self.__dict__.update(kw)


class Sched:
    def __init__(self, W, rng):
        self.workers = {f"tcp://w{i:03d}": NS(address=f"tcp://w{i:03d}", nthreads=2, occupancy=float(rng.random()),
                                              processing={}, nbytes=int(rng.integers(0, 1000)))
                        for i in range(W)}
        self.idle = {a: ws for a, ws in list(self.workers.items())[:3]}
        self.saturated = set(list(self.workers.values())[-2:])
        self.total_occupancy, self.total_nthreads, self.bandwidth = 12.5, 2 * W, 100_000_000
        self.unknown_durations = {}

    def get_task_duration(self, ts):  # scheduler.py:3024-3041
        d = ts.prefix.duration_average
        if d >= 0:
            return d
        self.unknown_durations.setdefault(ts.prefix.name, set()).add(ts)
        return 0.5

    def valid_workers(self, ts):
        return {self.workers[a] for a in ts.worker_restrictions}


def task(key, prio, deps, prefix, ws, restr=None):
    return NS(key=key, priority=prio, dependencies=deps, prefix=prefix, processing_on=ws, worker_restrictions=restr,
              host_restrictions=None, resource_restrictions=None, loose_restrictions=False)


def new_state(W=16, hot=16, seed=7, restrict=0.05, unpackable=None):
    """Scheduler, plugin and empty rows, with 2000 tasks (not put yet) on the first ``hot`` of
    ``W`` workers and 300 data on any of them. ``unpackable``: the index of one task whose
    priority ``pack_priority`` cannot hold (its generation is 2**20), so that every
    ``rows.problem`` while it is in the rows takes the host-ranked route (``pk_bad``)."""
    rng = np.random.default_rng(seed)
    s = Sched(W, rng)
    wss = list(s.workers.values())
    prefixes = [NS(name=f"p{j}", duration_average=-1.0 if j == 2 else 0.01 * (j + 1)) for j in range(4)]
    data = [NS(key=("d", i), nbytes=int(rng.integers(-1, 10_000)), who_has={wss[int(h)] for h in
                                                                          rng.choice(W, int(rng.integers(1, 3)),
                                                                                     replace=False)})
            for i in range(300)]
    for d in data:
        d.get_nbytes = (lambda d=d: d.nbytes if d.nbytes >= 0 else 1024)
    plugin = NS(scheduler=s, key_stealable={}, in_flight_occupancy={wss[1]: 0.25}, in_flight_tasks={wss[1]: 1})
    tasks = []
    for i in range(2000):
        k = int(rng.choice([0, 1, 2, 3, 9, 17]))  # rows past KD = 4 as well
        deps = [data[int(j)] for j in rng.choice(300, k, replace=False)]
        ws = wss[int(rng.integers(0, hot))]
        restr = {wss[int(rng.integers(0, W))].address} if rng.random() < restrict else None
        prio = (0, 1 << 20, i) if i == unpackable else (0, int(rng.integers(0, 50)), i)
        tasks.append(task(("t", i), prio, deps, prefixes[int(rng.integers(0, 4))], ws, restr))
    return NS(rng=rng, s=s, wss=wss, data=data, plugin=plugin, rows=StealRows(), tasks=tasks)


def put(st, ts):
    level = int(st.rng.integers(1, 15))
    st.plugin.key_stealable[ts] = (ts.processing_on.address, level)
    st.rows.put(ts, ts.processing_on.address, level)


def remove(st, ts):
    st.plugin.key_stealable.pop(ts, None)
    st.rows.remove(ts)


def phases(st):
    """The sequence, one phase at a time: yields the phase's name once the phase is done."""
    tasks, data, wss, rows = st.tasks, st.data, st.wss, st.rows
    W = len(wss)
    for ts in tasks[:1500]:
        put(st, ts)
    yield "put"
    for ts in tasks[::3]:  # removals (free slots, dependencies dropped), then reuse
        remove(st, ts)
    yield "removed"
    for ts in tasks[1500:]:
        put(st, ts)
    for ts in tasks[1:1500:7]:  # a task put again (a recalculated cost) moves to the end of its ties
        put(st, ts)
    yield "reused and put again"
    # who_has changes through the scheduler's replica hooks (add_replica / remove_replica /
    # remove_all_replicas), which the plugin forwards to the rows
    for i, d in enumerate(data[:60]):
        ws = wss[(i * 5) % W]
        if i % 3 == 0 and len(d.who_has) > 1:
            h = sorted(d.who_has, key=lambda w: w.address)[0]
            d.who_has.discard(h)
            rows.replica(d, h.address, -1)
        elif i % 3 == 1:
            d.who_has.add(ws)
            rows.replica(d, ws.address, +1)
        else:
            for w in wss[:12]:  # more holders than a dependency row keeps inline
                d.who_has.add(w)
                rows.replica(d, w.address, +1)
    yield "replicas"
    for d in data[60:70]:
        for w in list(d.who_has):
            d.who_has.discard(w)
        rows.replicas_cleared(d)
    yield "replicas cleared"


def load_workers(st, hot=16, victim_occ=8.0, thief_step=0.001):
    """Worker columns under which a balance() of the state moves tasks: the first ``hot``
    workers (which run every task) saturated, their occupancy ``victim_occ`` and their
    ``processing`` the tasks they run; every other worker idle, one task (not in the rows)
    and ``k * thief_step`` of occupancy on the k-th, so no two thieves tie on stack time."""
    s, wss = st.s, st.wss
    for ws in wss:
        ws.processing = {}
    for ts in st.rows.slot:
        ts.processing_on.processing[ts] = 0.0
    for k, ws in enumerate(wss):
        if k < hot:
            ws.occupancy = victim_occ
        else:
            ws.processing = {("other", k): 0.0}
            ws.occupancy = (k - hot + 1) * thief_step
    s.idle = {ws.address: ws for ws in wss[hot:]}
    s.saturated = set(wss[:hot])
    s.total_occupancy = float(sum(ws.occupancy for ws in wss))
    s.total_nthreads = sum(ws.nthreads for ws in wss)

"""Seams of the extension (distributed_amd/ext.py) around no-worker tasks that need neither a
GPU nor the reference scheduler: a stand-in SchedulerState with ``unrunnable`` / ``valid_workers``
/ ``workers`` / ``running`` and a recording stand-in engine.

A worker that runs again (handle_worker_status_change, scheduler.py:5872-5878) has the
scheduler recommend the no-worker tasks it may take to processing
(bulk_schedule_unrunnable_after_adding_worker :3173-3186). The engine does not model that: the
extension evaluates the recommendation as the handler is about to and, if there is one, lets
the scheduler decide the stimulus and resynchronises, where the engine used to leave the tasks
unplaced and the first decision the scheduler asked for ended GPU placement for the session.
"""
from types import SimpleNamespace

import numpy as np

from distributed_amd.ext import GPUPlacementExtension


class _Hashable(SimpleNamespace):  # WorkerState / TaskState stand-ins live in sets
    __hash__ = object.__hash__


def _ws(address, status="running", nthreads=2):
    return _Hashable(address=address, nthreads=nthreads, status=SimpleNamespace(name=status))


class _Sched:
    _TRANSITIONS_TABLE = {("waiting", "processing"): lambda *a, **k: ("ref-wp",),
                          ("queued", "processing"): lambda *a, **k: ("ref-qp",),
                          ("no-worker", "processing"): lambda *a, **k: ("ref-np",)}
    WORKER_SATURATION = 1.1

    def __init__(self, addresses, restrictions):
        self.workers = {a: _ws(a) for a in addresses}
        self.running = set(self.workers.values())
        self.restrictions = restrictions  # key -> set of addresses (absent: unrestricted)
        self.tasks = {}
        self.unrunnable = set()
        self.idle, self.saturated, self.plugins, self.extensions = {}, set(), {}, {}
        self.idle_task_count = set()
        self.placed = []

    def task(self, key, priority, state="no-worker"):
        ts = _Hashable(key=key, priority=priority, state=state, dependencies=set(), dependents=set(),
                       worker_restrictions=self.restrictions.get(key), host_restrictions=None,
                       resource_restrictions=None, loose_restrictions=False, _rootish=None)
        self.tasks[key] = ts
        return ts

    def valid_workers(self, ts):  # scheduler.py:3043-3107, worker restrictions only
        r = self.restrictions.get(ts.key)
        if r is None:
            return None
        s = {self.workers[a] for a in r if a in self.workers}
        if not s:
            return set()
        if len(self.running) < len(self.workers):
            s &= self.running
        return s

    def is_rootish(self, ts):
        return False

    def _add_to_processing(self, ts, ws, stimulus_id):
        self.placed.append((ts.key, ws.address))
        return {}, {}, {}

    def add_replica(self, ts, ws):
        return None

    def remove_replica(self, ts, ws):
        return None


class _Engine:
    """Records the calls; ``to_place``: the (task, worker) placements the next call makes."""

    def __init__(self):
        self.calls, self.log, self.to_place = [], [], []

    def _place(self):
        self.log += self.to_place
        self.to_place = []

    def set_worker_status(self, worker, running):
        self.calls.append(("set_worker_status", worker, running))
        self._place()
        return 0

    def num_placements(self):
        return len(self.log)

    def placements(self, offset=0, count=None, columns=None):
        rows = self.log[offset:offset + count]
        return {"pl_task": np.array([t for t, _ in rows], np.int32), "pl_worker": np.array([w for _, w in rows], np.int32)}

    def sync_placements(self, *a):
        pass

    sync_tasks = sync_workers = sync_globals = sync_placements


def _setup():
    """Workers a, b, c in the engine's table, b paused. Tasks x0..x2 are no-worker: x1 restricted
    to b, x2 to d (absent); x0 unrestricted is added by the tests that want it."""
    s = _Sched(["a", "b", "c"], {"x1": {"b"}, "x2": {"d"}})
    s.workers["b"].status = SimpleNamespace(name="paused")
    s.running.discard(s.workers["b"])
    ext = GPUPlacementExtension(s)
    eng = ext.engine = _Engine()
    ext.keys = ["x0", "x1", "x2"]
    ext.task_index = {k: i for i, k in enumerate(ext.keys)}
    ext.workers, ext.worker_index = ["a", "b", "c"], {"a": 0, "b": 1, "c": 2}
    for key, prio in (("x1", (0, 3)), ("x2", (0, 5))):
        s.unrunnable.add(s.task(key, prio))
    return s, ext, eng


def test_resume_that_schedules_suspends():
    s, ext, eng = _setup()
    ws = s.workers["b"]
    ext._on_worker_status_change({"worker": "b", "status": "running"})
    # x1 may use b once b runs (valid_workers intersects with running, :3105-3106): the
    # scheduler decides, the engine is not asked, the resync follows
    assert eng.calls == [] and ext.active and ext.suspended
    assert "no-worker tasks" in ext.suspend_reason and ext.stats["resume_unrunnable"] == 1
    assert ws not in s.running  # adding it is the handler's
    # the transition is the scheduler's own, recorded with decide_worker_non_rootish's route
    s.tasks["x1"].dependencies = {object()}
    assert s._TRANSITIONS_TABLE[("no-worker", "processing")](s, "x1", "stim") == ("ref-np",)
    assert ext._route == 0
    assert type(s)._TRANSITIONS_TABLE[("no-worker", "processing")] is not s._TRANSITIONS_TABLE[("no-worker", "processing")]


def test_resume_of_a_worker_no_task_may_use_goes_to_the_engine():
    s, ext, eng = _setup()
    s.workers["c"].status = SimpleNamespace(name="paused")
    s.running.discard(s.workers["c"])
    ext._on_worker_status_change({"worker": "c", "status": "running"})
    # neither x1 (b) nor x2 (d) may use c: nothing is recommended, the device follows the resume
    assert eng.calls == [("set_worker_status", 2, 1)]
    assert ext.active and not ext.suspended and ("queued", "processing") in ext._window[0]


def test_resume_with_an_unrestricted_no_worker_task_suspends():
    s, ext, eng = _setup()
    s.workers["c"].status = SimpleNamespace(name="paused")
    s.running.discard(s.workers["c"])
    s.unrunnable.add(s.task("x0", (0, 9)))  # valid_workers None: any worker that runs may take it
    ext._on_worker_status_change({"worker": "c", "status": "running"})
    assert eng.calls == [] and ext.suspended


def test_pause_and_resume_without_unrunnable_tasks_are_unchanged():
    s, ext, eng = _setup()
    s.unrunnable.clear()
    ext._on_worker_status_change({"worker": "b", "status": "running"})
    s.workers["b"].status = SimpleNamespace(name="running")
    ext._on_worker_status_change({"worker": "b", "status": "paused"})
    assert eng.calls == [("set_worker_status", 1, 1), ("set_worker_status", 1, 0)]
    assert not ext.suspended


def test_route_of_a_no_worker_decision():
    s, ext, eng = _setup()
    ts = s.tasks["x1"]
    s.is_rootish = lambda ts: True
    # decide_worker_non_rootish whatever the task (:2128): restricted -> route 0, never a root-ish route
    assert ext._route_of(s, ts, False, non_rootish=True) == 0 and ext._route_of(s, ts, False) == 1

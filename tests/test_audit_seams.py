"""Seams of the state audit between the extension and the engine (distributed_amd/ext.py
``audit`` / ``_audit_validate`` / ``_audit_due``, engine.py ``audit_state``) that need neither
a GPU nor the reference scheduler: a stand-in scheduler and engine doubles, as in
test_ext_seams.py.
"""
import ctypes as C
import sys
import time
import types
from types import SimpleNamespace

import pytest

from distributed_amd import _lib, config, engine
from distributed_amd.engine import Violation, ViolationList
from distributed_amd.ext import GPUPlacementExtension

BAD = Violation("WORKER_NPROC", "nproc", 3, -1, 2, 1)


class _Queued:
    def sorted(self):
        return []


class _Sched:
    _TRANSITIONS_TABLE = {("waiting", "processing"): lambda *a, **k: None,
                          ("queued", "processing"): lambda *a, **k: None}

    def __init__(self):
        self.workers, self.tasks, self.plugins = {}, {}, {}
        self.idle, self.saturated, self.running = {}, set(), set()
        self.extensions = {}
        # what sync.global_rows reads
        self._task_prefix_count_global, self.task_prefixes, self.task_groups = {}, {}, {}
        self.n_tasks, self._network_occ_global, self.bandwidth = 0, 0, 1e8
        self.queued = _Queued()

    def _add_to_processing(self, ts, ws, stimulus_id):
        return None

    def add_replica(self, ts, ws):
        return None

    def remove_replica(self, ts, ws):
        return None


class _Engine:
    """An engine double with the resync entry points and a scripted audit."""

    def __init__(self, found=()):
        self.found = ViolationList(found)
        self.found.total = len(self.found)
        self.calls = []

    def audit_state(self, cap=64):
        self.calls.append("audit_state")
        return self.found, 0

    def num_placements(self):
        return 0

    def sync(self, placements, tasks, workers, globals_):
        self.calls.append("sync")

    def sync_placements(self, *a):
        pass

    sync_tasks = sync_workers = sync_globals = sync_placements


class _NoAudit:
    def num_placements(self):
        return 0


def _extension(eng, **kw):
    ext = GPUPlacementExtension(_Sched(), **kw)
    ext.engine = eng
    ext.group_index, ext.prefix_dur = {}, []
    return ext


def test_audit_returns_what_the_engine_reports():
    eng = _Engine([BAD])
    ext = _extension(eng)
    assert ext.audit() == [BAD] and eng.calls == ["audit_state"]
    assert ext.active  # audit() itself only reports
    clean = _extension(_Engine())
    assert clean.audit() == [] and clean.audit(full=True) == []


def test_full_audit_runs_the_scheduler_rows_through_audit_rows():
    """audit(full=True): the rows a resync would send (sync.task_rows / worker_rows /
    global_rows of every engine task and worker) go to the engine's audit_rows, and its
    records join the self-audit's."""
    row = Violation("ROW_TASKS", "waiters", 0, -1, 1, 2)
    eng = _Engine([BAD])
    seen = {}

    def audit_rows(tasks, workers, globals_, cap=64):
        seen.update(tasks=tasks, workers=workers, globals=globals_)
        out = ViolationList([row])
        out.total = 1
        return out

    eng.audit_rows = audit_rows
    ext = _extension(eng)
    found = ext.audit(full=True)
    assert list(found) == [BAD, row] and found.total == 2
    assert set(seen["tasks"]) >= {"task", "state", "holder_ptr"} and "needs_ptr" in seen["workers"]
    assert "queued" in seen["globals"]
    assert ext.audit() == [BAD]  # without full the rows are not read
    assert list(_extension(_Engine([BAD])).audit(full=True)) == [BAD]  # an engine without audit_rows


def test_engine_without_the_method_is_skipped():
    ext = _extension(_NoAudit(), validate=True, audit_interval=1e-6)
    assert ext.audit() == []
    ext._last_audit = time.monotonic() - 1
    ext._enter()  # the interval ran out: nothing to ask, nothing falls back
    assert ext.active


def test_no_audit_while_the_scheduler_decides():
    """Suspended (the engine awaits its resync) or with a batch posted, the engine's state is
    not the scheduler's: no audit."""
    eng = _Engine([BAD])
    ext = _extension(eng)
    ext.suspended = True
    assert ext.audit() == [] and eng.calls == []


def test_validate_raises_on_a_violation_after_resync():
    eng = _Engine([BAD])
    ext = _extension(eng, validate=True)
    ext.suspended, ext.suspend_reason = True, "test"
    with pytest.raises(AssertionError, match="WORKER_NPROC"):
        ext._resync()
    assert eng.calls == ["sync", "audit_state"]
    # consistent state: the resync ends quietly, and without validate nothing is audited
    ok = _Engine()
    ext = _extension(ok, validate=True)
    ext.suspended, ext.suspend_reason = True, "test"
    ext._resync()
    assert ok.calls == ["sync", "audit_state"] and ext.active and not ext.suspended
    quiet = _Engine([BAD])
    ext = _extension(quiet)
    ext.suspended, ext.suspend_reason = True, "test"
    ext._resync()
    assert quiet.calls == ["sync"] and ext.active


def test_validate_audits_after_a_followed_release():
    eng = _Engine([BAD])
    eng.release_tasks = lambda t, f: 0
    eng.placements = lambda *a, **k: {"pl_task": [], "pl_worker": []}
    ext = _extension(eng, validate=True)
    with pytest.raises(AssertionError, match="release_tasks"):
        ext._engine_op("release_tasks", [0], [0])


def test_audit_interval_falls_back_with_the_record():
    eng = _Engine([BAD])
    ext = _extension(eng, audit_interval=30.0)
    ext._enter()  # the interval has not run out
    assert eng.calls == [] and ext.active
    ext._last_audit = time.monotonic() - 31
    ext._enter()
    assert eng.calls == ["audit_state"] and not ext.active
    assert "WORKER_NPROC" in ext.reason and "index=3" in ext.reason
    # off by default
    eng = _Engine([BAD])
    ext = _extension(eng)
    ext._last_audit = time.monotonic() - 1e6
    ext._enter()
    assert eng.calls == [] and ext.active


def test_settings_reads_the_knob(monkeypatch):
    store = {}

    def update_defaults(d):
        def walk(prefix, x):
            for k, v in x.items():
                if isinstance(v, dict):
                    walk(prefix + k + ".", v)
                else:
                    store.setdefault(prefix + k, v)
        walk("", d)

    cfg = SimpleNamespace(update_defaults=update_defaults, get=lambda k, default=None: store.get(k, default))
    dask = types.ModuleType("dask")
    dask.config = cfg
    monkeypatch.setitem(sys.modules, "dask", dask)
    store["distributed.scheduler.work-stealing"] = True
    st = config.settings()
    assert st["audit_interval"] == 0 and st["validate"] is False
    store["distributed.scheduler.gpu-placement.audit-interval"] = 2.5
    assert config.settings()["audit_interval"] == 2.5


def test_lib_declares_the_audit():
    assert _lib.ABI_VERSION == 22
    res, args = _lib.SIGNATURES["dgp_audit_state"]
    assert res is C.c_int and len(args) == 5 and args[1] is C.c_int64
    # the row audits take their dgp_sync_* arguments plus cap, out, n_violations
    for kind in ("tasks", "workers", "globals"):
        r_, a_ = _lib.SIGNATURES[f"dgp_audit_{kind}"]
        assert r_ is C.c_int and a_[:-3] == _lib.SIGNATURES[f"dgp_sync_{kind}"][1] and a_[-3] is C.c_int64, kind
    assert C.sizeof(engine._CViolation) == 40  # struct dgp_violation
    hdr = open(_lib.PKG + "/../include/dgplace.h").read()
    assert "#define DGP_ABI_VERSION 22" in hdr
    # the names the Python side decodes are the header's enums, id for id
    for i, name in engine.AUDIT_RULES.items():
        assert f"DGP_AR_{name} = {i}" in hdr, name
    for i, name in engine.AUDIT_FIELDS.items():
        assert f"DGP_AF_{name.upper()} = {i}" in hdr, name

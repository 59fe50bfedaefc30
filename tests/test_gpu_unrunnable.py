"""No-worker tasks on the engine (needs an MI355X): what it counts and what it leaves to the
scheduler.

A task is no-worker while no running worker may take it. The update_graph stimulus puts a
restricted task whose valid set is empty there and counts it (``Ctl.n_unrunnable``, read by
``dgp_num_unrunnable``). The reference empties the state when a worker joins
(scheduler.py:4416-4420) or runs again (:5872-5878) through
``bulk_schedule_unrunnable_after_adding_worker`` (:3173-3186); the engine models neither: a join
while the count is not 0 is refused (``dgp_add_worker(_at)``, DGP_E_STATE) and a resume is the
scheduler's own stimulus (the extension suspends and resynchronises,
``tests/test_unrunnable_seams.py``).

The expectations come from the oracle's replay of the same graph, which leaves the same tasks
unplaced; the CPU-side preconditions are asserted first.
"""
import numpy as np
import pytest

from oracle import oracle

pytestmark = pytest.mark.gpu

BASE_CFG = {"bandwidth": 100_000_000, "default_data_size": 1024, "unknown_duration": 0.5}
S_PROCESSING, S_NO_WORKER, S_MEMORY = 2, 4, 5
W0 = 12          # workers of the base graph, one thread each
N0 = 1200        # its tasks; the first 480 are roots (one root-ish group)
NTHREADS_NEW = 4
N_FREE = 20      # extra tasks without dependencies
N_DEP = 20       # extra tasks depending on one or two early roots


def cfg_of(sat):
    return dict(BASE_CFG, saturation=sat)


def base_graph(n_workers=W0, seed=8101):
    from distributed_amd import graphs

    return graphs.random_dag(N0, n_workers, seed=seed, n_inner_prefixes=2, random_durations=True, root_frac=0.4)


def with_extra(g, dep_rows, valid_rows, dur=-1.0):
    """``g`` plus len(dep_rows) extra tasks R under their own prefix "extra" (default duration
    ``dur``) and group, priorities after all of ``g``, restricted (not loose) to ``valid_rows``
    (worker indices, ascending; empty: no worker of the cluster). Returns (graph, R indices)."""
    n, k = g["n_tasks"], len(dep_rows)
    P, Gn = len(g["prefix_default_dur"]), len(g["group_prefix"])
    G = dict(g)
    ptr = np.cumsum([0] + [len(r) for r in dep_rows]) + int(g["dep_ptr"][-1])
    G["dep_ptr"] = np.concatenate([g["dep_ptr"], ptr[1:]]).astype(np.int64)
    G["dep_idx"] = np.concatenate([g["dep_idx"]] + [np.asarray(sorted(r), np.int32) for r in dep_rows]).astype(np.int32)
    G["prio"] = np.concatenate([g["prio"], int(g["prio"].max()) + 1 + np.arange(k)]).astype(np.int64)
    G["prefix_id"] = np.concatenate([g["prefix_id"], np.full(k, P)]).astype(np.int32)
    G["group_id"] = np.concatenate([g["group_id"], np.full(k, Gn)]).astype(np.int32)
    G["wanted"] = np.concatenate([g["wanted"], np.ones(k)]).astype(np.uint8)
    G["rootish_override"] = np.concatenate([g["rootish_override"], np.full(k, -1)]).astype(np.int8)
    G["nbytes"] = np.concatenate([g["nbytes"], np.full(k, 1000)]).astype(np.int64)
    G["start"] = np.concatenate([g["start"], np.zeros(k)])
    G["stop"] = np.concatenate([g["stop"], np.full(k, 0.01)])
    G["prefix_names"] = list(g["prefix_names"]) + ["extra"]
    G["group_names"] = list(g["group_names"]) + ["extra-0a1b2c3d4e5f60718293a4b5c6d7e8f9"]
    G["group_prefix"] = np.concatenate([g["group_prefix"], [P]]).astype(np.int32)
    G["prefix_default_dur"] = np.concatenate([g["prefix_default_dur"], [dur]])
    G["n_tasks"] = n + k
    flags = np.zeros(n + k, np.uint8) if g.get("restr_flags") is None else np.concatenate([g["restr_flags"], np.zeros(k, np.uint8)])
    flags[n:] = 1
    old_ptr = np.zeros(n + 1, np.int64) if g.get("restr_flags") is None else np.asarray(g["restr_ptr"], np.int64)
    old_idx = np.zeros(0, np.int32) if g.get("restr_flags") is None else np.asarray(g["restr_idx"], np.int32)
    rp = np.cumsum([0] + [len(r) for r in valid_rows]) + int(old_ptr[-1])
    G["restr_ptr"] = np.concatenate([old_ptr, rp[1:]]).astype(np.int64)
    G["restr_idx"] = np.concatenate([old_idx] + [np.asarray(sorted(r), np.int32) for r in valid_rows]).astype(np.int32)
    G["restr_flags"] = flags
    return G, np.arange(n, n + k, dtype=np.int32)


_REF = {}


def reference(key, build):
    """(graph, R, config, oracle replay) of a case: computed once, shared, never modified."""
    if key not in _REF:
        G, R, cfg = build()
        ref = oracle.replay(G, cfg)
        # the oracle leaves exactly R unplaced, in no-worker
        placed = np.zeros(G["n_tasks"], bool)
        placed[np.asarray(ref["pl_task"])] = True
        assert not placed[R].any() and placed[:G["n_tasks"] - len(R)].all(), key
        assert (np.asarray(ref["final_state"])[R] == S_NO_WORKER).all(), key
        _REF[key] = (G, R, cfg, ref)
    return _REF[key]


def case_free(sat, n_free=N_FREE, dur=-1.0, n_workers=W0):
    return reference(("free", sat, n_free, dur, n_workers),
                     lambda: with_extra(base_graph(n_workers), [[]] * n_free, [[]] * n_free, dur) + (cfg_of(sat),))


def no_violation(eng):
    v, _ = eng.audit_state()
    assert v.total == 0, list(v)[:4]


@pytest.fixture(scope="module")
def engine_cls():
    from distributed_amd.engine import PlacementEngine

    return PlacementEngine


def test_update_graph_counts_the_no_worker_tasks(engine_cls):
    G, R, cfg, ref = case_free(1.1)
    first = int(ref["round_nplaced"][0])
    with engine_cls(0) as eng:
        eng.load(G, cfg, results=False)
        eng.update_graph()
        assert eng.num_placements() == first and eng.num_unrunnable() == len(R)
        assert (eng.task_states()[R] == S_NO_WORKER).all()
        no_violation(eng)
    G, R, cfg, ref = case_free(1.1, n_free=2)
    with engine_cls(0) as eng:
        eng.load(G, cfg, results=False)
        eng.update_graph()
        assert eng.num_unrunnable() == 2


def test_join_while_tasks_are_no_worker_is_refused(engine_cls):
    """``add_worker`` while tasks are no-worker is DGP_E_STATE with nothing changed; the error
    carries its code."""
    from distributed_amd import _lib

    G, R, cfg, ref = case_free(1.1)
    first = int(ref["round_nplaced"][0])
    with engine_cls(0) as eng:
        eng.load(G, cfg, results=False)
        eng.update_graph()
        for position in (None, 5):
            with pytest.raises(_lib.DgpError, match=r"\(-3\).*no-worker tasks would be rescheduled \(not modelled\)") as ei:
                eng.add_worker(NTHREADS_NEW, position=position)
            assert ei.value.code == -3
        assert eng.n_workers == W0 and eng.num_unrunnable() == len(R) and eng.num_placements() == first
        no_violation(eng)


def test_join_without_no_worker_tasks_is_unchanged(engine_cls):
    g = base_graph()
    cfg = cfg_of(1.1)
    with engine_cls(0) as eng:
        eng.load(g, cfg, results=False)
        eng.update_graph()
        assert eng.num_unrunnable() == 0
        assert eng.add_worker(NTHREADS_NEW) == 5  # its 5 slots take the queue's head
        assert eng.num_unrunnable() == 0
        no_violation(eng)

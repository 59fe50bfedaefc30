"""Worker joins that renumber what the engine holds (needs an MI355X).

``dgp_add_worker_at`` at a position below the worker count shifts the per-worker rows,
``holder_of`` / ``proc_on``, the ``who_has`` bitsets (``k_insert_worker_remap``: one bit up
from the position, carried across 64-bit words), the groups' last worker and the restriction
rows, the static CSR as well as the run-time pool of ``dgp_update_restrictions``. The
reference-generated ``svcaddw_ins*`` streams run through tests/test_gpu_service.py like every
join fixture; here

* the same streams run with every restricted task's row restated through
  ``update_restrictions`` first, so the rows the decisions read are the pool's and the pool
  branch of the remap is what keeps them right;
* a sweep of small restricted graphs joins six workers at positions 0, W, alternately 0 and
  W - 1 and at random, from 1, 2, 63, 64 and 127 workers (bitsets of one word, growing to
  two, of two, growing to three), against the oracle (oracle/replay.cpp, whose insertion is
  pinned to the reference by tests/test_oracle_golden.py);
* one unrestricted graph does the same on the 32-slot build of the stream kernel.

Every comparison is bit for bit: placements, per-round snapshots, final task states.
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from join_census import relabel
from oracle import oracle
from test_gpu_parity import PL_KEYS, ROUND_KEYS, assert_same

pytestmark = pytest.mark.gpu

CFG = {"bandwidth": 100_000_000, "default_data_size": 1024, "unknown_duration": 0.5}
N_JOIN = 6


def run_stream(g, cfg, exp, msgs, ptr, add_at, per_message=False, after_update=None, window=None):
    """The stream through dgp_tasks_finished, one call per message or per round (batches end
    at the next join), the events of ``add_at`` (message index -> [(nthreads, position,
    running)], running = 2: a paused joiner at ``position`` resumes) before their message."""
    from distributed_amd.engine import PlacementEngine

    R = len(exp["round_nplaced"]) + 2
    status = []
    with PlacementEngine(0) as eng:
        eng.load(g, cfg, snapshots=R, results=False)
        eng.update_graph()
        if after_update is not None:
            after_update(eng)
        if window is not None:
            assert eng.get_window() == window
        for k in range(len(ptr) - 1):
            i, e = ptr[k], ptr[k + 1]
            while i < e:
                for nt, p_, r_ in add_at.get(i, ()):
                    n0 = eng.num_placements()
                    newp = eng.set_worker_status(p_, 1) if r_ == 2 else eng.add_worker(nt, running=bool(r_), position=p_)
                    assert eng.num_placements() == n0 + newp
                j = i + 1
                if not per_message:
                    while j < e and j not in add_at:
                        j += 1
                st, _ = eng.tasks_finished(*(np.array(c) for c in zip(*msgs[i:j])))
                status.extend(st.tolist())
                i = j
            if e > ptr[k]:
                eng.snapshot()
        out = eng.placements()
        out.update(eng.snapshots(R))
        out["final_state"] = eng.task_states()
        n_workers = eng.n_workers
    assert (np.array(status) == 0).all()
    return out, n_workers


# ------------------------------------------------------------- 1. pool rows across insertions
@pytest.mark.parametrize("name", ["svcaddw_insrestr_sat1.1", "svcaddw_insq_sat1.1", "svcaddw_insrestr_satinf",
                                  "svcaddw_ins64_sat1.1"])
def test_restated_rows_follow_the_insertions(name):
    """Right after update_graph every restricted task's own row and flags are restated
    (Scheduler.set_restrictions with unchanged values makes no transition, scheduler.py
    :7702-7707, so the reference's stream is still the expected output). From then on the
    engine reads the rows from its pool, and every insertion has to renumber them there.
    All restricted tasks are restated, the ones already processing too: the restatement
    writes a task's row offset and flags and nothing else."""
    path = os.path.join(GOLDEN, name + ".npz")
    g, cfg, exp, meta = oracle.load_fixture(path)
    z = np.load(path, allow_pickle=False)
    msgs = list(zip(*(z[k].tolist() for k in ("msg_task", "msg_worker", "msg_runid", "msg_nbytes", "msg_start", "msg_stop"))))
    add_at = {}
    for i, nt, p_, r_ in zip(z["add_msg"].tolist(), z["add_nthreads"].tolist(), z["add_pos"].tolist(), z["add_running"].tolist()):
        add_at.setdefault(i, []).append((nt, p_, r_))
    for i, w in zip(z["res_msg"].tolist(), z["res_worker"].tolist()):
        add_at.setdefault(i, []).append((0, w, 2))
    rp, ri, rf = g["restr_ptr"], g["restr_idx"], g["restr_flags"]
    ts = np.flatnonzero(rf & 1)
    assert len(ts) > 100

    def restate(eng):
        eng.update_restrictions(ts, [ri[rp[t]:rp[t + 1]] for t in ts], rf[ts])

    out, W = run_stream(g, cfg, exp, msgs, z["msg_round_ptr"].tolist(), add_at, after_update=restate, window=64)
    assert W == len(g["nthreads"]) + len(z["add_nthreads"])
    assert_same(out, exp, PL_KEYS + ROUND_KEYS)
    assert np.array_equal(out["final_state"], exp["final_state"])


# ------------------------------------------------------------------ 2. sweep against the oracle
def positions(pattern, W0, rng):
    W = W0 + np.arange(N_JOIN)  # the worker count at each join
    if pattern == "first":
        return np.zeros(N_JOIN, np.int64)
    if pattern == "append":
        return W
    if pattern == "alternate":
        return np.where(np.arange(N_JOIN) % 2 == 0, 0, W - 1)
    return rng.integers(0, W + 1)


def oracle_stream(g, cfg, W0, before, nthreads, pos):
    """The oracle's run with the joins, and the message stream it implies: completion i
    reports placement i from the index its worker has at that moment."""
    ref = oracle.replay(g, cfg, joins=(before, nthreads, pos))
    n = len(ref["pl_task"])
    assert n == g["n_tasks"]
    labels = relabel(W0, pos.tolist(), ref["join_placed"].tolist(), ref["pl_worker"]).tolist()
    order, k, msgs, add_at = list(range(W0)), 0, [], {}
    for i in range(n):
        while k < N_JOIN and before[k] <= i:
            order.insert(int(pos[k]), W0 + k)
            add_at.setdefault(i, []).append((int(nthreads[k]), int(pos[k]), 1))
            k += 1
        t = int(ref["pl_task"][i])
        msgs.append((t, order.index(labels[i]), i, int(g["nbytes"][t]), float(g["start"][t]), float(g["stop"][t])))
    assert k == N_JOIN
    ptr = np.concatenate([[0], np.cumsum(ref["round_nplaced"])]).tolist()
    return ref, msgs, ptr, add_at


SWEEP = [(W0, sat, pattern, seed) for W0 in (1, 2, 63, 64, 127) for sat in (1.1, "inf")
         for pattern, seed in (("first", 1), ("append", 2), ("alternate", 3), ("rng", 4), ("rng", 5))]


@pytest.mark.parametrize("W0,sat,pattern,seed", SWEEP, ids=[f"w{a}-sat{b}-{c}{d}" for a, b, c, d in SWEEP])
def test_joins_at_any_position_match_the_oracle(W0, sat, pattern, seed):
    from distributed_amd import graphs

    g = graphs.restrict(graphs.random_dag(800, W0, seed=100 + seed, n_inner_prefixes=3, random_durations=True,
                                          nthreads="random"), 0.3, seed=seed, max_valid=min(4, W0), empty_frac=0.0)
    cfg = dict(CFG, saturation=sat)
    rng = np.random.default_rng(seed)
    before = np.sort(rng.choice(g["n_tasks"] // 2, N_JOIN, replace=False)).astype(np.int64)
    nthreads = rng.integers(1, 5, N_JOIN).astype(np.int32)
    pos = positions(pattern, W0, rng).astype(np.int32)
    ref, msgs, ptr, add_at = oracle_stream(g, cfg, W0, before, nthreads, pos)
    # not vacuous: restricted tasks are placed after the last join
    later = ref["pl_task"][int(ref["join_placed"][-1]):]
    assert (g["restr_flags"][later] & 1).sum() >= 10
    out, W = run_stream(g, cfg, ref, msgs, ptr, add_at, window=64)
    assert W == W0 + N_JOIN
    assert_same(out, ref, PL_KEYS + ROUND_KEYS)
    assert np.array_equal(out["final_state"], ref["final_state"])


# -------------------------------------------------------------------------- 3. 32-slot window
def test_insertions_across_64_workers_on_the_32_slot_build():
    """An unrestricted graph keeps the 32-slot build (a restricted one picks the 64-slot build
    on its own): 63 workers growing to 69, with the join from 64 to 65 inserting at 6 (the
    bitsets grow to two words in the same call), then joins at 0, twice at 64 and an append."""
    from distributed_amd import graphs

    W0 = 63
    g = graphs.random_dag(800, W0, seed=7, n_inner_prefixes=3, random_durations=True, nthreads="random")
    cfg = dict(CFG, saturation=1.1)
    rng = np.random.default_rng(7)
    before = np.sort(rng.choice(g["n_tasks"] // 2, N_JOIN, replace=False)).astype(np.int64)
    nthreads = rng.integers(1, 5, N_JOIN).astype(np.int32)
    pos = np.array([5, 6, 0, 64, 64, 68], np.int32)
    ref, msgs, ptr, add_at = oracle_stream(g, cfg, W0, before, nthreads, pos)
    assert len(ref["pl_task"]) - int(ref["join_placed"][-1]) >= 100
    out, W = run_stream(g, cfg, ref, msgs, ptr, add_at, window=32)
    assert W == W0 + N_JOIN
    assert_same(out, ref, PL_KEYS + ROUND_KEYS)
    assert np.array_equal(out["final_state"], ref["final_state"])

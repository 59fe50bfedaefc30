"""The stream executor's taken path and each of its out-of-line fallbacks against the oracle
(needs an MI355X).

``exe_local`` keeps its common case inline and calls cold handlers for the rest: the
one-at-a-time needs_what loops (overflow entries, scan mode), the ``exact`` continuation, the
restricted-candidate loop, the ``nthreads != 1`` divisions and the duration row past 8
prefixes. A rare branch left wrong by such a split passes every common case, so each handler
gets the smallest graph that provably reaches it: the guard is asserted first, on the CPU, on
the oracle's log alone (``tests/stimulus_census.py``); then both stream-window builds (32, 64)
replay the graph and the placement log, every round's snapshot and the final task states are
compared with ``oracle.replay`` bit for bit.
"""
import numpy as np
import pytest

from oracle import oracle
from stimulus_census import NE, REASONS, scan_mode_refills, stimulus_census

pytestmark = pytest.mark.gpu

PL_KEYS = ("pl_task", "pl_worker", "pl_comm", "pl_start", "pl_wsnbytes", "pl_route")
ROUND_KEYS = ("round_nplaced", "round_occ", "round_wnbytes", "round_nproc", "round_idle", "round_sat",
              "round_itc", "round_nqueued")
WINDOWS = (32, 64)
BASE_CFG = {"bandwidth": 100_000_000, "default_data_size": 1024, "unknown_duration": 0.5}
LOCAL = REASONS.index("local")
LINE_CAP = 11  # entries of a worker's needs_what line in LDS; more go to overflow entries
SCAN_CAP = 63  # line + overflow entries; more puts the worker in scan mode


def build_case(name):
    """(graph, config) of a named case; deterministic."""
    from distributed_amd import graphs

    sat = 1.1
    if name == "overflow":
        g = graphs.layered_dag(8, 48, 6, seed=1, fanins=(7, 8), span=2, n_inner_prefixes=3, random_durations=True,
                               nthreads=2)
    elif name == "scan_exact":
        g = graphs.layered_dag(10, 120, 5, seed=2, fanins=(7, 8), span=2, n_inner_prefixes=3, random_durations=True,
                               nthreads=2)
    elif name == "plain":
        g = graphs.random_dag(5000, 64, seed=7)
    elif name == "plain_nth2":
        g = graphs.random_dag(5000, 64, seed=7, nthreads=2)
    elif name == "plain_p16":
        g = graphs.random_dag(5000, 64, seed=7, n_inner_prefixes=15)
    elif name == "plain_satinf":
        g, sat = graphs.random_dag(5000, 64, seed=7), "inf"
    elif name == "restricted":
        g = graphs.restrict(graphs.random_dag(5000, 64, seed=7), 0.3, seed=1)
    elif name in ("fanin4", "fanin5"):
        g = graphs.random_dag(3000, 32, seed=7, fanin=int(name[-1]))
    else:
        raise KeyError(name)
    return g, dict(BASE_CFG, saturation=sat)


CASES = ("overflow", "scan_exact", "plain", "plain_nth2", "plain_p16", "plain_satinf", "restricted", "fanin4",
         "fanin5")

_REF = {}
_CHECKED = set()


def reference(name):
    """The case's graph, config and oracle replay: computed once, shared, never modified."""
    if name not in _REF:
        g, cfg = build_case(name)
        ref = oracle.replay(g, cfg)
        # (restrictions leave some tasks of "restricted" without a valid worker: never placed)
        assert len(ref["pl_task"]) == g["n_tasks"] or name == "restricted"
        _REF[name] = (g, cfg, ref)
    return _REF[name]


def restricted_placed_locally(g, ref, sat):
    """Restricted tasks that the replay places and that are made ready by a completion the
    prefetcher leaves local: the executor decides them from the candidates the descriptor
    lists. The census walk does not model a restricted task's candidate entries (at most one
    per valid worker, after the task's dependency entries), so a stimulus counts only if the
    entries the walk counted plus every valid worker of every restricted task it makes ready
    still leave a quarter of the descriptor free: local on the device whatever the resolved
    candidates are."""
    c = stimulus_census(g, ref, sat)
    ptr, idx = np.asarray(g["dep_ptr"]), np.asarray(g["dep_idx"])
    restr = np.asarray(g["restr_flags"]) != 0
    n_valid = np.diff(np.asarray(g["restr_ptr"]))
    placed = np.zeros(g["n_tasks"], bool)
    pt = np.asarray(ref["pl_task"])
    placed[pt[pt >= 0]] = True
    left = np.diff(ptr).copy()
    dependents = [[] for _ in range(g["n_tasks"])]
    for x in range(g["n_tasks"]):
        for d in idx[ptr[x]:ptr[x + 1]].tolist():
            dependents[d].append(x)
    n = 0
    for r, t in enumerate(pt.tolist()):
        ready = []
        for x in dependents[t] if t >= 0 else ():
            left[x] -= 1
            if left[x] == 0:
                ready.append(x)
        rr = [x for x in ready if restr[x]]
        room = c["n"][r] + sum(int(n_valid[x]) for x in rr) <= NE - NE // 4
        if c["reason"][r] == LOCAL and room and all(n_valid[x] > 0 for x in rr):
            n += sum(bool(placed[x]) for x in rr)
    return n


def check_shape(name, g, cfg, ref):
    """The CPU-side guards: the oracle's own replay reaches the path the case is for."""
    sat = cfg["saturation"]
    if name == "overflow":
        # local stimuli on a worker past the 11-entry line, none of them in scan mode
        assert scan_mode_refills(g, ref, sat, LINE_CAP)[1] > 0
        assert scan_mode_refills(g, ref, sat, SCAN_CAP) == (0, 0)
    elif name == "scan_exact":
        assert scan_mode_refills(g, ref, sat, SCAN_CAP)[0] >= 5
    elif name.startswith("plain"):
        c = stimulus_census(g, ref, sat)
        assert len(c["reason"]) == g["n_tasks"] == 5000 and (c["reason"] == LOCAL).all()
        if name == "plain_nth2":
            assert set(np.asarray(g["nthreads"]).tolist()) == {2}
        if name == "plain_p16":
            assert len(g["prefix_names"]) == 16
    elif name == "restricted":
        assert restricted_placed_locally(g, ref, sat) > 0
    else:
        k = int(name[-1])
        c = stimulus_census(g, ref, sat)
        assert ((c["kt"] == k) & (c["reason"] == LOCAL)).any()
        assert c["kt"].max() == k  # the other side of the unroll's edge comes from the other case
        # the same tasks as frontier tasks of local stimuli: the comm loop and the commit's
        # whole-line update at the edge of their unrolled run (fan-in 5: the remainder loop)
        assert k in c["kx_local"].tolist()


@pytest.fixture(scope="module")
def engine_cls():
    from distributed_amd.engine import PlacementEngine

    return PlacementEngine


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("name", CASES)
def test_exe_paths_match_oracle(engine_cls, name, window):
    g, cfg, ref = reference(name)
    if name not in _CHECKED:  # the guards depend on the oracle's log alone: once per case
        check_shape(name, g, cfg, ref)
        _CHECKED.add(name)
    R = ref["n_rounds"] + 2
    with engine_cls(0, window=window) as eng:
        eng.load(g, cfg, snapshots=R)
        eng.replay()
        out = eng.placements()
        out.update(eng.snapshots(R))
        out["final_state"] = eng.task_states()
    for k in PL_KEYS + ROUND_KEYS:
        a, b = np.asarray(out[k]), np.asarray(ref[k])
        assert a.shape == b.shape, (name, k, a.shape, b.shape)
        bad = np.flatnonzero(a.reshape(-1) != b.reshape(-1))
        assert len(bad) == 0, f"{name} {k}: {len(bad)} mismatches, first at {bad[0]}"
    assert np.array_equal(out["final_state"], ref["final_state"]), name

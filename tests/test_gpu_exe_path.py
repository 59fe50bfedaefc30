"""The stream executor's per-stimulus path against the oracle (needs an MI355X).

Each case is a 1,500-3,000-task graph replayed on both stream-window builds (32, 64) and
compared with ``oracle.replay`` of the same graph bit for bit: the placement log, every
round's snapshot and the final task states. The cases follow the paths the executor takes
by shape: the prefix count (dicts of one or two entries take dict_add's short form, longer
ones the general one; the descriptor's duration table up to 8 prefixes, the duration row past
it), ties in the objective's start time (the argmin reads nbytes and the worker index only
then), stimuli with many frontier tasks, restricted frontier tasks, thread counts and
saturations, queue refills on 2- and 4-thread workers, and worker state out of LDS.

Two things are not asserted because the replay cannot contain them: a queue refill of more
than one pop (a single graph's replay opens one queue slot per completion; the refill cases
assert that completions pop at all), and frontier stimuli past a per-stimulus bound of a
prefetcher side ring, which the engine does not have.

What a case must contain is first asserted on the CPU, on the oracle's log alone (seeds were
picked so that the oracle satisfies it; none is a fixture's or another test's seed).
"""
import numpy as np
import pytest

from oracle import oracle
from stimulus_census import max_worker_prefixes, stimulus_census

pytestmark = pytest.mark.gpu

PL_KEYS = ("pl_task", "pl_worker", "pl_comm", "pl_start", "pl_wsnbytes", "pl_route")
ROUND_KEYS = ("round_nplaced", "round_occ", "round_wnbytes", "round_nproc", "round_idle", "round_sat",
              "round_itc", "round_nqueued")
WINDOWS = (32, 64)
BASE_CFG = {"bandwidth": 100_000_000, "default_data_size": 1024, "unknown_duration": 0.5}


def cfg_of(sat):
    return dict(BASE_CFG, saturation=sat)


def one_prefix(g):
    """Every task under the single prefix / group "root" (P = 1)."""
    g = dict(g)
    n = g["n_tasks"]
    g.update(prefix_id=np.zeros(n, np.int32), group_id=np.zeros(n, np.int32), prefix_names=["root"],
             group_names=[g["group_names"][0]], group_prefix=np.zeros(1, np.int32),
             prefix_default_dur=np.full(1, -1.0))
    return g


def equal_nbytes(g, nb=4096):
    g = dict(g)
    g["nbytes"] = np.full(g["n_tasks"], nb, np.int64)
    return g


def build_case(name):
    """(graph, config) of a named case; deterministic."""
    from distributed_amd import graphs

    kind, _, arg = name.partition(":")
    if kind == "prefixes":  # P prefixes in all (root + inner ones), random durations
        p = int(arg)
        seed = {1: 9101, 2: 9102, 3: 9103, 8: 9108, 9: 9109}[p]
        g = graphs.random_dag(2000, 48, seed=seed, n_inner_prefixes=max(p - 1, 1), random_durations=True)
        return (one_prefix(g) if p == 1 else g), cfg_of(1.1)
    if kind == "ties":  # equal nbytes and durations: candidates in equal state tie on start
        w = int(arg)
        seed = {2: 9202, 3: 9203, 5: 9205}[w]
        return equal_nbytes(graphs.random_dag(2000, w, seed=seed, fanin=4 if w == 2 else 3)), cfg_of(1.1)
    if kind == "frontier":  # late completions of a layer release several tasks, kx 1..8
        g = graphs.layered_dag(12, 200, 64, seed=9301, fanins=(1, 2, 3, 4, 5, 6, 7, 8), random_durations=True)
        return g, cfg_of(1.1)
    if kind == "restricted":
        g = graphs.restrict(graphs.random_dag(2000, 48, seed=9401, n_inner_prefixes=2, random_durations=True), 0.3,
                            seed=9402, max_valid=4, empty_frac=0.0)
        return g, cfg_of(1.1)
    if kind == "threads":  # "one" | "mixed", saturation
        nth, _, sat = arg.partition("@")
        sat = "inf" if sat == "inf" else float(sat)
        g = graphs.random_dag(2000, 40, seed=9501 if nth == "one" else 9502, n_inner_prefixes=2, random_durations=True,
                              nthreads=1 if nth == "one" else "random")
        return g, cfg_of(sat)
    if kind == "refill":  # every worker 2 or 4 threads, a long queue: most completions pop from it
        nth = int(arg)
        g = graphs.random_dag(3000, 16, seed=9600 + nth, root_frac=0.4, random_durations=True, nthreads=nth)
        return g, cfg_of(1.1)
    if kind == "global_state":  # W = 2,048: the worker state does not fit LDS
        return graphs.random_dag(3000, 2048, seed=9701, n_inner_prefixes=2, random_durations=True), cfg_of(1.1)
    raise KeyError(name)


CASES = (["prefixes:%d" % p for p in (1, 2, 3, 8, 9)] + ["ties:%d" % w for w in (2, 3, 5)]
         + ["frontier", "restricted"]
         + ["threads:%s@%s" % (n, s) for n in ("one", "mixed") for s in ("1.0", "1.1", "inf")]
         + ["refill:2", "refill:4", "global_state"])

_REF = {}


def reference(name):
    """The case's graph, config and oracle replay: computed once, shared, never modified."""
    if name not in _REF:
        g, cfg = build_case(name)
        ref = oracle.replay(g, cfg)
        assert len(ref["pl_task"]) == g["n_tasks"]
        _REF[name] = (g, cfg, ref)
    return _REF[name]


def log_positions(g, ref):
    pos = np.full(g["n_tasks"], -1, np.int64)
    pt = np.asarray(ref["pl_task"])
    real = pt >= 0
    pos[pt[real]] = np.flatnonzero(real)
    return pos


def start_ties(g, ref):
    """Frontier decisions of the replay in which two candidates provably had equal start
    times, from the log alone. Task x is decided while its last dependency completes (the
    dependency latest in the log, at position c); its candidates are its dependencies'
    holders. By then log[:c + 1] has completed and log[:pos(x)] has been placed, so what
    each worker is processing is known. A worker's occupancy is the sum over its processing
    tasks' prefixes of count x duration plus needed bytes / bandwidth. In these graphs there
    are two prefixes (a two-term sum is the same in either order) and every nbytes is equal,
    so two workers with equal per-prefix counts and equally many needed dependencies
    (distinct dependencies of their processing tasks held elsewhere) have bit-equal
    occupancy; with equally many of x's dependencies not held, equal comm, so equal start."""
    ptr, idx = np.asarray(g["dep_ptr"]), np.asarray(g["dep_idx"])
    pfx = np.asarray(g["prefix_id"])
    assert len(g["prefix_names"]) == 2 and len(set(np.asarray(g["nthreads"]).tolist())) == 1
    pt, pw = np.asarray(ref["pl_task"]).tolist(), np.asarray(ref["pl_worker"]).tolist()
    pos = log_positions(g, ref)
    worker_of = np.full(g["n_tasks"], -1, np.int64)
    worker_of[pt] = pw
    proc = [set() for _ in g["nthreads"]]
    done = ties = 0
    for i, (x, wx) in enumerate(zip(pt, pw)):
        deps = idx[ptr[x]:ptr[x + 1]]
        if len(deps):
            c = int(pos[deps].max())
            while done <= c:  # completions up to and including x's last dependency
                proc[pw[done]].discard(pt[done])
                done += 1
            holders = worker_of[deps]
            keys = {}
            for w in set(holders.tolist()):
                cnt = np.bincount(pfx[list(proc[w])], minlength=2) if proc[w] else np.zeros(2, np.int64)
                needs = {int(d) for t in proc[w] for d in idx[ptr[t]:ptr[t + 1]] if worker_of[d] != w}
                k = (int(cnt[0]), int(cnt[1]), len(needs), int((holders != w).sum()))
                keys[k] = keys.get(k, 0) + 1
            ties += max(keys.values()) >= 2
        proc[wx].add(x)
    return ties


def check_shape(name, g, cfg, ref):
    """The CPU-side assertions: the oracle's own replay contains what the case is for."""
    kind, _, arg = name.partition(":")
    assert not (np.asarray(ref["pl_task"]) < 0).all()
    if kind == "prefixes":
        assert len(g["prefix_names"]) == int(arg)
        if int(arg) > 8:  # past the descriptor's 8 durations, yet within the per-worker dict
            assert max_worker_prefixes(g, ref) <= 8
    elif kind == "ties":
        assert len(set(np.asarray(g["nbytes"]).tolist())) == 1
        assert start_ties(g, ref) >= 20
    elif kind == "frontier":
        c = stimulus_census(g, ref, cfg["saturation"])
        local = c["reason"] == 0
        assert int((c["nf"][local] >= 4).sum()) >= 50
        assert set(range(1, 9)) <= set(c["kx_local"].tolist())
    elif kind == "restricted":
        ptr, idx = np.asarray(g["dep_ptr"]), np.asarray(g["dep_idx"])
        worker_of = np.full(g["n_tasks"], -1, np.int64)
        pt, pw = np.asarray(ref["pl_task"]), np.asarray(ref["pl_worker"])
        worker_of[pt[pt >= 0]] = pw[pt >= 0]
        n_restr = n_excl = 0
        for x in np.flatnonzero(np.asarray(g["restr_flags"]) & 1).tolist():
            deps = idx[ptr[x]:ptr[x + 1]]
            valid = set(np.asarray(g["restr_idx"])[g["restr_ptr"][x]:g["restr_ptr"][x + 1]].tolist())
            if len(deps) and valid and worker_of[x] >= 0:
                n_restr += 1
                n_excl += not (valid & set(worker_of[deps].tolist()))
        assert n_restr >= 100 and n_excl >= 1  # frontier tasks with resolved candidates; one excludes every holder
    elif kind == "refill":
        # queued tasks are popped by completions (route 1 past update_graph's first wave)
        first = int(ref["round_nplaced"][0])
        assert int((np.asarray(ref["pl_route"])[first:] == 1).sum()) >= 500
    elif kind == "global_state":
        assert len(g["nthreads"]) > 1024


@pytest.fixture(scope="module")
def engine_cls():
    from distributed_amd.engine import PlacementEngine

    return PlacementEngine


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("name", CASES)
def test_exe_path_matches_oracle(engine_cls, name, window):
    g, cfg, ref = reference(name)
    check_shape(name, g, cfg, ref)
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

"""The cases of tests/test_wide_values.py (CPU: what they contain) and
tests/test_gpu_wide_values.py (GPU: the engine against ``oracle.replay``): graphs with the
values of a live cluster (``graphs.widen``: results of several GB on both sides of 2^31 and
2^32, sizes the worker did not report, Unix timestamps) under a config that is none of the
engine's built-in defaults.

No seed here is a fixture's or another test's. They were picked so that every condition of
``census`` and ``sensitivity`` holds on the oracle's log; a case that misses one gets another
seed, never a weaker condition.
"""
import numpy as np

from oracle import oracle

PL_KEYS = ("pl_task", "pl_worker", "pl_comm", "pl_start", "pl_wsnbytes", "pl_route")
ROUND_KEYS = ("round_nplaced", "round_occ", "round_wnbytes", "round_nproc", "round_idle", "round_sat",
              "round_itc", "round_nqueued")

# as tests/golden/gen_golden.py WIDE_CONFIG (the wide_* fixtures' meta carries it)
WIDE = {"bandwidth": 12_345_678_901, "default_data_size": 5_000_000_000, "unknown_duration": 0.02}
DEFAULT = {"bandwidth": 100_000_000, "default_data_size": 1024, "unknown_duration": 0.5}
TIE_NBYTES = 2 ** 33


def wide_cfg(sat=1.1):
    return dict(WIDE, saturation=sat)


def build_case(name):
    """(graph, config) of a named case; deterministic."""
    from distributed_amd import graphs

    kind, _, arg = name.partition(":")
    if kind == "prefixes":  # P prefixes in all: dict_add's short form, the duration row, the round engine
        p = int(arg)
        seed = {2: 9802, 9: 9809, 40: 9840}[p]
        g = graphs.random_dag(2000, 48, seed=seed, n_inner_prefixes=p - 1, random_durations=True)
        return graphs.widen(g, {2: 17852, 9: 10859, 40: 9890}[p]), wide_cfg()
    if kind == "global_state":  # W = 2,048: the worker state does not fit LDS
        g = graphs.random_dag(3000, 2048, seed=9871, n_inner_prefixes=2, random_durations=True)
        return graphs.widen(g, 9872), wide_cfg()
    if kind == "refill":  # 2-thread workers, a long queue: most completions pop from it
        g = graphs.random_dag(3000, 16, seed=9862, root_frac=0.4, random_durations=True, nthreads=2)
        return graphs.widen(g, 9863), wide_cfg()
    if kind == "frontier":  # late completions of a layer release several tasks, fan-ins 1..8
        g = graphs.layered_dag(12, 200, 64, seed=9831, fanins=(1, 2, 3, 4, 5, 6, 7, 8), random_durations=True)
        return graphs.widen(g, 9832), wide_cfg()
    if kind == "restricted":
        g = graphs.restrict(graphs.random_dag(2000, 48, seed=9841, n_inner_prefixes=2, random_durations=True), 0.3,
                            seed=9842, max_valid=4, empty_frac=0.0)
        return graphs.widen(g, 9843), wide_cfg()
    if kind == "shuffle":
        # the barrier (task 2P) keeps a size. The narrower spread leaves the barrier's argmin,
        # the one decision of this replay that reads sizes, within reach of the unknown ones
        g = graphs.shuffle_graph(1500, 64, seed=9851)
        return graphs.widen(g, 26852, sigma=0.7, known=[2 * 1500]), wide_cfg()
    if kind == "service":  # the c2var shape, driven through the service entry points
        g = graphs.random_dag(2000, 48, seed=9881, n_inner_prefixes=3, random_durations=True, nthreads="random")
        return graphs.widen(g, 9882), wide_cfg()
    if kind == "ties":
        # equal results of 2^33 bytes and equal durations (one timestamp, one interval):
        # candidates in equal state tie on the start time, and the argmin falls through to
        # ws.nbytes, whose values are multiples of 2^33: they differ only above bit 32
        g = dict(graphs.random_dag(2000, 5, seed=9825, fanin=3))
        n = g["n_tasks"]
        g.update(nbytes=np.full(n, TIE_NBYTES, np.int64), start=np.full(n, 1.7e9), stop=np.full(n, 1.7e9 + 0.01))
        return g, wide_cfg()
    raise KeyError(name)


WIDENED = ["prefixes:2", "prefixes:9", "prefixes:40", "global_state", "refill", "frontier", "restricted", "shuffle",
           "service"]
CASES = WIDENED + ["ties"]

# What no seed can give. In the shuffle's replay the inputs are root-ish (placed by queue
# slots, which read no value), every transfer runs where its one input is, and every unpack
# where the barrier is: only the barrier's argmin reads sizes. Its candidates then run at most
# one transfer of a known duration each (0.01 s), while their comm terms differ by seconds at
# either bandwidth, and the barrier's own unknown duration is the same on every candidate. So
# the bandwidth and the unknown duration move the expected log (start times, occupancies) of
# this case, not a worker; tests/test_wide_values.py asserts that much for them.
LOG_ONLY = {"shuffle": ("bandwidth", "unknown_duration")}

_REF = {}


def reference(name):
    """The case's graph, config and oracle replay: computed once, shared, never modified."""
    if name not in _REF:
        g, cfg = build_case(name)
        _REF[name] = (g, cfg, oracle.replay(g, cfg))
    return _REF[name]


def recomputed_comm(g, cfg, ref):
    """Each placement's comm bytes from the log alone: the sizes (``default_data_size`` for an
    unknown one) of the task's dependencies that the chosen worker does not hold. In a plain
    replay a result's only holder is the worker that ran it. Returns (comm, unknown): the
    sums as Python ints, and how many unknown-size dependencies each one includes."""
    ptr, idx = np.asarray(g["dep_ptr"]), np.asarray(g["dep_idx"])
    nb = np.asarray(g["nbytes"])
    dds = int(cfg["default_data_size"])
    pt, pw = np.asarray(ref["pl_task"]), np.asarray(ref["pl_worker"])
    worker_of = np.full(g["n_tasks"], -1, np.int64)
    worker_of[pt] = pw
    comm, unknown = [], []
    for x, w in zip(pt.tolist(), pw.tolist()):
        deps = idx[ptr[x]:ptr[x + 1]]
        away = deps[worker_of[deps] != w]
        comm.append(sum(int(nb[d]) if nb[d] >= 0 else dds for d in away))
        unknown.append(int((nb[away] < 0).sum()))
    return comm, np.array(unknown)


def census(g, cfg, log):
    """What a wide case must contain, on a placement log (the oracle's or a fixture's)."""
    nb = np.asarray(g["nbytes"])
    assert (nb >= 2 ** 31).any() and (nb >= 2 ** 32).any()
    assert ((nb >= 0) & (nb < 2 ** 31)).any()  # ... and values whose high word is zero
    assert (np.asarray(log["pl_comm"]) >= 2 ** 32).any()
    assert (np.asarray(log["round_wnbytes"]) >= 2 ** 36).any()
    # the bound under which every sum of sizes is exact in a double (graphs.widen)
    assert sum(int(x) for x in nb[nb >= 0]) + int((nb < 0).sum()) * int(cfg["default_data_size"]) < 2 ** 53
    comm, unknown = recomputed_comm(g, cfg, log)
    assert comm == np.asarray(log["pl_comm"]).tolist()
    return unknown


def variants(g, cfg):
    """The four ways a wrong engine could see the case: the high word of every size dropped,
    and each config value at the engine's built-in default."""
    low = dict(g)
    nb = np.asarray(g["nbytes"])
    low["nbytes"] = np.where(nb >= 0, nb & 0xffffffff, nb)
    return {"nbytes & 0xffffffff": (low, cfg),
            "bandwidth": (g, dict(cfg, bandwidth=DEFAULT["bandwidth"])),
            "default_data_size": (g, dict(cfg, default_data_size=DEFAULT["default_data_size"])),
            "unknown_duration": (g, dict(cfg, unknown_duration=DEFAULT["unknown_duration"]))}


def sensitivity(g, cfg, log, key="pl_worker"):
    """Which variants' replays differ from ``log`` in ``key``: with ``pl_worker``, which place
    some task on another worker."""
    out = {}
    for what, (g2, cfg2) in variants(g, cfg).items():
        alt = oracle.replay(g2, cfg2, snapshots=False)
        a, b = np.asarray(alt[key]), np.asarray(log[key])
        out[what] = a.shape != b.shape or bool((a != b).any())
    return out

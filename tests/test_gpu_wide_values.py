"""The engine away from the one point every other test runs at (needs an MI355X).

The cases of tests/wide_cases.py -- results of several GB on both sides of 2^31 and 2^32, a
tenth of the sizes unknown, Unix timestamps, a bandwidth, default_data_size and unknown-task
duration that are none of the engine's built-in defaults -- replayed by the engine and
compared with ``oracle.replay`` of the same graph bit for bit: the placement log, every
round's snapshot and the final task states, on both stream windows where the stream engine
runs. tests/test_wide_values.py shows on the CPU what each case contains and that an engine
which dropped a high word or kept a default config value would place tasks elsewhere; the
oracle itself is pinned to the reference at these values by the ``wide_*`` fixtures.

* by shape: 2, 9 and 40 prefixes (dict_add's short form, the duration row past 8, the
  round-kernel engine), 2,048 workers (worker state outside LDS), queue refills, frontiers of
  fan-in 1..8, restrictions, the shuffle, and start-time ties that fall through to
  ``ws.nbytes`` values differing only above bit 32;
* service mode: one graph per message, per round, through the resident kernel and posted,
  the state audit clean after every round, the compute-task messages' sizes as reported;
* the config reaches the device: one engine replays under the wide config, the default one
  and the wide one again, also with the resident kernel running when the config changes;
* stealing at two other bandwidths against ``oracle.steal_balance``.
"""
import numpy as np
import pytest

import wide_cases as wc
from oracle import oracle
from test_gpu_audit import Audited
from test_gpu_exe_path import start_ties
from test_gpu_service import drive, drive_posted, fixture_messages
from test_oracle_steal import assert_same as assert_same_steal

pytestmark = pytest.mark.gpu

# the round-kernel engine (more than 32 prefixes) has no stream window
REPLAYS = [(name, w) for name in wc.CASES if name != "service"
           for w in ((32,) if name == "prefixes:40" else (32, 64))]


@pytest.fixture(scope="module")
def engine_cls():
    from distributed_amd.engine import PlacementEngine

    return PlacementEngine


def assert_log(out, ref, keys, what):
    for k in keys:
        a, b = np.asarray(out[k]), np.asarray(ref[k])
        assert a.shape == b.shape, (what, k, a.shape, b.shape)
        if a.dtype.kind == "f":  # bit-exact, not just ==
            a, b = a.view(np.int64), b.view(np.int64)
        bad = np.flatnonzero(a.reshape(-1) != b.reshape(-1))
        assert len(bad) == 0, (f"{what} {k}: {len(bad)} mismatches, first at {bad[0]}: "
                               f"{np.asarray(out[k]).reshape(-1)[bad[0]]!r} vs {np.asarray(ref[k]).reshape(-1)[bad[0]]!r}")
    assert np.array_equal(out["final_state"], ref["final_state"]), what


def collect(eng, R=0):
    out = eng.placements()
    if R:
        out.update(eng.snapshots(R))
    out["final_state"] = eng.task_states()
    return out


@pytest.mark.parametrize("name,window", REPLAYS)
def test_wide_replay_matches_oracle(engine_cls, name, window):
    g, cfg, ref = wc.reference(name)
    assert len(ref["pl_task"]) == g["n_tasks"]
    if name == "ties":
        assert start_ties(g, ref) >= 20
    R = ref["n_rounds"] + 2
    with engine_cls(0, window=window) as eng:
        eng.load(g, cfg, snapshots=R)
        eng.replay()
        out = collect(eng, R)
    assert_log(out, ref, wc.PL_KEYS + wc.ROUND_KEYS, name)


def expected_messages(g, ref, first):
    """The who_has / nbytes fields of the compute-task messages of placements [first, ...) once
    every task has completed: each dependency's reported size (-1: none reported, as
    ``_task_to_msg`` sends ``ts.nbytes``) and its one holder, the worker that ran it."""
    ptr, idx = np.asarray(g["dep_ptr"]), np.asarray(g["dep_idx"])
    pt, pw = np.asarray(ref["pl_task"]), np.asarray(ref["pl_worker"])
    worker_of = np.full(g["n_tasks"], -1, np.int64)
    worker_of[pt] = pw
    deps = np.concatenate([idx[ptr[x]:ptr[x + 1]] for x in pt[first:].tolist()])
    return deps, np.asarray(g["nbytes"])[deps], worker_of[deps]


@pytest.mark.parametrize("mode", ["per-message", "per-round", "resident-per-message", "resident-per-round", "posted",
                                  "resident-posted"])
def test_wide_service_matches_oracle(engine_cls, mode):
    g, cfg, ref = wc.reference("service")
    msgs, ptr = fixture_messages(g, ref)
    resident, posted = mode.startswith("resident"), mode.endswith("posted")
    R = ref["n_rounds"] + 2
    first = int(ref["round_nplaced"][0])
    with engine_cls(0) as eng:
        eng.load(g, cfg, snapshots=R, results=False)
        eng.set_resident(resident)
        if posted:
            eng.set_task_messages(resident)
        eng.update_graph()
        p = Audited(eng)
        p.check("snapshot")  # right after update_graph
        status = drive_posted(p, msgs, ptr) if posted else drive(p, msgs, ptr, mode.endswith("per-message"))
        out = collect(eng, R)
        tm = eng.task_messages(first, len(out["pl_task"]) - first)
    assert (status == 0).all(), np.bincount(status)
    assert p.n["snapshot"] >= ref["n_rounds"] - 1 and p.skipped == 0  # audited after every round
    assert_log(out, ref, wc.PL_KEYS + wc.ROUND_KEYS, mode)
    deps, sizes, holder = expected_messages(g, ref, first)
    assert np.array_equal(tm["dep_task"], deps)
    assert np.array_equal(tm["dep_nbytes"], sizes) and (sizes >= 2 ** 32).any() and (sizes < 0).any()
    assert np.array_equal(np.diff(tm["holder_ptr"]), np.ones(len(deps), np.int64))
    assert np.array_equal(tm["holder_idx"], holder)


_DEFAULT_REF = {}


def config_sequence():
    """The service case under its own config (A), the engine's built-in defaults (B) and A
    again, each with the oracle's log under that config. tests/test_wide_values.py shows that
    each of the three values alone moves a placement of this case."""
    g, cfg_a, ref_a = wc.reference("service")
    cfg_b = dict(wc.DEFAULT, saturation=cfg_a["saturation"])
    if "b" not in _DEFAULT_REF:
        _DEFAULT_REF["b"] = oracle.replay(g, cfg_b)
    ref_b = _DEFAULT_REF["b"]
    assert not np.array_equal(ref_a["pl_worker"], ref_b["pl_worker"])
    return g, [(cfg_a, ref_a), (cfg_b, ref_b), (cfg_a, ref_a)]


@pytest.mark.parametrize("window", (32, 64))
def test_config_reaches_the_device(engine_cls, window):
    """dgp_set_config on a loaded engine: reset, set_config, set_graph, replay."""
    g, seq = config_sequence()
    R = max(ref["n_rounds"] for _, ref in seq) + 2
    with engine_cls(0, window=window) as eng:
        eng.load(g, seq[0][0], snapshots=R)
        for k, (cfg, ref) in enumerate(seq):
            if k:
                eng.reset()
                eng.set_config(cfg)
                eng.set_graph(g)
            eng.replay()
            assert_log(collect(eng, R), ref, wc.PL_KEYS + wc.ROUND_KEYS, f"config {k}")


def test_config_reaches_a_relaunched_resident_kernel(engine_cls):
    """The same with the resident kernel running when the config changes: dgp_set_config ends
    it, and the kernel launched by the next batch must see the new values."""
    g, seq = config_sequence()
    with engine_cls(0) as eng:
        eng.load(g, seq[0][0], results=False)
        eng.set_resident(True)
        for k, (cfg, ref) in enumerate(seq):
            eng.update_graph()
            msgs, ptr = fixture_messages(g, ref)
            for a, b in zip(ptr[:-1], ptr[1:]):  # one batch per round, the kernel stays launched
                if b > a:
                    t, w, r, nb, s0, s1 = (np.array(c) for c in zip(*msgs[a:b]))
                    st, _ = eng.tasks_finished(t, w, r, nb, s0, s1)
                    assert (st == 0).all()
            eng.set_config(seq[(k + 1) % len(seq)][0])  # ends the resident kernel
            assert_log(collect(eng), ref, wc.PL_KEYS, f"resident config {k}")
            eng.reset()
            eng.set_graph(g, results=False)


STEAL_BW = (12_500_000_000, 1_000_000)


@pytest.mark.parametrize("bw", STEAL_BW)
def test_steal_balance_at_another_bandwidth(engine_cls, bw):
    from distributed_amd import graphs

    p = graphs.steal_problem(256, 20000, seed=9891, bandwidth=bw)
    ref = oracle.steal_balance(p)
    assert len(ref["st_task"]) > 0
    # the levels read the bandwidth: the default one gives others
    assert not np.array_equal(oracle.steal_balance(dict(p, bandwidth=wc.DEFAULT["bandwidth"]))["level"], ref["level"])
    with engine_cls(0) as eng:
        out = eng.steal_balance(p)
    assert_same_steal(out, ref)

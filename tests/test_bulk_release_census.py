"""What the ``svcbulk_*`` streams (tests/golden/gen_bulk_release.py -> tests/golden/bulk/) hold,
from the fixture arrays alone (no GPU): multi-key client-releases-keys calls whose plans are long, start from
every task state, remove queued tasks at the head, inside, at the tail and all at once, meet
two-word who_has rows, paused workers, long-running tasks, replicated results and no-worker
tasks, forget tasks, and release dependencies together with their cancelled dependents."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

BULK = os.path.join(GOLDEN, "bulk")

RELEASED, WAITING, PROCESSING, QUEUED, NO_WORKER, MEMORY = range(6)
EV_PAUSE, EV_LONG_RUNNING, EV_RELEASE_KEYS = 3, 5, 10

# per stream: the entry states its plans must start from (its own conditions)
STREAMS = {
    "svcbulk_half_c2var_sat1.1": {WAITING, PROCESSING, MEMORY},
    "svcbulk_half_c2mini_satinf": {RELEASED, WAITING, MEMORY},
    "svcbulk_all_c2var_sat1.1": {WAITING, PROCESSING, QUEUED, MEMORY},
    "svcbulk_all_c2mini_satinf": {RELEASED, WAITING, PROCESSING, MEMORY},
    "svcbulk_group_c2var_sat1.1": {RELEASED, WAITING, PROCESSING, MEMORY},
    "svcbulk_queue_sat1.1": {WAITING, PROCESSING, QUEUED, MEMORY},
    "svcbulk_tail_sat1.1": {WAITING, PROCESSING, QUEUED, MEMORY},
    "svcbulk_w70_sat1.1": {WAITING, MEMORY},
    "svcbulk_restr_sat1.1": {WAITING, PROCESSING, NO_WORKER, MEMORY},
    "svcbulk_skew_satinf": {PROCESSING, MEMORY},
    "svcbulk_skew_wide_satinf": {RELEASED, PROCESSING, MEMORY},
    "svcbulk_skew_thin_satinf": {PROCESSING, MEMORY},
}
# the streams whose first long call lists a few workers' exits before most of the others'
# (gen_bulk_release.py's skew policy); the nine before them carry no bk_sens_* split
SKEW = ("svcbulk_skew_satinf", "svcbulk_skew_wide_satinf", "svcbulk_skew_thin_satinf")
ALL_SINKS = ("svcbulk_skew_satinf", "svcbulk_skew_thin_satinf")  # no task has a dependency


def load(name):
    return np.load(os.path.join(BULK, name + ".npz"), allow_pickle=False)


def queue_removals(z):
    """Per call that removes queued tasks: (queue length, places removed)."""
    qp = z["bk_qpos_ptr"]
    return [(int(z["bk_qlen"][i]), z["bk_qpos"][qp[i]:qp[i + 1]]) for i in range(len(z["bk_n"])) if qp[i + 1] > qp[i]]


def test_every_stream_is_there():
    have = sorted(f[:-4] for f in os.listdir(BULK) if f.startswith("svcbulk_") and f.endswith(".npz"))
    assert have == sorted(STREAMS)


@pytest.mark.parametrize("name", sorted(STREAMS))
def test_stream_reaches_its_conditions(name):
    z = load(name)
    n, rp = z["bk_n"], z["rk_evptr"]
    assert len(n) >= 1 and n.max() > 64, n  # a multi-key call with a long plan
    assert np.array_equal(z["bk_event"], np.flatnonzero(z["ev_kind"] == EV_RELEASE_KEYS))
    assert np.array_equal(n, (rp[1:] - rp[:-1])[z["bk_event"]])  # one plan per call, bk_n its length
    assert len(z["rk_state"]) == len(z["rk_task"]) == len(z["rk_forget"])
    states = set(np.unique(z["rk_state"]).tolist())
    assert STREAMS[name] <= states, (STREAMS[name] - states, states)
    assert z["rk_forget"].any()  # forgotten entries
    for t in (z["rk_task"][rp[e]:rp[e + 1]] for e in z["bk_event"]):
        assert len(np.unique(t)) == len(t)  # each task listed once
    dp, di = z["dep_ptr"], z["dep_idx"]
    if name in ALL_SINKS:
        assert len(di) == 0
        return
    # a dependency released in the same plan as its cancelled dependent
    both = 0
    for e in z["bk_event"]:
        t, st = z["rk_task"][rp[e]:rp[e + 1]], z["rk_state"][rp[e]:rp[e + 1]]
        listed = np.zeros(len(dp) - 1, bool)
        listed[t] = True
        both += sum(bool(listed[di[dp[x]:dp[x + 1]]].any()) for x in t[np.isin(st, (WAITING, PROCESSING, QUEUED, NO_WORKER))])
    assert both > 0


def test_queue_removal_places():
    head = tail = inside = everything = 0
    for name in STREAMS:
        for qlen, pos in queue_removals(load(name)):
            assert len(pos) <= qlen and (np.diff(pos) > 0).all() and pos[0] >= 0 and pos[-1] < qlen
            if len(pos) == qlen:
                everything += 1
                continue
            head += pos[0] == 0
            tail += pos[-1] == qlen - 1
            kept = np.setdiff1d(np.arange(qlen), pos)
            inside += bool(((pos > kept.min()) & (pos < kept.max())).any())
    assert head >= 1 and tail >= 1 and inside >= 1 and everything >= 1, (head, tail, inside, everything)
    assert len(queue_removals(load("svcbulk_all_c2var_sat1.1"))) == 1
    qlen, pos = queue_removals(load("svcbulk_all_c2var_sat1.1"))[0]
    assert len(pos) == qlen >= 64


def test_two_holder_words_paused_workers_long_running_and_replicas():
    assert len(load("svcbulk_w70_sat1.1")["nthreads"]) == 70  # who_has rows of two words
    zs = [load(n) for n in STREAMS]
    # the svcev machinery runs in every stream; the long ones pause workers and secede tasks
    assert sum({EV_PAUSE, EV_LONG_RUNNING} <= set(np.unique(z["ev_kind"]).tolist()) for z in zs) >= 5
    assert sum(int((z["bk_npaused"][z["bk_n"] > 64] > 0).sum()) for z in zs) >= 1  # a long plan with a worker paused
    assert sum(int(z["bk_nlr"].sum()) for z in zs) >= 1  # a long-running task cancelled
    assert sum(int(z["bk_nmulti"].sum()) for z in zs) >= 1  # a result with several replicas released
    assert sum(int((z["rk_state"] == NO_WORKER).sum()) for z in zs) >= 1
    assert set(np.unique(np.concatenate([z["rk_state"] for z in zs])).tolist()) == set(range(6))


def test_order_sensitivity_of_check_idle_saturated():
    """bk_sens counts, per call, the workers that lost a processing task and whose idle /
    saturated flags would differ had check_idle_saturated read the end-of-call total
    occupancy instead of the total at the worker's last exit. The generator's bounded search
    (200 seeds of the svcbulk_half_c2mini_satinf stream, recorded in bk_search) found no such
    worker in the nine earlier streams: their plans cancel few processing tasks (the wanted
    keys are sinks, mostly still waiting), and a worker that loses one is idle by its thread
    count whatever the total is. That stays a fact about those fixtures.

    The skew streams' long calls have such workers, split by the flag that would differ
    (bk_sens_idle / bk_sens_sat) and by the term of the total that moves it when it alone is
    read at the end of the call (bk_sens_cnt: the prefix counts, bk_sens_net: the network
    bytes). In the all-sink streams nothing is fetched, so only the counts can; in the wide
    stream the cancelled tasks' fetches of several GB each are most of the total."""
    zs = {n: load(n) for n in STREAMS}
    assert zs["svcbulk_half_c2mini_satinf"]["bk_search"].tolist() == [200, 0]
    assert sum(int(z["bk_sens"].sum()) for n, z in zs.items() if n not in SKEW) == 0

    def on_long_calls(z, k):
        return int(z[k][z["bk_n"] > 64].sum())

    for k in ("bk_sens_idle", "bk_sens_sat", "bk_sens_cnt"):
        assert sum(on_long_calls(zs[n], k) for n in SKEW) >= 1, k
    assert on_long_calls(zs["svcbulk_skew_wide_satinf"], "bk_sens_net") >= 1
    for n in SKEW:
        z = zs[n]
        assert on_long_calls(z, "bk_sens") >= 1, n
        assert (z["bk_sens"] <= z["bk_sens_idle"] + z["bk_sens_sat"]).all()
        assert z["bk_idle"].shape == z["bk_sat"].shape == (len(z["bk_n"]), len(z["nthreads"]))
        assert not (z["bk_idle"] & z["bk_sat"]).any()
    for n in ALL_SINKS:  # nothing is fetched: the counts alone move the total
        assert not zs[n]["bk_freed"].any() and not zs[n]["bk_sens_net"].any()
        assert np.array_equal(zs[n]["bk_sens_cnt"], zs[n]["bk_sens"])
    # the thin stream's second call: idle by half the average at the exit, not by the end's
    z = zs["svcbulk_skew_thin_satinf"]
    assert z["bk_n"][:2].min() > 64 and z["bk_sens_idle"][1] >= 1


def test_wide_skew_stream_byte_sums_pass_2_32():
    """The bulk path's 64-bit sums on a long plan: one call of the wide stream frees more
    than 2^32 network bytes (the reference's _network_occ_global before and after it), its
    plan long and with many exits, and releases results of more than 2^32 bytes each."""
    z = load("svcbulk_skew_wide_satinf")
    rp = z["rk_evptr"]
    big = [i for i in range(len(z["bk_n"])) if z["bk_n"][i] > 64 and z["bk_freed"][i] > 2 ** 32]
    assert big, z["bk_freed"]
    found = 0
    for i in big:
        e = z["bk_event"][i]
        t, st = z["rk_task"][rp[e]:rp[e + 1]], z["rk_state"][rp[e]:rp[e + 1]]
        assert (st == PROCESSING).sum() > 64
        found += int((z["nbytes"][t[st == MEMORY]] > 2 ** 32).sum())
    assert found >= 1
    # (double)freed / bandwidth at a bandwidth of the stream's own
    assert json.loads(str(z["meta"]))["config"]["bandwidth"] not in (None, 100_000_000)

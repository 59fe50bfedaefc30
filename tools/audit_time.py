"""Device time of one dgp_audit_state call on the C2 graph (1M tasks x 1,024 workers), half-way
through: python tools/audit_time.py [--out profiles/audit_time.json] [--tasks N --workers W]

The audit is refused between replay rounds, so the graph is advanced in service mode: each
batch completes the placements of the one before (the replay protocol's rounds) until half the
tasks have finished. Then 2 warm-up calls and 10 timed ones, with HIP events on the engine's
stream around the audit's five launches (dgp_set_timing, kernel-time id "audit") and a host
clock around the whole call (it ends in a stream synchronise). Also written: the bytes the
rules must read at least at that point, from the shapes and the task states -- every per-task
array once, the who_has rows, the dependency rows of the waiting / queued / processing /
no-worker tasks, the dependents rows of the tasks in memory, the workers' tables.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_amd import graphs  # noqa: E402
from distributed_amd.engine import PlacementEngine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                              "audit_time.json"))
ap.add_argument("--tasks", type=int, default=1_000_000)
ap.add_argument("--workers", type=int, default=1024)
a = ap.parse_args()

g = graphs.random_dag(a.tasks, a.workers, seed=0)
N, W, P, G = int(g["n_tasks"]), len(g["nthreads"]), len(g["prefix_default_dur"]), len(g["group_prefix"])
with PlacementEngine(0) as e:
    e.load(g, {"saturation": 1.1}, results=False)
    e.update_graph()
    pos = done = 0
    while done < N // 2:
        n = e.num_placements() - pos
        assert n > 0, "the graph stalled"
        pl = e.placements(pos, n, columns=("pl_task", "pl_worker"))
        t = pl["pl_task"]
        st, _ = e.tasks_finished(t, pl["pl_worker"], np.arange(pos, pos + n), g["nbytes"][t], g["start"][t], g["stop"][t])
        assert (st == 0).all()
        pos += n
        done += n
    state = e.task_states()
    e.set_timing(True)
    for _ in range(2):
        found, skipped = e.audit_state()
        assert found == [], found[:4]
    ms0, n0 = e.kernel_times()["audit"]
    wall = []
    for _ in range(10):
        t0 = time.perf_counter()
        e.audit_state()
        wall.append(time.perf_counter() - t0)
    ms1, n1 = e.kernel_times()["audit"]
assert n1 - n0 == 10
WB = (W + 63) // 64
deg_in = np.diff(g["dep_ptr"])
deg_out = np.bincount(g["dep_idx"], minlength=N)
active = np.isin(state, (1, 2, 3, 4))
memory = state == 5
per_task = 1 + 1 + 1 + 4 + 4 + 4 + 4 + 4 + 4 + 8 + 8 * WB  # state, tdyn, tflags, proc_on, prefix, group, holder_of,
#                                                             remaining, waiters, cur_nbytes, the who_has row
edges = int(deg_in[active].sum()) + int(deg_out[memory].sum())
per_worker = 4 * 4 + 2 * 4 * 8 + 3 * 8 + 1 + 4 * (12 + 52)  # nproc, cap, plen, nthreads; the dict; netocc, nbytes, slots;
#                                                              flags; the needs_what line and overflow entries
res = dict(graph=g["name"], N=N, W=W, P=P, G=G, tasks_finished=int(done),
           states={k: int((state == v).sum()) for k, v in (("released", 0), ("waiting", 1), ("processing", 2),
                                                           ("queued", 3), ("memory", 5))},
           device_ms_per_call=(ms1 - ms0) / 10, host_ms_per_call=1e3 * float(np.median(wall)),
           host_ms_min_max=[1e3 * min(wall), 1e3 * max(wall)], calls=10, warmups=2, scan_mode_workers=int(skipped),
           min_bytes=int(N * per_task + 2 * 8 * (N + 1) + 4 * edges + W * per_worker),
           edges_walked=edges)
res["min_GBps_at_device_time"] = res["min_bytes"] / (res["device_ms_per_call"] * 1e-3) / 1e9
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps(res))

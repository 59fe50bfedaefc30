"""Host time of loss.release_plan for one client-releases-keys call of ~100k keys, on the
reference's own scheduler state (build container: python3.9 + tests/golden/_refshim):

    PYTHONHASHSEED=0 /opt/conda/bin/python3.9 tools/release_plan_time.py [--tasks N] [--out FILE]

A C2-shaped graph (random_dag, 256 workers, saturation 1.1) with every task wanted by the
client, right after update_graph; the call releases every key. Reported: the plan's length
and the time per planned task, best of 3 (the plan is a dry run on a shadow of the state, so
it repeats), next to the reference's own client_releases_keys for the same call, which runs
once, last, since it changes the state.
-> profiles/bulk_release/release_plan_host.txt
"""
import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests", "golden"))

import gen_service as S  # noqa: E402  (re-executes under PYTHONHASHSEED=0, installs the shim)

import numpy as np  # noqa: E402

G = S.G


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tasks", type=int, default=100_000)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bulk_release", "release_plan_host.txt"))
    a = ap.parse_args()
    from distributed.scheduler import Scheduler

    g = G.graphs.random_dag(a.tasks, 256, seed=9)
    g["wanted"] = np.ones(g["n_tasks"], np.uint8)
    cfg = G.config_dict(1.1)
    loss = S._load_repo_module("loss")
    with G.reference_config(cfg):
        s, tss, widx, rec, tidx = G.build_state(g, cfg)
        cls = type(s)
        cls.client_releases_keys = Scheduler.client_releases_keys
        cls.send_all = lambda self, client_msgs, worker_msgs: None
        s._transitions({ts.key: "waiting" for ts in sorted(tss, key=lambda t: t.priority, reverse=True)}, {}, {},
                       "update-graph")
        states = np.bincount([G.STATE_CODES[ts.state] for ts in tss], minlength=6).tolist()
        keys = [ts.key for ts in tss]
        best, plan = None, None
        for _ in range(3):
            t0 = time.perf_counter()
            plan = loss.release_plan(s, "client-0", keys)
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        assert plan is not None and len(plan) == len(tss)
        t0 = time.perf_counter()
        s.client_releases_keys(keys=keys, client="client-0", stimulus_id="release-all")
        ref = time.perf_counter() - t0
    lines = [f"loss.release_plan, one call of {len(keys)} keys (random_dag {g['n_tasks']} x 256, saturation 1.1, after "
             f"update_graph; states released/waiting/processing/queued/no-worker/memory {states})",
             f"plan of {len(plan)} tasks: {best:.3f} s best of 3, {1e6 * best / len(plan):.2f} us per planned task",
             f"the reference's own client_releases_keys for the same call: {ref:.3f} s, "
             f"{1e6 * ref / len(plan):.2f} us per task (one run)"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()

"""Time of dgp_release_tasks on its two device paths: python tools/release_time.py [--out DIR]

A cancelled graph: every key released right after update_graph, the plan in reverse
topological order. Two shapes on 64 workers, graphs of 16 to 16k tasks: "free" (saturation
inf: nothing queued, a tenth of the tasks processing) and "queued" (saturation 1.1, half the
tasks roots: almost all of them queued). Each (shape, size, mode) is a step: a child process
under its own time limit that, five times, loads the graph, runs update_graph and times the
one release call. The call is synchronous (it ends in a stream synchronise and the
bulk path reads its pre-pass back half-way), so the time is the host clock around it: what
the scheduler's thread is blocked for. Best of five. The serial path (mode 1) runs only
where n * len(queued) <= 1e8. The first step that fails ends the run.

-> DIR/crossover.txt   the table, and the smallest n from which the bulk path is not slower
                       on both shapes (DGP_RELEASE_BULK_MIN is that, as a power of two)
-> DIR/c2_cancel.txt   the bulk path alone on C2 (1M tasks x 1,024 workers) and C3 (the P2P
                       shuffle, 66,666 partitions x 512 workers), with the serial path's cost
                       extrapolated from the largest measured queued size (n * len(queued))
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SIZES = (16, 64, 256, 1024, 4096, 16384)
SERIAL_LIMIT = 1e8
CFG = {"bandwidth": 100_000_000, "default_data_size": 1024, "unknown_duration": 0.5}


def graph_of(shape, n):
    from distributed_amd import graphs

    if shape == "free":
        return graphs.random_dag(n, 64, seed=1), float("inf")
    if shape == "queued":
        return graphs.random_dag(n, 64, seed=1, root_frac=0.5), 1.1
    if shape == "c2":
        return graphs.random_dag(1_000_000, 1024, seed=0), 1.1
    if shape == "c3":
        return graphs.shuffle_graph(66_666, 512), 1.1
    raise ValueError(shape)


def step(shape, n, mode, reps):
    from distributed_amd.engine import PlacementEngine

    g, sat = graph_of(shape, n)
    N = int(g["n_tasks"])
    order = np.argsort(-np.asarray(g["prio"]), kind="stable").astype(np.int32)  # dependents first
    forget = np.zeros(N, np.uint8)
    ts, qlen = [], 0
    with PlacementEngine(0) as e:
        e.set_release_mode(mode)
        for r in range(reps):
            if r == 0:
                e.load(g, dict(CFG, saturation=sat), results=False)
            else:  # a release clears the wanted flags: the graph anew (which resets the engine)
                e.set_graph(g, results=False)
            e.update_graph()
            st = e.task_states()
            qlen = int((st == 3).sum())
            if mode == 1 and N * qlen > SERIAL_LIMIT:
                return dict(shape=shape, n=N, mode=mode, qlen=qlen, skipped="n * len(queued) > 1e8")
            t0 = time.perf_counter()
            assert e.release_tasks(order, forget) is not None, e.refusal
            ts.append(time.perf_counter() - t0)
            assert e.last_release_path == mode
            assert (e.task_states() == 0).all()
    return dict(shape=shape, n=N, mode=mode, qlen=qlen, nproc=int((st == 2).sum()), best_ms=1e3 * min(ts),
                all_ms=[round(1e3 * t, 4) for t in ts])


def child(shape, n, mode, limit, reps=5):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", shape, str(n), str(mode), str(reps)],
                       capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        raise SystemExit(f"step {shape} n={n} mode={mode} failed ({r.returncode}): {r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bulk_release"))
    ap.add_argument("--step", nargs=4, metavar=("SHAPE", "N", "MODE", "REPS"))
    ap.add_argument("--no-large", action="store_true", help="skip the C2 / C3 steps")
    a = ap.parse_args()
    if a.step:
        print(json.dumps(step(a.step[0], int(a.step[1]), int(a.step[2]), int(a.step[3]))))
        return
    os.makedirs(a.out, exist_ok=True)
    rows = {}
    lines = ["dgp_release_tasks, every key of the graph released after update_graph; host clock around the call, "
             "best of 5, ms", f"{'shape':8}{'n':>8}{'queued':>8}{'processing':>12}{'serial':>12}{'bulk':>12}"]
    for shape in ("free", "queued"):
        for n in SIZES:
            for mode in (1, 2):
                rows[shape, n, mode] = child(shape, n, mode, 120)
            s, b = rows[shape, n, 1], rows[shape, n, 2]
            lines.append(f"{shape:8}{n:>8}{b['qlen']:>8}{b['nproc']:>12}"
                         f"{('%.3f' % s['best_ms']) if 'best_ms' in s else 'not run':>12}{b['best_ms']:>12.3f}")
            print(lines[-1], flush=True)

    def bulk_wins(n):
        return all("best_ms" not in rows[sh, n, 1] or rows[sh, n, 2]["best_ms"] <= rows[sh, n, 1]["best_ms"]
                   for sh in ("free", "queued"))

    first = next((n for i, n in enumerate(SIZES) if all(bulk_wins(m) for m in SIZES[i:])), None)
    lines.append(f"smallest n from which the bulk path is not slower on both shapes: {first}")
    if first is not None:
        lines.append(f"DGP_RELEASE_BULK_MIN (that, as a power of two): {1 << (first - 1).bit_length()}")
    with open(os.path.join(a.out, "crossover.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-2:]), flush=True)
    if a.no_large:
        return
    # the serial kernel's cost per (task, queue entry) step, from the largest queued size it ran at
    ref = max((r for (sh, n, m), r in rows.items() if sh == "queued" and m == 1 and "best_ms" in r), key=lambda r: r["n"])
    per_step = ref["best_ms"] / (ref["qlen"] * ref["qlen"] / 2)  # each queued task searches the queue left: ~qlen / 2
    out = ["dgp_release_tasks on the bulk path, every key released after update_graph; host clock, best of 3, ms"]
    for shape in ("c2", "c3"):
        r = child(shape, 0, 2, 600, reps=3)
        est = per_step * r["qlen"] * r["qlen"] / 2
        out.append(f"{shape}: n {r['n']}, queued {r['qlen']}, processing {r['nproc']}: bulk {r['best_ms']:.3f} ms "
                   f"(runs {r['all_ms']})")
        out.append(f"{shape}: serial path, EXTRAPOLATED (not run): {per_step * 1e6:.3f} ns per queue step measured at "
                   f"n {ref['n']}, queued {ref['qlen']} ({ref['best_ms']:.3f} ms) x queued^2 / 2 = {est / 1e3:.1f} s")
        print("\n".join(out[-2:]), flush=True)
    with open(os.path.join(a.out, "c2_cancel.txt"), "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()

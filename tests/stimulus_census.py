"""What each completion of a replay looks like to the engines, counted on the CPU from a graph
and a placement log alone (test bookkeeping; nothing here runs the code under test).

``stimulus_census`` walks the tests of the stream engine's prefetcher in the order
``build_desc`` applies them (distributed_amd/csrc/dgp_stream.h, the places that set
``F_GLOBAL``), with the limits below, which restate that header's constants. The census shows
that a graph has stimuli on both sides of each limit; it does not predict the device's result.
"""
import math

import numpy as np

E_HDR = 7     # header entries of a descriptor
NE = 64       # descriptor entries of a local stimulus
KT_MAX = 24   # dependencies of the completing task in local mode
KX_MAX = 8    # dependencies of a ready task in local mode
TMAX = 32     # distinct workers a local stimulus touches
PLC = 64      # staging rows of a local stimulus

REASONS = ("local", "kt", "release_ne", "kx", "ne", "tmax", "plc")


def stimulus_census(g, out, saturation):
    """The replay completes tasks in log order (``out``: ``pl_task`` / ``pl_worker``, the
    reference's or the oracle's). Completion r of task t on worker w is walked as the
    prefetcher walks it:

    1. ``kt`` = dependencies of t; ``kt > KT_MAX``: global ("kt"), nothing more is counted;
    2. n = E_HDR + kt entries; one more entry, and the touch of its holder, per dependency of
       t that this completion releases (its last dependent, not wanted); no room (n >= NE):
       global ("release_ne");
    3. the tasks made ready, in ascending priority: ``kx > KX_MAX`` ("kx") or
       ``n + 1 + kx > NE`` ("ne") make the stimulus global and end the walk; else 1 + kx
       entries and the touch of every dependency's holder;
    4. more than TMAX workers touched ("tmax"), or nf + max(ceil(nthreads[w] * saturation), 1)
       + 1 staging rows > PLC (nf + 1 at saturation inf; "plc"): global.

    Per completion: ``kt``, ``nf`` (tasks made ready, all of them), ``staging``, ``reason``
    (index into REASONS, 0 = local), ``n`` and ``nt`` (entries and workers counted when the
    walk ended), ``trip_n`` (the n + 1 + kx that tripped "ne", else 0), ``entries_all`` /
    ``nt_all`` (E_HDR + kt + sum(1 + kx) and w plus the holders over every ready task, whatever
    the walk did: marginal counts, which a stimulus that is global for another reason reaches
    without the device ever counting that far). ``kx``: every ready
    task's dependency count, all completions concatenated; ``kx_local``: those of stimuli the
    walk left local. Root-ish and restricted ready tasks (global, or with candidate entries of
    their own) are not modelled: use it on graphs whose non-root tasks are neither."""
    n_tasks = int(g["n_tasks"])
    ptr, idx = np.asarray(g["dep_ptr"]), np.asarray(g["dep_idx"])
    nth, wanted, prio = np.asarray(g["nthreads"]), np.asarray(g["wanted"]), np.asarray(g["prio"])
    sat = math.inf if saturation == "inf" else float(saturation)
    ndep = np.diff(ptr).astype(np.int64)
    src = np.repeat(np.arange(n_tasks), ndep)
    order = np.lexsort((prio[src], idx))  # dependents of each task, ascending priority
    dpt_idx = src[order]
    dpt_ptr = np.zeros(n_tasks + 1, np.int64)
    if len(idx):
        dpt_ptr[1:] = np.cumsum(np.bincount(idx, minlength=n_tasks))
    left = ndep.copy()
    waiters = np.diff(dpt_ptr).copy()
    holder = np.full(n_tasks, -1, np.int64)
    cols = {k: [] for k in ("kt", "nf", "staging", "reason", "n", "nt", "trip_n", "entries_all", "nt_all")}
    kx_all, kx_local = [], []
    for t, w in zip(np.asarray(out["pl_task"]).tolist(), np.asarray(out["pl_worker"]).tolist()):
        holder[t] = w
        deps = idx[ptr[t]:ptr[t + 1]]
        released = []
        for d in deps.tolist():
            waiters[d] -= 1
            if waiters[d] == 0 and not wanted[d]:
                released.append(d)
        ready = []
        for x in dpt_idx[dpt_ptr[t]:dpt_ptr[t + 1]].tolist():
            left[x] -= 1
            if left[x] == 0:
                ready.append(x)
        kxs = [int(ndep[x]) for x in ready]
        kx_all += kxs
        kt, nf = int(ndep[t]), len(ready)
        staging = nf + 1 + (0 if math.isinf(sat) else max(math.ceil(int(nth[w]) * sat), 1))
        touched = {w}
        n, reason, trip = E_HDR, 0, 0
        if kt > KT_MAX:
            reason = 1
        else:
            n += kt
            for d in released:
                if n >= NE:
                    reason = 2
                    break
                touched.add(int(holder[d]))
                n += 1
        if not reason:
            for x, kx in zip(ready, kxs):
                if kx > KX_MAX:
                    reason = 3
                    break
                if n + 1 + kx > NE:
                    reason, trip = 4, n + 1 + kx
                    break
                n += 1 + kx
                touched.update(holder[idx[ptr[x]:ptr[x + 1]]].tolist())
        if not reason and len(touched) > TMAX:
            reason = 5
        if not reason and staging > PLC:
            reason = 6
        if not reason:
            kx_local += kxs
        every = {w}
        for x in ready:
            every.update(holder[idx[ptr[x]:ptr[x + 1]]].tolist())
        for k, v in (("kt", kt), ("nf", nf), ("staging", staging), ("reason", reason), ("n", n),
                     ("nt", len(touched)), ("trip_n", trip), ("entries_all", E_HDR + kt + sum(1 + k for k in kxs)),
                     ("nt_all", len(every))):
            cols[k].append(v)
    res = {k: np.array(v, np.int64) for k, v in cols.items()}
    res["kx"] = np.array(kx_all, np.int64)
    res["kx_local"] = np.array(kx_local, np.int64)
    return res


def max_worker_prefixes(g, out):
    """The most distinct task prefixes any worker is given over two consecutive rounds of a
    replay (``out``: ``pl_task`` / ``pl_worker`` / ``round_nplaced``). What a worker
    processes at any moment was placed in the round before or in the running one, so this
    bounds the entries of its ``task_prefix_count`` from above; the engines keep 8 per worker
    (``PMAX``), a documented limit."""
    pt, pw = np.asarray(out["pl_task"]), np.asarray(out["pl_worker"])
    pfx = np.asarray(g["prefix_id"])[pt]
    ends = np.cumsum(np.asarray(out["round_nplaced"], np.int64))
    ends = ends[: int(np.searchsorted(ends, len(pt))) + 1]
    starts = np.concatenate([[0], ends[:-1]])
    P = int(pfx.max()) + 1 if len(pfx) else 1
    best = 0
    for k in range(len(ends)):
        a, b = int(starts[max(k - 1, 0)]), int(ends[k])
        pairs = np.unique(pw[a:b].astype(np.int64) * P + pfx[a:b])
        if len(pairs):
            best = max(best, int(np.bincount(pairs // P).max()))
    return best


def scan_mode_refills(g, out, saturation, cap):
    """(refills, local stimuli on a scanning worker): the stimuli that found the engines'
    scan-mode error. A worker whose needs_what has passed ``cap`` entries (63 on the stream
    engine, 31 on the round-kernel engine) decides "does anything here still need d" by
    scanning processing_on, until it has nothing processing. A refill is a stimulus the
    prefetcher leaves local (``stimulus_census``) whose completion of t on such a worker w
    places a ready task on w itself (``out``'s placement) that shares with t a dependency
    held elsewhere and needed by nothing else on w: counted right only if t no longer
    counts as processing on w. needs_what is kept as the reference keeps it (:800-823)."""
    c = stimulus_census(g, out, saturation)
    n = int(g["n_tasks"])
    ptr, idx, prio = np.asarray(g["dep_ptr"]), np.asarray(g["dep_idx"]), np.asarray(g["prio"])
    pt, pw = np.asarray(out["pl_task"]).tolist(), np.asarray(out["pl_worker"]).tolist()
    W = len(g["nthreads"])
    placed_on = dict(zip(pt, pw))
    holder = np.full(n, -1, np.int64)
    needs = [dict() for _ in range(W)]
    nproc, scan = [0] * W, [False] * W
    left = np.diff(ptr).copy()
    src = np.repeat(np.arange(n), np.diff(ptr))
    dpt = src[np.lexsort((prio[src], idx))]
    dptr = np.zeros(n + 1, np.int64)
    if len(idx):
        dptr[1:] = np.cumsum(np.bincount(idx, minlength=n))

    def place(x, w):
        nproc[w] += 1
        for d in idx[ptr[x]:ptr[x + 1]].tolist():
            if holder[d] != w:
                needs[w][d] = needs[w].get(d, 0) + 1
        if len(needs[w]) > cap:
            scan[w] = True

    for t in pt[:int(out["round_nplaced"][0])]:  # update_graph's placements
        place(t, placed_on[t])
    refills = scanning = 0
    for r, (t, w) in enumerate(zip(pt, pw)):
        holder[t] = w
        nproc[w] -= 1
        tdeps = set(idx[ptr[t]:ptr[t + 1]].tolist())
        for d in tdeps:
            if d in needs[w]:
                needs[w][d] -= 1
                if not needs[w][d]:
                    del needs[w][d]
        if nproc[w] == 0:
            scan[w] = False
        local = c["reason"][r] == 0
        scanning += bool(local and scan[w])
        for x in dpt[dptr[t]:dptr[t + 1]].tolist():
            left[x] -= 1
            if left[x]:
                continue
            wx = placed_on[x]
            if local and wx == w and scan[w] and any(
                    d in tdeps and holder[d] != w and d not in needs[w] for d in idx[ptr[x]:ptr[x + 1]].tolist()):
                refills += 1
            place(x, wx)
    return refills, scanning

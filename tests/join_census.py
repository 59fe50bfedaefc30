"""What a ``svcaddw_*`` stream reaches, from the fixture's own arrays (test infrastructure,
CPU only; tests/test_join_census.py asserts on it, tests/test_gpu_join_rows.py uses the
label bookkeeping).

Worker indices in a fixture are "of their time": a join at a position below the worker
count moves every later index up by one (the canonical index is the SortedDict rank of the
address, distributed/scheduler.py:3746, :4353). The walk below gives every worker a label
that never changes -- the initial workers 0..W0-1 keep their first index, joiner k is
W0 + k -- and replays ``add_msg`` / ``add_pos`` to know, at every event, which label sits at
which index. The events of a stream, in order: per message m the joins with add_msg == m,
the resumes with res_msg == m, then completion m; ``stim_nplaced`` holds the placements of
update_graph and then of each event.
"""
import numpy as np


def events(z):
    """[(kind, k)] in stream order: ("join", k), ("resume", k), ("done", m)."""
    M = len(z["msg_task"])
    joins, resumes = {}, {}
    for k, m in enumerate(z["add_msg"].tolist()):
        joins.setdefault(m, []).append(k)
    for k, m in enumerate((z["res_msg"].tolist() if "res_msg" in z else [])):
        resumes.setdefault(m, []).append(k)
    ev = []
    for m in range(M):
        ev += [("join", k) for k in joins.get(m, ())]
        ev += [("resume", k) for k in resumes.get(m, ())]
        ev.append(("done", m))
    return ev


def join_positions(W0, z):
    """add_pos, or the append positions of a fixture from before it was stored."""
    n = len(z["add_nthreads"])
    return z["add_pos"].tolist() if "add_pos" in z else [W0 + k for k in range(n)]


def relabel(W0, add_pos, n_events_placed, pl_worker):
    """Labels of ``pl_worker`` (indices of their time). ``n_events_placed[k]``: how many
    placements had been made when join k happened."""
    order = list(range(W0))
    out = np.array(pl_worker, np.int64)
    lo = 0
    for k, p in enumerate(add_pos):
        hi = n_events_placed[k]
        out[lo:hi] = np.array(order, np.int64)[out[lo:hi]]
        order.insert(p, W0 + k)
        lo = hi
    out[lo:] = np.array(order, np.int64)[out[lo:]]
    return out


def join_census(g, z):
    """Walk the stream once. Returns a dict of plain facts (see the keys at the end)."""
    W0 = len(g["nthreads"])
    N = int(g["n_tasks"])
    flags = g["restr_flags"] if g.get("restr_flags") is not None else np.zeros(N, np.uint8)
    rptr = g["restr_ptr"] if g.get("restr_ptr") is not None else np.zeros(N + 1, np.int64)
    ridx = g["restr_idx"] if g.get("restr_idx") is not None else np.zeros(0, np.int32)
    restricted = (flags & 1) != 0
    pos = join_positions(W0, z)
    running = z["add_running"].tolist() if "add_running" in z else [1] * len(pos)
    stim = z["stim_nplaced"].tolist()
    pl_task, pl_worker = z["pl_task"].tolist(), z["pl_worker"].tolist()
    ev = events(z)
    assert len(stim) == 1 + len(ev) and sum(stim) == len(pl_task)
    placed_at = {t: i for i, t in enumerate(pl_task)}  # each task is placed once in these streams
    assert len(placed_at) == len(pl_task)
    dep_ptr, dep_idx = g["dep_ptr"], g["dep_idx"]
    dependents = [[] for _ in range(N)]
    for t in range(N):
        for d in dep_idx[dep_ptr[t]:dep_ptr[t + 1]].tolist():
            dependents[d].append(t)

    n, at_join = stim[0], []
    for e, (kind, k) in enumerate(ev):
        if kind == "join":
            at_join.append(n)
        n += stim[1 + e]
    pl_label = relabel(W0, pos, at_join, pl_worker).tolist()  # the placement log in labels

    order = list(range(W0))          # index -> label
    at = {l: l for l in range(W0)}   # label -> index
    ran_on = {}                      # completed task -> label of the worker holding its result
    joins = []                       # per join: dict(pos, W, placed, restr_after)
    first = None                     # position of the first insertion
    moved_rows = moved_placed = 0
    resumed = False
    refill_resumes = 0               # queued tasks the resumes took
    restr_after_resume = 0
    W4 = False                       # a who_has bit carried across the word boundary is read again
    n = stim[0]
    res_worker = z["res_worker"].tolist() if "res_worker" in z else []
    paused = set()

    def place(lo, hi):
        nonlocal moved_rows, moved_placed, restr_after_resume
        for i in range(lo, hi):
            t, w = pl_task[i], pl_worker[i]
            lab = order[w]
            assert lab == pl_label[i]
            assert lab not in paused, ("a placement on a paused worker", i, t, w)
            if not restricted[t]:
                continue
            for j in joins:
                j["restr_after"] += 1
            if resumed:
                restr_after_resume += 1
            row = ridx[rptr[t]:rptr[t + 1]].tolist()  # labels: the rows name initial workers
            if row:
                assert lab in row or (flags[t] & 2), ("a restricted task outside its row", i, t, w, row)
            if first is not None and any(at[l] >= first for l in row):
                moved_rows += 1
                if lab < W0 and at[lab] != lab and lab in row:
                    moved_placed += 1

    for e, (kind, k) in enumerate(ev):
        if kind == "join":
            p, W = pos[k], len(order)
            assert 0 <= p <= W, (k, p, W)
            if p <= 63 < W:  # the worker at index 63 moves to 64: its who_has bits change word
                # a result it holds with a dependent not yet placed stays in memory until that
                # dependent has run, and its placement reads the bit (the comm bytes)
                W4 = W4 or any(placed_at[d] >= n for t, l in ran_on.items() if l == order[63] for d in dependents[t])
            order.insert(p, W0 + k)
            at = {l: i for i, l in enumerate(order)}
            if not running[k]:
                paused.add(W0 + k)
            if p < W and first is None:
                first = p
            joins.append(dict(pos=p, W=W, placed=stim[1 + e], restr_after=0, running=bool(running[k])))
        elif kind == "resume":
            lab = order[res_worker[k]]
            assert lab in paused, ("a resume of a worker that is not paused", k, res_worker[k])
            paused.discard(lab)
            resumed = True
            refill_resumes += stim[1 + e]
        else:
            t = z["msg_task"][k].item()
            lab = order[z["msg_worker"][k].item()]
            # the message names the worker the task was placed on, by its index of now
            assert lab == pl_label[placed_at[t]], (k, t)
            ran_on[t] = lab
        place(n, n + stim[1 + e])
        n += stim[1 + e]
    widths = np.diff(rptr)[restricted]
    return dict(
        W0=W0, joins=joins, n_inserted=sum(j["pos"] < j["W"] for j in joins), first_insertion=first,
        moved_rows=moved_rows, moved_placed=moved_placed,
        n_paused=sum(not j["running"] for j in joins), n_resumes=len(res_worker),
        restr_after_resume=restr_after_resume,
        refill=sum(j["placed"] for j in joins) + refill_resumes,
        row_widths=sorted(set(widths.tolist())),
        strict_empty_rows=int(((np.diff(rptr) == 0) & restricted & ((flags & 2) == 0)).sum()),
        W4=W4, order=order, pl_label=pl_label, on_joiners=sum(l >= W0 for l in pl_label))

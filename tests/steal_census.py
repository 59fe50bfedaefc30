"""Which paths of the device ``balance()`` a steal problem reaches (CPU, numpy / Python).

``census(p, ref)`` replays one ``WorkStealing.balance()`` (reference stealing.py:401-503)
over problem ``p`` in the reference's order, but with the bookkeeping of ``k_balance``
(distributed_amd/csrc/dgp_steal.h): every bin is walked in chunks of 64
tasks, each task carries the thief precomputed over the *initial* thief set, a window
runs from task ``j`` to the first task ``d`` whose thief has left, the accepted prefix
``[j, b)`` ends at the first rejection or just after the first fill, and every task from
``d`` on whose thief has left gets a batched search over the runs of equal stack time.

Before it reports anything it asserts that its own request list (task, thief, in order)
is ``ref``'s (the oracle's or the reference's) -- otherwise the counts mean nothing. It
returns a ``collections.Counter`` over the names in ``SITES``. This is a model of the
kernel's control flow for the tests' census, not a checker of values: values are compared
bit-for-bit elsewhere (test_oracle_steal.py, test_gpu_steal*.py).
"""
from __future__ import annotations

from collections import Counter

import numpy as np

N_LEVELS = 15
MAXH = 4
NO_THIEF = -2

SITES = (
    # bins and chunks
    "bin.size1", "bin.size63", "bin.size64", "bin.size65", "bin.size128", "bin.size129",
    "chunk.prefix_to_lane63_with_repeat",
    # windows
    "win.repeat", "win.prefix_splits_repeat", "win.fill_repeats_later", "win.reject_after_fill_same",
    "win.reject_after_fill_other", "win.reject_lane0", "win.thieves_exhausted_midchunk",
    # searches
    "search.batched", "search.again", "rows.nh0", "rows.nh1", "rows.nh2", "rows.nh3", "rows.nh4", "rows.many",
    "restr.valid", "restr.none_loose", "restr.none_strict", "search.live_runs_gt64", "search.past_window",
    "search.winner_not_first_run", "search.crossed_empty_run", "search.first_run_changed", "search.tie_in_run",
    "search.tie_across_runs", "search.tie_across_runs_by_index", "search.holder_wins", "search.holder_tie_wins", "search.holder_tie_loses",
    "search.holder_at_min_start", "search.holder_first_of_run",
    # victims
    "vict.topk_w_lt10", "vict.topk_w_ge10", "vict.topk_tie", "vict.sort_tie", "vict.nsat19", "vict.nsat20",
    "vict.live_left_sat", "vict.occ_negative",
    # inputs
    "in.level_in_neg", "in.inflight_in", "in.nthreads_mixed",
)


def holders_csr(p):
    if "holder_ptr" in p:
        return np.asarray(p["holder_ptr"], np.int64), np.asarray(p["holder_idx"], np.int32)
    h = np.asarray(p["data_holder"], np.int32)
    ptr = np.zeros(len(h) + 1, np.int64)
    ptr[1:] = np.cumsum(h >= 0)
    return ptr, h[h >= 0].astype(np.int32)


def thief_runs(p):
    """(initial thieves, runs of equal stack time among them, size of the run at 0.0)."""
    idle = np.asarray(p["idle"]) != 0
    a = (np.asarray(p["occ"], np.float64) / np.asarray(p["nthreads"], np.float64))[idle] + 0.0
    return int(idle.sum()), len(np.unique(a)), int((a == 0.0).sum())


def byte_sum_bound(p):
    """The largest byte sum the engine can form over ``p`` (below 2**53)."""
    dep_ptr = np.asarray(p["dep_ptr"], np.int64)
    dep_idx = np.asarray(p["dep_idx"], np.int64)
    T = len(dep_ptr) - 1
    src = np.repeat(np.arange(T), np.diff(dep_ptr))
    m = 0
    for k in ("data_nbytes", "data_get_nbytes"):
        per = np.zeros(T, object)
        np.add.at(per, src, np.asarray(p[k], np.int64)[dep_idx].astype(object))
        m = max(m, int(max(per, default=0)))
    return max(m, int(np.asarray(p["wnbytes"]).max(initial=0)))


def census(p, ref):
    c = Counter()
    W = len(p["nthreads"])
    T = len(p["victim"])
    nth = np.asarray(p["nthreads"], np.int64)
    occ = [float(x) + 0.0 for x in np.asarray(p["occ"], np.float64)]
    nproc = [int(x) for x in p["nproc"]]
    wnb = [int(x) for x in p["wnbytes"]]
    bw = float(int(p["bandwidth"]))
    victim = np.asarray(p["victim"], np.int64)
    dur = [float(x) for x in np.asarray(p["duration"], np.float64)]
    dep_ptr = np.asarray(p["dep_ptr"], np.int64)
    dep_idx = np.asarray(p["dep_idx"], np.int64)
    hptr, hidx = holders_csr(p)
    dg = np.asarray(p["data_get_nbytes"], np.int64)
    dr = np.asarray(p["data_nbytes"], np.int64)
    level = np.asarray(ref["level"], np.int64)
    rfl = np.asarray(p["restr_flags"]) if p.get("restr_flags") is not None else None
    rptr = np.asarray(p["restr_ptr"], np.int64) if rfl is not None else None
    ridx = np.asarray(p["restr_idx"], np.int64) if rfl is not None else None
    avg = float(p["total_occ"]) / float(int(p["total_nthreads"]))

    # ---- inputs
    if p.get("level_in") is not None and (np.asarray(p["level_in"]) < 0).any():
        c["in.level_in_neg"] += int((np.asarray(p["level_in"]) < 0).sum())
    for k in ("inflight_occ_in", "inflight_tasks_in"):
        if p.get(k) is not None:
            c["in.inflight_in"] += int(np.count_nonzero(np.asarray(p[k])))
    if (nth == 1).any() and (nth >= 64).any():  # workers at either end of a mixed cluster
        c["in.nthreads_mixed"] += int((nth == 1).sum() + (nth >= 64).sum())

    # ---- task rows (k_best_thief): byte sums and what each worker holds of each task
    cget = np.zeros(T, np.int64)
    craw = np.zeros(T, np.int64)
    held_g = np.zeros((T, W), np.int64)
    held_r = np.zeros((T, W), np.int64)
    nhold = np.zeros(T, np.int64)
    src = np.repeat(np.arange(T), np.diff(dep_ptr))
    np.add.at(cget, src, dg[dep_idx])
    np.add.at(craw, src, dr[dep_idx])
    for t, d in zip(src, dep_idx):
        hs = hidx[hptr[d]:hptr[d + 1]]
        held_g[t, hs] += dg[d]
        held_r[t, hs] += dr[d]
    holder_of = [None] * T  # distinct holders in first-seen order (the row's hw)
    for t in range(T):
        seen = []
        for d in dep_idx[dep_ptr[t]:dep_ptr[t + 1]]:
            for h in hidx[hptr[d]:hptr[d + 1]]:
                if int(h) not in seen:
                    seen.append(int(h))
        holder_of[t] = seen
        nhold[t] = len(seen)
    a = np.array([occ[w] / float(nth[w]) for w in range(W)])

    def start_row(t):  # worker_objective's start of task t on every worker
        return a + (cget[t] - held_g[t]).astype(np.float64) / bw

    def cct(t, w):
        return float(int(craw[t] - held_r[t, w])) / bw

    def argmin(t, mask):
        idx = np.flatnonzero(mask)
        if len(idx) == 0:
            return -1
        s = start_row(t)[idx]
        idx = idx[s == s.min()]
        return min(idx, key=lambda w: (wnb[w], w))

    def valid_mask(t):
        m = np.zeros(W, bool)
        m[ridx[rptr[t]:rptr[t + 1]]] = True
        return m

    thief = np.asarray(p["idle"]) != 0
    idle = [int(x) for x in p["idle"]]
    sat = [int(x) for x in p["sat"]]
    n_thieves = int(thief.sum())
    ifo = [float(x) for x in p["inflight_occ_in"]] if p.get("inflight_occ_in") is not None else [0.0] * W
    pend = [nproc[w] + (int(p["inflight_tasks_in"][w]) if p.get("inflight_tasks_in") is not None else 0)
            for w in range(W)]
    req = []

    def done():
        got = (np.array([r[0] for r in req], np.int64), np.array([r[1] for r in req], np.int64))
        exp = (np.asarray(ref["st_task"], np.int64), np.asarray(ref["st_thief"], np.int64))
        assert len(got[0]) == len(exp[0]), ("census walk: request count", len(got[0]), len(exp[0]))
        assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1]), "census walk: requests differ"
        for k, x in (("inflight_occ", ifo), ("idle_after", idle), ("sat_after", sat)):
            assert np.array_equal(np.asarray(x, np.asarray(ref[k]).dtype), np.asarray(ref[k])), ("census walk", k)
        return c

    if n_thieves == 0 or n_thieves == W:
        return done()

    # ---- thief order and runs (k_thief_keys, the two sorts, k_runs)
    th_order = sorted(np.flatnonzero(thief).tolist(), key=lambda w: (a[w], wnb[w], w))
    run_start, run_a, run_of = [], [], {}
    for q, w in enumerate(th_order):
        if q == 0 or a[w] != a[th_order[q - 1]]:
            run_start.append(q)
            run_a.append(float(a[w]))
        run_of[w] = len(run_a) - 1
    R = len(run_a)
    run_start.append(len(th_order))
    run_alive = [run_start[r + 1] - run_start[r] for r in range(R)]

    # ---- the precomputed thief of every stealable task, over the initial thief set
    pre = np.full(T, -1, np.int64)
    for t in np.flatnonzero(level >= 0):
        if rfl is not None and rfl[t] & 1:
            w = argmin(t, thief & valid_mask(t))
            if w < 0:
                w = argmin(t, thief) if rfl[t] & 2 else NO_THIEF
        else:
            w = argmin(t, thief)
        pre[t] = w

    # ---- victims (:412-428)
    comb = lambda w: occ[w] + ifo[w]  # noqa: E731
    nsat = sum(sat)
    live = False
    if nsat:
        c["vict.nsat19"] += nsat == 19
        c["vict.nsat20"] += nsat == 20
        pv = [w for w in range(W) if sat[w]]
        live = nsat >= 20
    else:
        c["vict.topk_w_lt10" if W < 10 else "vict.topk_w_ge10"] += 1
        allw = sorted(range(W), key=lambda w: -comb(w))
        c["vict.topk_tie"] += sum(comb(allw[i]) == comb(allw[i + 1]) for i in range(min(10, W - 1)))
        pv = [w for w in allw[:10] if comb(w) > 0.2 and pend[w] > nth[w] and not thief[w]]
        if not pv:
            return done()
    if not live:
        pv = sorted(pv, key=lambda w: -comb(w))
        c["vict.sort_tie"] += sum(comb(pv[i]) == comb(pv[i + 1]) for i in range(len(pv) - 1))

    bins = {}
    for t in np.flatnonzero(level >= 0):
        bins.setdefault((int(level[t]), int(victim[t])), []).append(int(t))

    wc_r0 = -1  # the first live run the search's window of run stack times starts at
    ever_victim, left_sat = set(), set()

    def first_live_run(r):
        while r < R and run_alive[r] == 0:
            r += 1
        return r

    def general_search(t):
        """The run-ordered search of one task: (winner, sites)."""
        nonlocal wc_r0
        hs = holder_of[t]
        x = float(int(cget[t])) / bw
        rf = first_live_run(0)
        if rf > 0:
            c["search.crossed_empty_run"] += 1
        if rf != wc_r0:
            if wc_r0 >= 0:
                c["search.first_run_changed"] += 1
            wc_r0 = rf
        if sum(1 for r in range(R) if run_alive[r]) > 64:
            c["search.live_runs_gt64"] += 1
        r, bs, bwk, win_run = rf, None, None, -1
        past = crossed = tie_across = tie_index = first_holder = False
        while r < R:
            sv = run_a[r] + x
            if bwk is not None and sv > bs:
                break
            past |= r - rf >= 64
            livew = [w for w in th_order[run_start[r]:run_start[r + 1]] if thief[w]]
            first_holder |= livew[0] in hs
            cand = [w for w in livew if w not in hs]
            if cand:
                if bwk is None:
                    bs, bwk, win_run = sv, cand[0], r
                elif sv == bs:
                    tie_across = True
                    tie_index |= wnb[cand[0]] == wnb[bwk] and cand[0] < bwk  # equal ws.nbytes: the index decides
                    if (wnb[cand[0]], cand[0]) < (wnb[bwk], bwk):
                        bwk, win_run = cand[0], r
            nx = first_live_run(r + 1)
            crossed |= nx > r + 1 and nx < R
            r = nx
        n_in_run = 0
        if bwk is not None:
            n_in_run = sum(1 for w in th_order[run_start[win_run]:run_start[win_run + 1]] if thief[w] and w not in hs)
        # then the live holders, each with its own comm term
        hold_win = False
        hb = min(((occ[h] / float(nth[h]) + float(int(cget[t] - held_g[t, h])) / bw, wnb[h], h)
                  for h in hs if thief[h]), default=None)
        if hb is not None:
            if bwk is None or hb[0] < bs:
                hold_win = True
            elif hb[0] == bs:
                hold_win = hb[1:] < (wnb[bwk], bwk)
                c["search.holder_tie_wins" if hold_win else "search.holder_tie_loses"] += 1
            c["search.holder_at_min_start"] += hold_win or hb[0] == bs
            if hold_win:
                bwk = hb[2]
        c["search.past_window"] += past
        c["search.crossed_empty_run"] += crossed and rf == 0
        c["search.tie_across_runs"] += tie_across
        c["search.tie_across_runs_by_index"] += tie_index
        c["search.holder_first_of_run"] += first_holder
        if hold_win:
            c["search.holder_wins"] += 1
        else:
            c["search.tie_in_run"] += n_in_run > 1
        c["search.winner_not_first_run"] += run_of[bwk] != rf
        return bwk

    for lv in range(N_LEVELS):
        if n_thieves == 0:
            break
        vs = [w for w in range(W) if sat[w]] if live else pv
        if live:  # each victim once, at the first level it is absent from
            gone = ever_victim - set(vs) - left_sat
            c["vict.live_left_sat"] += len(gone)
            left_sat |= gone
            ever_victim |= set(vs)
        for v in vs:
            tasks = bins.get((lv, v), [])
            if not tasks or n_thieves == 0:
                continue
            if len(tasks) in (1, 63, 64, 65, 128, 129):
                c[f"bin.size{len(tasks)}"] += 1
            occ_v, ifo_v, pend_v = occ[v], ifo[v], pend[v]
            for c0 in range(0, len(tasks), 64):
                ch = tasks[c0:c0 + 64]
                nq = len(ch)
                th = [int(pre[t]) for t in ch]
                cq = [cct(t, w) if w >= 0 else 0.0 for t, w in zip(ch, th)]
                vq = [cct(t, v) for t in ch]
                dq = [dur[t] for t in ch]
                alive = [w >= 0 and bool(thief[w]) for w in th]
                nsearch = [0] * nq
                j = 0
                while j < nq and n_thieves > 0:
                    todo = [l for l in range(j, nq) if th[l] != NO_THIEF]
                    d = next((l for l in todo if not (th[l] >= 0 and alive[l])), nq)
                    inw = [l for l in todo if l < d]
                    lanes_of = {}
                    for l in inw:
                        lanes_of.setdefault(th[l], []).append(l)
                    rep = any(len(v_) > 1 for v_ in lanes_of.values())
                    c["win.repeat"] += rep
                    # every lane's accounts as if the window's earlier tasks were all accepted
                    vb, tb, pb = {}, {}, {}
                    run = ifo_v
                    inws = set(inw)
                    for k in range(j, d):
                        vb[k] = run
                        run = run - (dq[k] + vq[k] if k in inws else 0.0)
                    for x_, ls in lanes_of.items():
                        cur = ifo[x_]
                        for n_, k in enumerate(ls):
                            tb[k] = cur
                            pb[k] = pend[x_] + n_
                            cur = cur + (dq[k] + cq[k])
                    fb = ff = 64
                    for l in inw:
                        w = th[l]
                        ot, ov = occ[w] + tb[l], occ_v + vb[l]
                        acc = ot + cq[l] + dq[l] <= ov - (vq[l] + dq[l]) / 2
                        nt = int(nth[w])
                        full = acc and not ((pb[l] + 1) < nt or occ[w] + (tb[l] + (dq[l] + cq[l])) < nt * avg / 2)
                        if not acc and fb == 64:
                            fb = l
                        if full and ff == 64:
                            ff = l
                    b = min(fb, ff + 1, d)
                    com = [l for l in inw if l < b]
                    if rep and b >= 64:
                        c["chunk.prefix_to_lane63_with_repeat"] += 1
                    for x_, ls in lanes_of.items():
                        inn = [l for l in ls if l < b]
                        if inn and len(inn) < len(ls):
                            c["win.prefix_splits_repeat"] += 1
                        if inn:
                            last = inn[-1]
                            ifo[x_] = tb[last] + (dq[last] + cq[last])
                            pend[x_] = pb[last] + 1
                    ifo_v = vb[b] if b < d else run
                    for l in com:
                        req.append((ch[l], th[l]))
                    pend_v -= len(com)
                    if fb == j:
                        c["win.reject_lane0"] += 1
                    if ff < b:
                        x_ = th[ff]
                        if lanes_of[x_][-1] > ff:
                            c["win.fill_repeats_later"] += 1
                        if fb == ff + 1 and fb < 64:
                            c["win.reject_after_fill_same" if th[fb] == x_ else "win.reject_after_fill_other"] += 1
                        thief[x_] = False
                        run_alive[run_of[x_]] -= 1
                        n_thieves -= 1
                        for l in range(nq):
                            if th[l] == x_:
                                alive[l] = False
                        if n_thieves == 0 and b < nq:
                            c["win.thieves_exhausted_midchunk"] += 1
                    j = b + 1 if (fb <= ff and b == fb) else b
                    if b != d or d >= nq or n_thieves == 0:
                        continue
                    # the batched search: every task from d on whose thief has left
                    sl = [l for l in range(d, nq) if th[l] != NO_THIEF and not (th[l] >= 0 and alive[l])]
                    c["search.batched"] += len(sl) > 1
                    for l in sl:
                        t = ch[l]
                        nsearch[l] += 1
                        c["search.again"] += nsearch[l] == 2
                        w = -1
                        if rfl is not None and rfl[t] & 1:
                            w = argmin(t, thief & valid_mask(t))
                            if w >= 0:
                                c["restr.valid"] += 1
                            elif rfl[t] & 2:
                                c["restr.none_loose"] += 1
                            else:
                                c["restr.none_strict"] += 1
                                w = NO_THIEF
                        if w == -1:
                            brute = argmin(t, thief)
                            if nhold[t] > MAXH:
                                c["rows.many"] += 1
                                w = brute
                            else:
                                c[f"rows.nh{nhold[t]}"] += 1
                                w = general_search(t)
                                assert w == brute, ("census search", t, w, brute)
                        th[l] = int(w)
                        alive[l] = w >= 0
                        cq[l] = cct(t, w) if w >= 0 else 0.0
            ifo[v], pend[v] = ifo_v, pend_v
            # check_idle_saturated(victim, occ=combined) (scheduler.py:2949-2995)
            o = comb(v)
            if o < 0:
                c["vict.occ_negative"] += 1
                o = occ[v]
            pn, nc = nproc[v], int(nth[v])
            idle[v] = sat[v] = 0
            if pn < nc or o < nc * avg / 2:
                idle[v] = 1
            elif pn > nc:
                pending = o * float(pn - nc) / float(pn * nc)
                if 0.4 < pending and pending > 1.9 * avg:
                    sat[v] = 1
    return done()

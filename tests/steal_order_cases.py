"""Steal problems as the plugin hands them to the device: task rows in slots, out of walk
order, with a ``(task_prio, task_arrival)`` key per row (``StealRows.problem`` ->
``dgp_steal_order``: the device sorts the rows itself).

A problem in walk order (a ``tests/golden/steal_*.npz`` fixture, a ``steal_cases`` problem)
is relabelled: ``slotted`` puts its tasks into slots by a permutation and gives them keys
whose ascending (priority, arrival) order -- slot order between equal pairs -- is the
original order. Whatever the device answers for the slotted problem must then be the
original's expected answer with the task ids relabelled (``map_back``). ``WRONG`` names the
orders a mistaken device sort would walk in instead; tests/test_steal_order_cases.py shows on
the CPU, with the oracle, that each of them changes the requests of a named case.

Nothing here touches the device: numpy, ``stealing.pack_priority`` and, for the cases at the end,
the oracle."""
from __future__ import annotations

import functools
import os

import numpy as np

from distributed_amd.stealing import pack_priority

I64 = np.iinfo(np.int64)
SCHEMES = ("rank", "wide", "packed", "extremes", "dupes")
DUPES = 5  # positions that share one key pair in the "dupes" scheme


def _csr_gather(ptr, idx, rows):
    """Rows ``rows`` of the CSR (ptr, idx) -> (ptr, idx) of those rows in that order."""
    ptr = np.asarray(ptr, np.int64)
    cnt = np.diff(ptr)[rows]
    new = np.zeros(len(rows) + 1, np.int64)
    np.cumsum(cnt, out=new[1:])
    src = np.repeat(ptr[:-1][rows], cnt) + (np.arange(int(new[-1]), dtype=np.int64) - np.repeat(new[:-1], cnt))
    return new, np.asarray(idx, np.int32)[src]


def reorder(p, idx):
    """``p`` with its task rows gathered by ``idx`` (row k of the result is row idx[k] of
    ``p``): victim, duration, fast, level_in if present, the dependency CSR, the restriction
    CSR and flags if present. Worker and data arrays, and any keys, are left as they are."""
    idx = np.asarray(idx, np.int64)
    q = dict(p)
    for k in ("victim", "duration", "fast"):
        q[k] = np.asarray(p[k])[idx]
    if p.get("level_in") is not None:
        q["level_in"] = np.asarray(p["level_in"])[idx]
    q["dep_ptr"], q["dep_idx"] = _csr_gather(p["dep_ptr"], p["dep_idx"], idx)
    if p.get("restr_flags") is not None:
        q["restr_ptr"], q["restr_idx"] = _csr_gather(p["restr_ptr"], p["restr_idx"], idx)
        q["restr_flags"] = np.asarray(p["restr_flags"])[idx]
    return q


def unkeyed(q):
    return {k: v for k, v in q.items() if k not in ("task_prio", "task_arrival")}


def _keys(scheme, pos, slot):
    """(prio, arrival) of the tasks at walk positions ``pos`` (held in slots ``slot``)."""
    i = pos.astype(np.int64)
    T = len(i)
    if scheme == "rank":  # what StealRows sends when a priority does not pack (pk_bad)
        return i.copy(), np.zeros(T, np.int64)
    if scheme == "wide":
        # both keys on both sides of 0, decided above bit 32; priority constant over 7
        # positions, arrival deciding inside; the low 32 bits of both run against the order
        g, G = i // 7, (T + 6) // 7
        return ((g - G // 2) << 33) | ((G - g) & 0xffff), ((i % 7) - 3) * (1 << 40) + (6 - i % 7)
    if scheme == "packed":
        # TaskState.priority as the plugin packs it: (a, b) constant over a sixteenth of the
        # positions, the dask.order position c deciding inside -- below bit 27, so two keys
        # of a group agree in their high 32 bits; arrival counts the slots
        A = (-(1 << 15), -1, 0, (1 << 15) - 1)
        B = (0, 31, 32, (1 << 20) - 1)  # 0 / 31 and 32 / 2^20 - 1 differ below / above bit 32 of the key
        n16 = -(-T // 16)
        grp = i // n16
        c = (i % n16) * (((1 << 27) - 1) // max(n16 - 1, 1))
        prio = np.array([pack_priority((A[int(g) // 4], B[int(g) % 4], int(cc))) for g, cc in zip(grp, c)], np.int64)
        return prio, slot.astype(np.int64)
    if scheme == "extremes":
        # INT64_MIN, -1, 0 and INT64_MAX in both keys: priority one of the four over a quarter
        # of the positions, arrival ascending inside through four runs: up from INT64_MIN, up
        # to -1, up from 0, up to INT64_MAX (neighbours differ in their lowest bits only)
        n4 = -(-T // 4)
        n16 = -(-n4 // 4)
        prio = np.array([I64.min, -1, 0, I64.max], np.int64)[i // n4]
        j = i % n4
        run, r = j // n16, j % n16
        arr = np.where(run == 0, I64.min + r,
                       np.where(run == 1, r - n16, np.where(run == 2, r, I64.max - (n4 - 1 - j))))
        return prio, arr.astype(np.int64)
    if scheme == "dupes":
        # groups of DUPES positions share one (priority, arrival) pair: slot order decides
        g, G = i // DUPES, (T + DUPES - 1) // DUPES
        return g // 3 - G // 6, g % 3 - 1
    raise ValueError(scheme)


def slotted(p, pi, scheme):
    """``p`` (in walk order) with the task of walk position pi[s] in slot s, and the keys of
    ``scheme``: ``np.lexsort((task_arrival, task_prio))`` of the result -- stable, so slot
    order between equal pairs -- restores the original order exactly. Returns (problem, pi):
    the ``dupes`` scheme first sorts the slots of each group of equal pairs, so that slot
    order is the original order there; every other scheme returns ``pi`` as given."""
    pi = np.asarray(pi, np.int64).copy()
    T = len(pi)
    assert T == len(p["victim"]) and np.array_equal(np.sort(pi), np.arange(T))
    if scheme == "dupes":
        inv = np.argsort(pi)  # slot of each position
        for a in range(0, T, DUPES):
            inv[a:a + DUPES] = np.sort(inv[a:a + DUPES])
        pi = np.argsort(inv)
    q = reorder(p, pi)
    q["task_prio"], q["task_arrival"] = _keys(scheme, pi, np.arange(T))
    assert q["task_prio"].dtype == q["task_arrival"].dtype == np.int64
    assert np.array_equal(pi[np.lexsort((q["task_arrival"], q["task_prio"]))], np.arange(T)), scheme
    return q, pi


def map_back(out, pi, perm=None):
    """Oracle outputs on a problem in walk order -> the same with the tasks named by their
    slots, as the device names them: ``st_task`` through the permutation, ``level``
    scattered; everything else is per request or per worker and stays. ``perm``: the walk
    the oracle's problem was put in (its row k is slot perm[k]); by default the right one,
    the inverse of ``pi``."""
    if perm is None:
        perm = np.argsort(np.asarray(pi, np.int64))
    perm = np.asarray(perm, np.int64)
    res = dict(out)
    res["st_task"] = perm[np.asarray(out["st_task"], np.int64)].astype(np.int32)
    lv = np.empty_like(np.asarray(out["level"]))
    lv[perm] = out["level"]
    res["level"] = lv
    return res


def _u(x):
    return x.astype(np.uint64)


def _unstable(p, a):
    slot = np.arange(len(p))
    return np.lexsort((-slot, a, p))


# the walks a mistaken device sort would give, as functions of (prio, arrival) in slot order
WRONG = {
    "slot_order": lambda p, a: np.arange(len(p)),                 # the keys ignored
    "prio_only": lambda p, a: np.argsort(p, kind="stable"),        # the arrival pass lost
    "arrival_major": lambda p, a: np.lexsort((p, a)),              # the passes swapped
    "unsigned_prio": lambda p, a: np.lexsort((a, _u(p))),          # a sign flip lost
    "unsigned_arrival": lambda p, a: np.lexsort((_u(a), p)),
    "low32_prio": lambda p, a: np.lexsort((a, p & 0xffffffff)),    # a key compared on 32 bits
    "low32_arrival": lambda p, a: np.lexsort((a & 0xffffffff, p)),
    "high32_prio": lambda p, a: np.lexsort((a, p >> 32)),
    "high32_arrival": lambda p, a: np.lexsort((a >> 32, p)),
    "descending": lambda p, a: np.lexsort((a, p))[::-1],
    "unstable_ties": _unstable,                                    # slots reversed inside a tie
}


def wrong_walk(q, name):
    """The walk-order problem a device with mistake ``name`` would balance, and its walk."""
    perm = np.asarray(WRONG[name](q["task_prio"], q["task_arrival"]), np.int64)
    return reorder(unkeyed(q), perm), perm


# ------------------------------------------------------------------ the cases of the GPU test
# Built at their first use and kept: tests/test_steal_order_cases.py (CPU) and
# tests/test_gpu_steal_order.py run the same problems.
FIXTURE_SCHEMES = ("rank", "wide")
SCHEME_FIXTURES = ("steal_busy_small.npz", "steal_restricted_small.npz", "steal_busy_second.npz")
KEY_SCHEMES = ("packed", "extremes", "dupes")
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 4097)
ROWS_VARIANTS = ("packed", "pk_bad")
SEED = 5


@functools.lru_cache(maxsize=None)
def _fixture(name):
    from conftest import GOLDEN
    from oracle import oracle

    p, exp, meta = oracle.load_steal_fixture(os.path.join(GOLDEN, name))
    return p, exp


@functools.lru_cache(maxsize=None)
def fixture_case(name, scheme):
    """A reference fixture in slots -> (slotted problem, pi, the fixture's expected arrays)."""
    p, exp = _fixture(name)
    q, pi = slotted(p, np.random.default_rng(SEED).permutation(len(p["victim"])), scheme)
    return q, pi, exp


@functools.lru_cache(maxsize=None)
def aimed_case(name):
    """A ``steal_cases`` problem in slots with the ``wide`` keys; expected: the oracle's answer
    for the problem as it was."""
    import steal_cases
    from oracle import oracle

    p = steal_cases.problem(name)
    q, pi = slotted(p, np.random.default_rng(SEED + 1).permutation(len(p["victim"])), "wide")
    return q, pi, oracle.steal_balance(p)


@functools.lru_cache(maxsize=None)
def _size_base():
    from distributed_amd import graphs

    return graphs.steal_problem(16, max(SIZES), seed=77, hot_frac=0.25)


@functools.lru_cache(maxsize=None)
def size_case(T):
    """The first ``T`` tasks of one 16-worker problem (the workers as the whole problem loads
    them), with rows that are in no bin, so the last bin key is present: ``fast`` tasks under
    fresh levels for every other size, ``level_in`` = -1 for the sizes between."""
    from oracle import oracle

    b = _size_base()
    p = dict(b, victim=b["victim"][:T], duration=b["duration"][:T], fast=b["fast"][:T].copy(),
             dep_ptr=b["dep_ptr"][:T + 1], dep_idx=b["dep_idx"][:b["dep_ptr"][T]])
    t = np.arange(T)
    if SIZES.index(T) % 2 == 0:
        p["fast"][t % 5 == 3] = 1
    else:
        lv = oracle.steal_balance(p)["level"].copy()
        lv[t % 4 == 1] = -1
        p["level_in"] = lv
    q, pi = slotted(p, np.random.default_rng(SEED + T).permutation(T), "wide")
    return q, pi, oracle.steal_balance(p)


@functools.lru_cache(maxsize=None)
def rows_case(variant):
    """``StealRows.problem`` of the stand-in state of tests/steal_rows_state.py after its whole
    put / remove / re-put / replica sequence, on 160 workers of which the first 16 run the
    tasks -> (the problem as the plugin hands it over, None, the oracle's answer on it in
    walk order, named by the problem's rows). ``pk_bad``: one priority does not pack, so the
    keys are the host's ranks."""
    import steal_rows_state as SR
    from distributed_amd.stealing import ordered_problem
    from oracle import oracle

    st = SR.new_state(W=160, hot=16, restrict=0.15, unpackable=1700 if variant == "pk_bad" else None)
    for _ in SR.phases(st):
        pass
    assert not st.rows.free and len(st.rows.task) < 1500 + 500  # every freed slot was taken again
    for ts in st.tasks[5::13]:  # and some are free at the time of the balance
        SR.remove(st, ts)
    SR.load_workers(st, hot=16)
    p, slots, wss = st.rows.problem(st.plugin)
    assert bool(st.rows.pk_bad) == (variant == "pk_bad")
    assert st.rows.free and st.rows.more and st.rows.hmore and p.get("restr_flags") is not None
    perm = np.lexsort((p["task_arrival"], p["task_prio"]))
    walk, _ = ordered_problem(p, slots)
    return p, None, map_back(oracle.steal_balance(walk), None, perm)

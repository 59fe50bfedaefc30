"""Steal levels at their rounding boundaries.

``WorkStealing.steal_time_ratio`` (distributed/stealing.py:270-275) computes
``level = int(round(log2(cost_multiplier) + 6))``: CPython's ``math.log2`` (the C
library's ``log2``) and round-half-even. A level changes where ``log2(cm) + 6`` crosses
k + 0.5, i.e. at cm = 2^(k - 5.5). This sweeps the duration so that cm walks ±6 ulp
around every boundary of levels 0..16 and compares

* the oracle (oracle/steal.cpp, host ``std::log2``) — CPU, here;
* the HIP kernel (``k_steal_levels``: device ``log2`` + ``rint``, dgp_steal.h) — GPU;

with the reference expression evaluated by this Python (``math.log2``, ``round``).
"""
import math

import numpy as np
import pytest

from oracle import oracle

BW = 100_000_000
LATENCY = 0.1  # distributed/stealing.py:25


def sweep_problem(nb=1000, span=6, bw=BW):
    transfer = nb / bw + LATENCY
    durs = []
    for k in range(-1, 17):
        target = 2.0 ** (k - 5.5)
        c0 = transfer / target
        for j in range(-span, span + 1):
            c = c0
            step = math.inf if j > 0 else -math.inf
            for _ in range(abs(j)):
                c = float(np.nextafter(c, step))
            durs.append(c)
    durs = np.array(durs)
    T = len(durs)
    W = 4
    p = dict(nthreads=np.full(W, 2, np.int32), occ=np.array([50.0, 0.0, 1.0, 2.0]), nproc=np.array([T, 0, 1, 1], np.int32),
             wnbytes=np.zeros(W, np.int64), idle=np.array([0, 1, 0, 0], np.uint8), sat=np.array([1, 0, 0, 0], np.uint8),
             total_occ=53.0, total_nthreads=2 * W, bandwidth=bw, victim=np.zeros(T, np.int32), duration=durs,
             fast=np.zeros(T, np.uint8), dep_ptr=np.arange(T + 1, dtype=np.int64), dep_idx=np.zeros(T, np.int32),
             data_nbytes=np.array([nb], np.int64), data_get_nbytes=np.array([nb], np.int64),
             data_holder=np.array([0], np.int32))
    return p


def reference_levels(p):
    """stealing.py:255-275 on Python floats."""
    out = []
    for t in range(len(p["victim"])):
        nbytes = sum(int(p["data_get_nbytes"][d]) for d in p["dep_idx"][p["dep_ptr"][t]:p["dep_ptr"][t + 1]])
        if nbytes == 0 and p["dep_ptr"][t] == p["dep_ptr"][t + 1]:
            out.append(0)
            continue
        compute = float(p["duration"][t])
        cm = (nbytes / int(p["bandwidth"]) + LATENCY) / compute
        level = int(round(math.log2(cm) + 6))
        out.append(-1 if level >= 15 else max(level, 1))
    return np.array(out, np.int8)


def test_sweep_hits_half_integers():
    """The sweep really lands on cm values whose log2 + 6 is (or straddles) k + 0.5."""
    p = sweep_problem()
    cm = (1000 / BW + LATENCY) / p["duration"]
    x = np.log2(cm) + 6
    assert np.any(x == np.floor(x) + 0.5)  # exact ties: round-half-even decides


def test_oracle_levels_at_boundaries():
    p = sweep_problem()
    assert np.array_equal(oracle.steal_balance(p)["level"], reference_levels(p))


# other bandwidths than the reference's default (a deployment's distributed.scheduler.bandwidth;
# the extension passes the live scheduler's), with a dependency whose transfer is not latency
# alone: 5 GB (past 2^32 bytes) at 12.5 GB/s, 1 kB and 3 GB at 1 MB/s
OTHER_BW = [(12_500_000_000, 5_000_000_000), (12_500_000_000, 1000), (1_000_000, 1000), (1_000_000, 3_000_000_000)]


@pytest.mark.parametrize("bw,nb", OTHER_BW)
def test_oracle_levels_at_boundaries_other_bandwidths(bw, nb):
    p = sweep_problem(nb=nb, bw=bw)
    want = reference_levels(p)
    assert len(set(want.tolist())) >= 10  # the sweep still crosses the levels
    assert np.array_equal(oracle.steal_balance(p)["level"], want)
    if nb > 1000:  # the default bandwidth would give other levels
        assert not np.array_equal(reference_levels(dict(p, bandwidth=BW)), want)


@pytest.mark.gpu
@pytest.mark.parametrize("bw,nb", OTHER_BW)
def test_device_levels_at_boundaries_other_bandwidths(bw, nb):
    from distributed_amd.engine import PlacementEngine

    p = sweep_problem(nb=nb, bw=bw)
    with PlacementEngine(0) as eng:
        got = eng.steal_balance(p)["level"]
    want = reference_levels(p)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, [(float(p["duration"][i]), int(got[i]), int(want[i])) for i in bad[:5]]


@pytest.mark.gpu
def test_device_levels_at_boundaries():
    from distributed_amd.engine import PlacementEngine

    p = sweep_problem()
    with PlacementEngine(0) as eng:
        got = eng.steal_balance(p)["level"]
    want = reference_levels(p)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, [(float(p["duration"][i]), int(got[i]), int(want[i])) for i in bad[:5]]

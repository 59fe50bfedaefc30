"""The ``svcaddw_*`` join fixtures reach what they were made for (CPU only).

A worker that joins at an address sorting among the known ones makes the engine rewrite every
worker index it holds (``dgp_add_worker_at``): the per-worker rows, ``holder_of`` /
``proc_on``, the ``who_has`` bitsets (one bit up from the position, carried across 64-bit
words), the groups' last worker and the restriction rows, static and pooled. A stream
that never places a restricted task on a renumbered worker, or never carries a bit across
a word that is read again, would pass on an engine that is wrong there. So the conditions
below are asserted on the fixtures' own arrays -- the graph, the joins and the reference's
placement log, walked by ``join_census`` (tests/join_census.py). Nothing here measures the
code under test; the generator's seeds and ``near`` lists were chosen until the reference
alone satisfied every condition.

The last test replays each stream on the oracle with every joiner appended and compares the
placement logs in labels that do not depend on the indices (see its docstring for what that
can and cannot show). The oracle has no paused workers, so ``svcaddw_insrestr_sat1.1`` is
not part of it; its insertions are counted by the conditions above it.
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from join_census import join_census, relabel
from oracle import oracle

RESTR12 = "svcaddw_restr12_sat1.1"
INSERTED = ["svcaddw_insrestr_sat1.1", "svcaddw_insq_sat1.1", "svcaddw_insrestr_satinf", "svcaddw_ins64_sat1.1"]
UNPAUSED = [n for n in INSERTED if n != "svcaddw_insrestr_sat1.1"]  # the oracle restates no paused worker

_cache = {}


def census(name):
    """(graph, config, fixture arrays, census) of a fixture, computed once."""
    if name not in _cache:
        path = os.path.join(GOLDEN, name + ".npz")
        g, cfg, exp, meta = oracle.load_fixture(path)
        z = dict(np.load(path, allow_pickle=False))
        _cache[name] = (g, cfg, z, join_census(g, z))
    return _cache[name]


def test_census_on_a_stream_counted_by_hand():
    """Two workers, tasks 0 and 1 roots on workers 0 and 1, task 2 (restricted to worker 1)
    needs both. A worker joins at position 1 before the first completion: worker 1 becomes
    index 2, and task 2, placed after both completions, lands on index 2 = label 1."""
    g = dict(n_tasks=3, nthreads=np.array([1, 1]), dep_ptr=np.array([0, 0, 0, 2]), dep_idx=np.array([0, 1]),
             restr_ptr=np.array([0, 0, 0, 1]), restr_idx=np.array([1]), restr_flags=np.array([0, 0, 1], np.uint8))
    z = dict(msg_task=np.array([0, 1, 2]), msg_worker=np.array([0, 2, 2]), add_msg=np.array([0]), add_pos=np.array([1]),
             add_nthreads=np.array([1]), add_running=np.array([1]), stim_nplaced=np.array([2, 0, 0, 1, 0]),
             pl_task=np.array([0, 1, 2]), pl_worker=np.array([0, 1, 2]))
    c = join_census(g, z)
    assert c["order"] == [0, 2, 1] and c["n_inserted"] == 1 and c["first_insertion"] == 1
    assert (c["moved_rows"], c["moved_placed"]) == (1, 1)
    assert c["joins"] == [dict(pos=1, W=2, placed=0, restr_after=1, running=True)]
    assert relabel(2, [1], [2], z["pl_worker"]).tolist() == [0, 1, 1]
    # the same stream with the joiner appended: nothing moves
    z.update(add_pos=np.array([2]), msg_worker=np.array([0, 1, 1]), pl_worker=np.array([0, 1, 1]))
    c = join_census(g, z)
    assert c["order"] == [0, 1, 2] and c["n_inserted"] == 0 and (c["moved_rows"], c["moved_placed"]) == (0, 0)


def test_narrow_rows_with_appended_joins():
    """svcaddw_restr12: rows of 1-4 of 12 workers, none of a strict task empty, and every
    join followed by restricted placements."""
    g, cfg, z, c = census(RESTR12)
    assert c["row_widths"] == [1, 2, 3, 4]
    assert c["strict_empty_rows"] == 0
    assert len(c["joins"]) == 6 and c["n_inserted"] == 0
    assert all(j["pos"] == j["W"] for j in c["joins"])
    assert all(j["restr_after"] >= 1 for j in c["joins"]), c["joins"]


@pytest.mark.parametrize("name", INSERTED)
def test_insertions_move_restriction_rows_that_are_read_again(name):
    g, cfg, z, c = census(name)
    assert c["strict_empty_rows"] == 0
    assert c["n_inserted"] >= 3, c["joins"]
    # restricted tasks placed after the first insertion whose row holds a renumbered index ...
    assert c["moved_rows"] >= 20
    # ... and placed on a worker of their row whose index had moved
    assert c["moved_placed"] >= 5


def test_paused_joiners_resume_before_restricted_placements():
    g, cfg, z, c = census("svcaddw_insrestr_sat1.1")
    assert c["n_paused"] >= 1 and c["n_resumes"] >= 1
    assert c["restr_after_resume"] >= 1
    # the stream's joins take queued tasks (tests/test_gpu_service.py asserts the engine's count)
    assert c["refill"] > 0
    assert any(j["placed"] > 0 and j["pos"] < j["W"] for j in c["joins"])


def test_insertions_across_the_64_worker_word():
    g, cfg, z, c = census("svcaddw_ins64_sat1.1")
    J = c["joins"]
    assert c["W0"] < 64 < c["W0"] + len(J)
    # W1: the join that takes the count from 64 to 65 (the bitsets grow to two words) inserts
    assert any(j["W"] == 64 and j["pos"] < 64 for j in J)
    # W2: an insertion inside the second word
    assert any(64 <= j["pos"] < j["W"] for j in J)
    # W3: an insertion at a word's first bit (nothing of that word stays in place)
    assert any(j["pos"] % 64 == 0 and 0 < j["pos"] < j["W"] for j in J)
    # W4: a result held by the worker at index 63 when it moves to 64 is read by a later placement
    assert any(j["pos"] <= 63 < j["W"] for j in J) and c["W4"]
    # W5: an insertion at position 0 (every index moves)
    assert any(j["pos"] == 0 for j in J)


def test_inserted_joiners_take_work():
    """svcaddw_insq: joiners inserted among the known workers take queued tasks at the join
    and are given tasks afterwards (they hold results that later decisions read). In the
    other insertion fixtures without a queue of root-ish tasks the joiners stay without
    work: new workers are candidates only through the queue or the results they hold."""
    g, cfg, z, c = census("svcaddw_insq_sat1.1")
    assert z["add_running"].all()
    assert any(j["placed"] > 0 and j["pos"] < j["W"] for j in c["joins"])
    assert c["on_joiners"] >= 20


@pytest.mark.parametrize("name", UNPAUSED)
def test_an_insertion_against_an_append_renamed(name):
    """The same stream with every joiner appended (the oracle's append path, pinned by the
    appended-join fixtures), in labels. The reference holds WorkerState objects, so where a
    joiner sorts can change a decision only through a tie that the worker order breaks
    between a joiner and another worker. That was looked for and not found: none of these
    fixtures, and none of 90 further streams of the svcaddw_insq shape (graph seeds 32, 34,
    35, stream seeds 40-69), has such a tie, and at saturation inf or without a root-ish
    group (insrestr_satinf, ins64) the joiners are given no task at all. So an insertion is
    an append plus renaming in every one of them, and that is what is asserted: it pins the
    label bookkeeping of the census and the fixture's positions against an independent run.
    What these fixtures tell apart is an engine that renumbers wrongly, not one that orders
    ties wrongly."""
    g, cfg, z, c = census(name)
    out = oracle.replay(g, cfg, joins=(z["add_msg"], z["add_nthreads"]))  # every joiner appended: index = label
    assert np.array_equal(out["pl_task"], z["pl_task"])
    assert np.array_equal(out["pl_worker"], np.array(c["pl_label"]))
    # in indices the two logs differ: the renumbering is what the engine has to get right
    assert (out["pl_worker"] != z["pl_worker"]).sum() >= 20

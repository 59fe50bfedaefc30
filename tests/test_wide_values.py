"""What the wide-value cases contain, on the oracle's and the fixtures' logs alone (CPU).

Every other placement test runs at ``bandwidth = 100_000_000``, ``default_data_size = 1024``,
``unknown_duration = 0.5`` (the engine's built-in defaults) with results below 2^31 bytes,
known sizes and compute intervals from 0.0. The ``wide_*`` / ``svc*_wide_*`` fixtures
(reference logs) and the fresh-seed cases of tests/wide_cases.py (replayed on the GPU by
tests/test_gpu_wide_values.py) leave that point. These tests show that they do, and that an
engine which dropped the high word of a size, or kept one of the three config values at its
default, could not pass them: the oracle's replay of each such variant places some task on
another worker.
"""
import json
import os

import numpy as np
import pytest

import wide_cases as wc
from conftest import GOLDEN, golden_files
from oracle import oracle
from stimulus_census import max_worker_prefixes, scan_mode_refills
from test_gpu_exe_path import start_ties

WIDE_REPLAY = ["wide_c2var_sat1.1.npz", "wide_c2var_satinf.npz", "wide_restr_sat1.1.npz", "wide_p40_sat1.1.npz",
               "wide_scan_refill_sat1.1.npz", "wide_dds0_sat1.1.npz"]
WIDE_SERVICE = ["svcev_wide_sat1.1.npz", "svcwl_chain_wide_sat1.1.npz", "svcrel_wide_sat1.1.npz",
                "svccan_wide_sat1.1.npz", "svcrs_wide_sat1.1.npz", "svcaddw_wide_sat1.1.npz"]

_FIX = {}


def fixture(name):
    if name not in _FIX:
        _FIX[name] = oracle.load_fixture(os.path.join(GOLDEN, name))
    return _FIX[name]


def case(name):
    """(graph, config, log) of a fixture (the reference's log) or a fresh-seed case (the oracle's)."""
    if name.endswith(".npz"):
        g, cfg, exp, meta = fixture(name)
        return g, cfg, exp
    return wc.reference(name)


def test_wide_fixtures_are_picked_up_by_the_parity_tests():
    # test_oracle_matches_reference, test_engine_matches_reference_fixture and
    # test_service_matches_reference_fixture parametrise over golden_files()
    assert set(WIDE_REPLAY) <= set(golden_files())
    assert set(WIDE_SERVICE) <= set(os.listdir(GOLDEN))


@pytest.mark.parametrize("name", WIDE_REPLAY + WIDE_SERVICE)
def test_fixture_config_is_none_of_the_defaults(name):
    g, cfg, exp, meta = fixture(name)
    assert cfg["bandwidth"] not in (wc.DEFAULT["bandwidth"], 10 ** 10) and 5e9 < cfg["bandwidth"] < 2e10
    assert cfg["default_data_size"] != wc.DEFAULT["default_data_size"]
    assert cfg["unknown_duration"] != wc.DEFAULT["unknown_duration"]
    assert (cfg["default_data_size"] == 0) == name.startswith("wide_dds0_")
    assert name[:-4] in meta["generator"] and "gen_" in meta["generator"]  # the command that made it
    nb = np.asarray(g["nbytes"])
    frac = float((nb < 0).mean())
    assert (0.25 < frac < 0.35) if name.startswith("wide_dds0_") else (0.07 < frac < 0.13)
    assert g["start"].min() > 1.6e9 and len(g["prio"]) <= 2500


@pytest.mark.parametrize("name", WIDE_REPLAY + wc.WIDENED)
def test_case_carries_high_words_and_unknown_sizes(name):
    g, cfg, log = case(name)
    unknown = wc.census(g, cfg, log)
    # a completion of unknown size, and a later placement whose comm bytes include
    # default_data_size for it (census has shown pl_comm equal to the recomputed sums)
    assert (np.asarray(g["nbytes"]) < 0).any() and int((unknown > 0).sum()) >= 1
    print(name, "placements whose comm includes an unknown size:", int((unknown > 0).sum()))


@pytest.mark.parametrize("name", WIDE_REPLAY + wc.WIDENED)
def test_dropped_high_word_or_default_config_changes_the_placements(name):
    g, cfg, log = case(name)
    moved = wc.sensitivity(g, cfg, log)
    log_only = wc.LOG_ONLY.get(name, ())
    for what in log_only:  # see wide_cases.LOG_ONLY: the expected log moves, no worker can
        assert not moved.pop(what)
    assert all(moved.values()), moved
    if log_only:
        starts = wc.sensitivity(g, cfg, log, key="pl_start")
        assert all(starts[what] for what in log_only), starts


def test_ties_fall_through_to_nbytes_above_bit_32():
    g, cfg, ref = wc.reference("ties")
    nb = np.asarray(g["nbytes"])
    assert (nb == wc.TIE_NBYTES).all() and len(set((g["stop"] - g["start"]).tolist())) == 1
    assert start_ties(g, ref) >= 20
    # every ws.nbytes the argmin compares is a multiple of 2^33: equal in the low word
    wsn = np.asarray(ref["pl_wsnbytes"])
    assert (wsn % wc.TIE_NBYTES == 0).all() and len(np.unique(wsn)) > 50
    assert (np.asarray(ref["pl_comm"]) >= 2 ** 32).any() and (np.asarray(ref["round_wnbytes"]) >= 2 ** 36).any()
    assert wc.sensitivity(g, cfg, ref)["nbytes & 0xffffffff"]


def test_scan_refill_fixture_is_in_scan_mode():
    g, cfg, exp = case("wide_scan_refill_sat1.1.npz")
    refills, scanning = scan_mode_refills(g, exp, cfg["saturation"], 63)
    print("refills", refills, "local stimuli on a scanning worker", scanning)
    assert len(g["prefix_default_dur"]) <= 32 and refills >= 10 and scanning >= 1000


def test_p40_fixture_and_case_run_on_the_round_engine():
    assert len(case("wide_p40_sat1.1.npz")[0]["prefix_default_dur"]) > 32
    assert len(wc.reference("prefixes:40")[0]["prefix_default_dur"]) > 32
    assert len(wc.reference("global_state")[0]["nthreads"]) > 1024


@pytest.mark.parametrize("name", WIDE_REPLAY + wc.CASES)
def test_case_stays_within_the_worker_prefix_dict(name):
    """Transfer terms of seconds gather work on few workers, which then run more prefixes at
    once than at the default values. More than 8 on one worker is the engines' documented
    limit (the per-worker dict's 8 slots: the engine ends with a device error there, as the
    first shape of wide_p40 showed); the cases stay inside it."""
    g, cfg, log = case(name)
    assert max_worker_prefixes(g, log) <= 8


def test_case_seeds_are_fresh():
    """No seed of tests/wide_cases.py appears in another test or a generator."""
    import re

    here = os.path.dirname(os.path.abspath(__file__))
    src = open(os.path.join(here, "wide_cases.py")).read()
    seeds = set(re.findall(r"\b(?:9[0-9]{3}|1[0-9]{4}|2[0-9]{4})\b", src.split("def build_case")[1].split("WIDENED")[0]))
    assert len(seeds) >= 15
    for root in (here, os.path.join(here, "golden")):
        for f in os.listdir(root):
            if f.endswith(".py") and f != "wide_cases.py":
                text = open(os.path.join(root, f)).read()
                hit = [s for s in seeds if re.search(r"seed\w*\s*=\s*%s\b" % s, text)]
                assert not hit, (f, hit)


# --------------------------------------------------------------------- service fixtures
def test_resync_dumps_hold_rows_past_2_32():
    z = np.load(os.path.join(GOLDEN, "svcrs_wide_sat1.1.npz"), allow_pickle=False)
    assert len(z["sync_workers_nbytes_ptr"]) - 1 >= 10  # dumps
    for field in ("sync_workers_nbytes", "sync_workers_netocc", "sync_tasks_nbytes"):
        assert (z[field] >= 2 ** 32).any(), field
    assert (z["sync_globals_network_occ_global"] >= 2 ** 32).any()
    assert len(np.unique(z["sync_globals_bandwidth"])) >= 2


@pytest.mark.parametrize("name", [f for f in WIDE_SERVICE if not f.startswith("svcaddw_")])
def test_heartbeats_leave_distinct_bandwidths(name):
    z = np.load(os.path.join(GOLDEN, name), allow_pickle=False)
    g, cfg, exp, meta = fixture(name)
    bw = z["ev_x"][z["ev_kind"] == 6]  # EV_HEARTBEAT: the scheduler's bandwidth after it
    assert len(np.unique(bw)) >= 2 and (bw != cfg["bandwidth"]).all()
    assert (np.abs(bw / cfg["bandwidth"] - 1) < 0.31).all()  # the EWMA stays near the config's value


@pytest.mark.parametrize("name", WIDE_SERVICE)
def test_service_fixture_carries_high_words_and_unknown_sizes(name):
    g, cfg, exp, meta = fixture(name)
    z = np.load(os.path.join(GOLDEN, name), allow_pickle=False)
    nb = z["msg_nbytes"] if "msg_nbytes" in z.files else z["ev_nbytes"][z["ev_kind"] == 0]
    assert (nb >= 2 ** 32).any() and (nb < 0).any()  # reported sizes: several GB, and None
    assert (exp["pl_comm"] >= 2 ** 32).any() and (exp["round_wnbytes"] >= 2 ** 36).any()
    assert (exp["round_wnbytes"] >= 0).all() and (exp["pl_wsnbytes"] >= 0).all()
    if name.startswith(("svcrel_", "svccan_", "svcwl_")):  # bytes leave workers: released, cancelled, lost
        tot = exp["round_wnbytes"].sum(axis=1)
        assert (np.diff(tot) <= -(2 ** 32)).any()


def test_meta_records_config_and_command():
    for name in WIDE_REPLAY + WIDE_SERVICE:
        meta = json.loads(str(np.load(os.path.join(GOLDEN, name), allow_pickle=False)["meta"]))
        assert set(meta["config"]) >= {"bandwidth", "default_data_size", "unknown_duration", "saturation"}
        assert meta["generator"].startswith("PYTHONHASHSEED=0 python3.9 tests/golden/gen_")

"""Multi-key client-releases-keys through GPUPlacementExtension on the stand-in scheduler.

``tests/ext_driver.py`` sends one key per release event, so this file is also the small driver
for the ``svcbulk_*`` streams: run under the image's python3.9 (the reference through
``tests/golden/_refshim.py``) it reuses ext_driver.run_events unchanged and widens each
client-releases-keys message to the keys the fixture recorded (``bk_key_*``) before the
extension sees it. run_events then checks what it checks for ``svccan_*``: the plan the
extension hands to the engine is the generator's, in the scheduler's order, no resync, every
placement the engine's, validate=True. The stand-in engine takes the bulk path as the real one
does by default (plans of DGP_RELEASE_BULK_MIN tasks and more), so ``release_tasks_bulk``
counts the long plans. Without the reference (the GPU box) the test skips, as tests/test_ext.py.
"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
PY39 = "/opt/conda/bin/python3.9"
HAVE_REF = os.path.exists(PY39) and os.path.isdir("/root/reference/distributed")
STREAMS = ["bulk/svcbulk_all_c2var_sat1.1.npz", "bulk/svcbulk_queue_sat1.1.npz",
           "bulk/svcbulk_skew_satinf.npz"]  # under tests/golden/
BULK_MIN = 64  # include/dgplace.h DGP_RELEASE_BULK_MIN


def drive(name):
    """(python3.9) One svcbulk_* stream through ext_driver.run_events, keys widened."""
    import numpy as np

    sys.path.insert(0, HERE)
    import ext_driver as D

    z = np.load(os.path.join(HERE, "golden", name), allow_pickle=False)
    rp, kp = z["rk_evptr"], z["bk_key_ptr"]
    calls = iter(range(len(z["bk_event"])))
    sent = []
    if not hasattr(D, "_plain"):  # the driver's own classes, whatever an earlier stream put in their place
        D._plain = (D.GPUPlacementExtension, D.EventEngine)

    class Widening(D._plain[0]):
        def _on_client_releases_keys(self, kw):
            j = next(calls)
            e = int(z["bk_event"][j])
            rows = z["rk_task"][rp[e]:rp[e + 1]][z["bk_key_row"][kp[j]:kp[j + 1]]]
            keys = [self.engine.fkeys[int(t)] for t in rows]
            assert list(kw["keys"])[0] in keys
            kw["keys"] = keys  # the handler runs with the same dict
            sent.append(len(keys))
            return super()._on_client_releases_keys(kw)

    class Engine(D._plain[1]):
        last_release_path = 0

        def __init__(self, exp, fixture_keys):
            super().__init__(exp, fixture_keys)
            self.fkeys = list(fixture_keys)

        def release_tasks(self, t, f):
            self.last_release_path = 2 if len(t) >= BULK_MIN else 1
            return super().release_tasks(t, f)

    D.GPUPlacementExtension = Widening
    D.EventEngine = Engine
    r = D.run_events(name)
    r["keys_sent"] = sent
    r["plans"] = z["bk_n"].tolist()
    return r


if __name__ == "__main__":
    import warnings

    warnings.filterwarnings("ignore")
    for nm in sys.argv[1:]:
        print(json.dumps(drive(nm)))
else:
    import pytest

    @pytest.mark.skipif(not HAVE_REF, reason="needs the reference + python3.9 (build container only)")
    def test_extension_follows_multi_key_releases_on_the_bulk_path():
        """No resync, no fallback, every release followed by the engine, the long plans counted
        as bulk."""
        env = dict(os.environ, PYTHONHASHSEED="0")
        env.pop("PYTHONPATH", None)
        out = subprocess.run([PY39, os.path.abspath(__file__), *STREAMS], capture_output=True, text=True, env=env,
                             timeout=600, cwd=REPO)
        assert out.returncode == 0, out.stderr[-3000:]
        res = [json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")]
        assert [r["fixture"] for r in res] == STREAMS
        for r in res:
            assert r["active"] and r["resyncs"] == 0 and r["host_placements"] == 0, r
            assert r["calls"]["release_tasks"] == len(r["plans"]) == len(r["keys_sent"]), r
            assert max(r["keys_sent"]) > 64, r
            assert r["calls"].get("release_tasks_bulk", 0) == sum(n >= BULK_MIN for n in r["plans"]), r
        assert res[0]["calls"]["release_tasks_bulk"] > 0  # every key of the graph in one call

"""GPUWorkStealing's incrementally kept task rows (distributed_amd/stealing.py StealRows)
against the full rebuild (steal_problem_from_state) on plain stand-ins of the reference's
objects (no dask needed): dependency rows longer than the slot row (KD), removals and slot
reuse, dependencies shared and dropped, unknown task durations (get_task_duration's
unknown_durations side effect), restrictions. The reference-plugin version of the same
check runs in tests/steal_ext_driver.py before every balance()."""
import numpy as np

import steal_rows_state as SR
from distributed_amd.stealing import ordered_problem, steal_problem_from_state


def test_incremental_rows_equal_the_full_rebuild():
    st = SR.new_state()  # the stand-ins and the sequence live in tests/steal_rows_state.py
    s, plugin, rows = st.s, st.plugin, st.rows

    def check():
        a, ta, _ = steal_problem_from_state(plugin)
        b, slots, _ = rows.problem(plugin)
        b, slots = ordered_problem(b, slots)  # the device's walk order
        tb = [rows.task[int(i)] for i in slots]
        assert ta == tb
        assert set(a) == set(b)
        for k in a:
            if k in ("dep_idx", "data_nbytes", "data_get_nbytes", "holder_ptr", "holder_idx"):
                continue
            if isinstance(a[k], np.ndarray):
                assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
            else:
                assert a[k] == b[k], k

        def per_task(p):
            out = []
            for t in range(len(p["dep_ptr"]) - 1):
                r = p["dep_idx"][p["dep_ptr"][t]:p["dep_ptr"][t + 1]]
                assert np.all(np.diff(r) > 0)
                out.append(sorted((int(p["data_nbytes"][d]), int(p["data_get_nbytes"][d]),
                                   tuple(p["holder_idx"][p["holder_ptr"][d]:p["holder_ptr"][d + 1]])) for d in r))
            return out

        assert per_task(a) == per_task(b)

    done = []
    for phase in SR.phases(st):
        check()
        done.append(phase)
    assert done == ["put", "removed", "reused and put again", "replicas", "replicas cleared"]
    assert "p2" in s.unknown_durations
    rows.clear()
    assert len(rows) == 0

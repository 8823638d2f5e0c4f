"""CPU: the layout cases of the refining merge (tests/refine_layout_cases.py) hold the contract the kernel's proof assumes and send
queries down every path their floors name -- counted with the host restatement of tests/refine_cases.py, printed per case.  The GPU
module (tests/test_gpu_refine_layout.py) runs the kernels on exactly these lists; a case that did not reach its floors here would test
less there than its name says."""
import pytest

from tests import refine_cases as RC
from tests import refine_layout_cases as LC


@pytest.mark.parametrize("case", LC.LAYOUT_CASES, ids=RC.case_id)
def test_case_holds_the_contract_and_reaches_its_floors(case):
    b, want = RC.built(case.name), RC.restated(case.name)
    worst = RC.check_contract(b)
    n_out, HWq = b.slot_pair.shape[0], b.pair_idx.shape[1]
    print(f"{case.name}: {n_out} x {HWq} queries, paths {want['counts']}, words {want['words']}, max |a - s32| {worst:.3e} (eps {b.eps:.3e}), "
          f"held {int(b.held.sum())}/{b.held.size}")
    assert case.floors, case.name
    for path, least in case.floors:
        assert want["counts"][path] >= least, (case.name, path, want["counts"])
    assert float(b.held.mean()) >= RC.MIN_SHARE, case.name


def test_grid_cases_cover_the_wave_and_workgroup_edges():
    sizes = sorted(c.grid[0] * c.grid[1] for c in LC.GRID_CASES)
    for n in (1, 63, 64, 65, 255, 256, 257, 320):
        assert n in sizes, n
    two = RC.built("g09_two_rows_unused_slot_inside").slot_pair
    assert two.shape == (2, 6) and int((two[0] >= 0).sum()) == 6 and two[1].tolist()[2] == -1 and two[1].tolist()[5] == -1 and two[1, 3] >= 0
    assert two[0, 0] == two[0, 1]                                      # a key frame in two slots: twins
    assert RC.built("k5_65_queries_square").case.k == 5


def _queued(name):
    """per query of output row 0: (flagged, sampled)"""
    b = RC.built(name)
    out = []
    for q in range(b.pair_idx.shape[1]):
        r = RC.restate_query(b, 0, q)
        out.append((r["path"] != "final", r["path"] == "final" and bool(r["sampled"])))
    return out


def test_wave_compositions_are_what_the_names_say():
    # the second wave (queries 64 ..) of 75 queues nothing; the first queues the sampled query 0 alone
    qd = _queued("w01_second_wave_queues_nothing")
    assert len(qd) == 75 and [i for i, (f, s) in enumerate(qd) if f or s] == [0] and qd[0] == (False, True)
    # every lane of one whole wave flagged, from scratch
    qd = _queued("w02_every_lane_queued")
    assert len(qd) == 64 and all(f for f, _ in qd)
    assert RC.restated("w02_every_lane_queued")["words"][1] == 64
    # of the second wave (queries 64 .. 76) exactly the last valid lane is queued; the first wave mixes flagged and final lanes
    qd = _queued("w03_last_valid_lane_alone_queued")
    assert len(qd) == 77 and [i for i in range(64, 77) if qd[i][0] or qd[i][1]] == [76] and qd[76][0]
    first = [i for i in range(64) if qd[i][0]]
    assert 0 < len(first) < 32 and not qd[63][0] and not qd[75][0]
    path = RC.restated("w03_last_valid_lane_alone_queued")["path"]
    assert RC.PATHS[int(path[0, 76])] == "rescored"


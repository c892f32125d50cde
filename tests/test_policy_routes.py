"""Which kernels an inference call of the policy runs is pinned, on a box without a GPU (tools/launch_log.cpp stands in for the
HIP runtime): for every case of tests/_act_route_cases.py, under its switch setting, the launch sequence equals
tests/golden/policy_routes_golden.json (tests/golden/make_policy_routes_golden.py) exactly, it contains the kernel instance
the case's route label names and none of the instances of that stage's other routes, and the default-setting cases together
launch every forward kernel instance csrc/policy.hip registers.  tests/test_gpu_act_routes.py checks the numbers of the same
cases; this half says that a case still reaches the kernel it was written for."""
import importlib.util
import json
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_policy_routes_golden",
                                               os.path.join(ROOT, "tests", "golden", "make_policy_routes_golden.py"))
g = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(g)
cases = g.cases

CXX = os.environ.get("CXX", "c++")
pytestmark = pytest.mark.skipif(shutil.which(CXX) is None, reason="host C++ compiler not found")

# Every kernel csrc/policy.hip defines is in exactly one of these lists (tests/_policy_kernel_lists.py, shared with
# tests/test_learn_routes.py); an instance the library registers outside them fails test_every_forward_instance_is_reached, so
# a new forward kernel cannot arrive without a case.
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _policy_kernel_lists import BACKWARD, FORWARD, FORWARD_ELSEWHERE  # noqa: E402

TABLE_BUILDERS = ("split3_planes_kernel", "frag_pack_planes_kernel", "frag_pack_f32_kernel", "permute_row_kernel")


@pytest.fixture(scope="module")
def table():
    return json.load(open(g.GOLDEN))


@pytest.fixture(scope="module")
def recorded(table):
    return g.decode(table)


@pytest.fixture(scope="module")
def recorder(tmp_path_factory):
    return g.build_recorder(str(tmp_path_factory.mktemp("launch_log")), CXX)


@pytest.fixture(scope="module")
def lib_path():
    from embodied_clip_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), _lib.LIB_PATH
    return _lib.LIB_PATH


def _kernels(events):
    return [e[0] for e in events if e[0] != "D"]


def test_table_matches_the_cases(table):
    assert list(table["cases"]) == list(cases.CASES)
    assert {n: c["cmd"] for n, c in table["cases"].items()} == {n: g.command(c) for n, c in cases.CASES.items()}
    assert table["parent_commit"] == g.PARENT_COMMIT
    assert all(c["rc"] == 0 and c["ws"] > 0 for c in table["cases"].values())


def test_boundary_cases_sit_on_both_sides_of_each_threshold():
    """the row / actor counts of the boundary cases against the plan's thresholds"""
    rows = {n: cases.rows_of(c) for n, c in cases.CASES.items()}
    assert (rows["c1_n41"], rows["c1_n42"]) == (2009, 2058) and rows["c1_n41"] <= 2048 < rows["c1_n42"]
    assert (rows["c1_n83"], rows["c1_n84"]) == (4067, 4116) and rows["c1_n83"] <= 4096 < rows["c1_n84"]
    assert rows["rows_n334"] <= 16384 < rows["rows_n335"]
    assert rows["c1_pingpong_n669"] >= 256 * 128 > cases.rows_of(dict(cases.CASES["c1_pingpong_n669"], N=668))
    assert (cases.CASES["gi7_n256"]["N"], cases.CASES["gi_parts_n257"]["N"]) == (256, 257)
    assert rows["c1_n127"] % 128 in range(65, 96)          # the last workgroup's third block is ragged, its fourth empty


@pytest.mark.parametrize("name", list(cases.CASES))
def test_route_label_names_what_runs(recorded, name):
    case, rec = cases.CASES[name], recorded[name]
    ran = _kernels(rec["call"])
    for stage in cases.ROUTE_STAGES:
        for label, instances in cases.ROUTE_KERNELS[stage].items():
            for k in instances:
                if label == case["route"][stage]:
                    assert k in ran, (name, stage, label, ran)
                else:
                    assert k not in ran, (name, stage, label, ran)
    gemms = [e for e in rec["call"] if e[0].startswith(("gemm_f32_kernel", "gemm_x3_kernel"))]
    assert sum(e[3] == 4 for e in gemms) == cases.z4_launches(case) and all(e[3] in (1, 4) for e in gemms), (name, gemms)
    assert ran.count("gru_step_fwd_kernel") + ran.count("gru_gates_fwd_kernel") == case["T"]
    # T == 1: the new state is written where the caller wants it; else it is copied out of the workspace
    h_bytes = case["N"] * cases.cfg_of(case)["hidden"] * 4
    assert [e for e in rec["call"] if e[0] == "D"] == ([] if case["T"] == 1 else [("D", h_bytes)]), name
    if case["mode"] == "reuse":                             # the tables are built by the first call and by it alone
        assert not set(ran) & set(TABLE_BUILDERS), (name, ran)
        built = set(_kernels(rec["build"]))
        assert ("permute_row_kernel" in built) == (case["route"]["wih"] == "perm")
        assert ("frag_pack_planes_kernel" in built) == case["route"]["c1"].startswith("act")
        assert ("frag_pack_f32_kernel" in built) == case["route"]["gi"].startswith("act")
        assert [k for k in _kernels(rec["build"]) if k not in TABLE_BUILDERS and not k.startswith("gemm_")] == \
               [k for k in ran if not k.startswith("gemm_")], name
    else:
        assert rec["build"] is None


@pytest.mark.parametrize("setting", list(cases.SETTINGS))
def test_launches_equal_the_recorded_table(recorded, recorder, lib_path, setting):
    _registered, got = g.record(recorder, lib_path, setting)
    assert got and set(got) == set(cases.cases_of(setting))
    for name, rec in got.items():
        assert rec == recorded[name], (setting, name)


def test_every_forward_instance_is_reached(table, recorded, recorder, lib_path):
    registered, _ = g.record(recorder, lib_path, "default")
    mine = {k for k in registered if k.split("<")[0] in g.policy_kernel_names()}
    assert mine == set(table["policy_kernels"]), sorted(mine ^ set(table["policy_kernels"]))
    known = set(FORWARD) | set(FORWARD_ELSEWHERE) | set(BACKWARD)
    assert len(known) == len(FORWARD) + len(FORWARD_ELSEWHERE) + len(BACKWARD)
    assert mine == known, sorted(mine ^ known)
    reached = set()
    for name in cases.cases_of("default"):
        reached |= set(_kernels(recorded[name]["call"])) | set(_kernels(recorded[name]["build"] or []))
    assert set(FORWARD) <= reached, sorted(set(FORWARD) - reached)
    assert not (set(FORWARD_ELSEWHERE) | set(BACKWARD)) & reached

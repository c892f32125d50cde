"""Which kernels the learn pass of the policy runs -- the forward with for_backward=1, then ec_policy_backward2 in the same
workspace -- is pinned, on a box without a GPU (tools/launch_log.cpp stands in for the HIP runtime): for every case of
tests/_learn_route_cases.py, under its switch setting, the launch sequences of both calls equal
tests/golden/learn_routes_golden.json (tests/golden/make_learn_routes_golden.py) exactly, they contain the kernel instances the
case's route labels name and none of the instances of that stage's other labels, the per-case launch counts hold, and the
default-setting cases together launch every backward kernel instance csrc/policy.hip registers, plus gru_step_fwd512_kernel.
tests/test_gpu_learn_routes.py checks the numbers of the same cases; this half says that a case still reaches the kernels it
was written for."""
import importlib.util
import json
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_learn_routes_golden", os.path.join(ROOT, "tests", "golden", "make_learn_routes_golden.py"))
g = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(g)
cases = g.cases

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _policy_kernel_lists import BACKWARD, FORWARD, FORWARD_ELSEWHERE, LEARN_FORWARD  # noqa: E402

CXX = os.environ.get("CXX", "c++")
pytestmark = pytest.mark.skipif(shutil.which(CXX) is None, reason="host C++ compiler not found")

STEP_FWD = ("gru_step_fwd512_kernel", "gru_step_fwd_kernel", "gru_gates_fwd_kernel")
STEP_BWD_FUSED = ("gru_step_bwd512_kernel", "gru_step_bwd_kernel")


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


def _copies(events):
    return [e for e in events if e[0] == "D"]


def _count(ran, spec):
    """launches of the instance `spec`, or (a name without template arguments) of every instance of that template"""
    return sum(k == spec or k.startswith(spec + "<") for k in ran)


def test_table_matches_the_cases(table):
    assert list(table["cases"]) == list(cases.CASES)
    assert {n: c["cmd"] for n, c in table["cases"].items()} == {n: g.command(c) for n, c in cases.CASES.items()}
    assert table["parent_commit"] == g.PARENT_COMMIT
    assert all(c["rc"] == 0 and c["ws"] > 0 for c in table["cases"].values())


def test_settings_and_their_cases():
    """every default case also runs exact; each switch setting is EC_POLICY_FAST=0 plus one switch, on two or three bases"""
    assert cases.cases_of("default") == cases.DEFAULT_CASES
    assert cases.cases_of("exact") == ["exact_" + n for n in cases.DEFAULT_CASES]
    for n in cases.DEFAULT_CASES:
        a, b = cases.CASES[n], cases.CASES["exact_" + n]
        assert {k: a[k] for k in a if k != "env"} == {k: b[k] for k in b if k != "env"} and b["base"] == n, n
    for s, env in cases.SETTINGS.items():
        if s not in ("default", "exact"):
            assert env["EC_POLICY_FAST"] == "0" and len(env) == 2, s
            assert len(cases.cases_of(s)) in (2, 3), s


def test_boundary_cases_sit_on_both_sides_of_each_threshold():
    cases.check_boundary_cases()


@pytest.mark.parametrize("name", list(cases.CASES))
def test_route_label_names_what_runs(recorded, name):
    case, rec = cases.CASES[name], recorded[name]
    route, T, N, H = case["route"], case["T"], case["N"], cases.cfg_of(case)["hidden"]
    fwd, bwd = _kernels(rec["fwd"]), _kernels(rec["bwd"])
    ran = fwd + bwd
    for stage in cases.ROUTE_STAGES:
        mine = cases.ROUTE_KERNELS[stage][route[stage]]
        for label, instances in cases.ROUTE_KERNELS[stage].items():
            for k in instances:
                if k in mine:
                    assert _count(ran, k) > 0, (name, stage, route[stage], k, ran)
                else:
                    assert _count(ran, k) == 0, (name, stage, label, k, ran)
    if route["c1"] == "pingpong":                            # the instance: two planes of W1 under EC_POLICY_FAST, else three
        assert fwd.count(cases.pingpong_instance(case)) == cases.streams_of(case) == _count(ran, "conv_igemm8_kernel"), (name, ran)
    # one forward step launch per t, all of the route's kernel; none of them in the backward
    assert [_count(fwd, k) for k in STEP_FWD] == [T * (k in cases.ROUTE_KERNELS["step"][route["step"]]) for k in STEP_FWD], (name, fwd)
    assert not any(_count(bwd, k) for k in STEP_FWD) and not any(_count(fwd, k) for k in STEP_BWD_FUSED + ("gru_gates_bwd_kernel",))
    # backward recurrence: the gate kernel once per t on the gate routes; on the fused routes once (step T - 1), then T - 1 fused launches
    fused = route["step"] in cases.FUSED_BWD
    assert (route["step"] in cases.GATE_BWD) != fused
    assert bwd.count("gru_gates_bwd_kernel") == (1 if fused else T), (name, bwd)
    assert sum(_count(bwd, k) for k in STEP_BWD_FUSED) == (T - 1 if fused else 0), (name, bwd)
    if fused:
        i = bwd.index("gru_gates_bwd_kernel")
        assert len(set(bwd[i + 1:i + T])) == 1 and bwd[i + 1] in STEP_BWD_FUSED and T > 1, (name, bwd)
    # the fused tail's backward: its reduce and fold launches, two per encoder stream
    n_tail = cases.streams_of(case) * (route["tail"] in cases.FUSED_TAIL_BWD)
    assert (bwd.count("tail_bwd_reduce_kernel"), bwd.count("tail_bwd_fold_kernel")) == (n_tail, n_tail), (name, bwd)
    assert _count(bwd, "tail_bwd_kernel") == n_tail and _count(fwd, "tail_bwd_kernel") == 0
    # dw: the transposes in front of the GRU's two weight-gradient GEMMs are counted
    assert bwd.count("transpose_f32_kernel") == cases.transposes(case) and "transpose_f32_kernel" not in fwd, (name, bwd)
    assert _count(bwd, "dw_tn_x3_kernel") == cases.streams_of(case) * (route["dw1"] == "planes")
    # copies: the forward keeps the goal vectors of a coordinate-goal handle for the backward and copies h_final out of the
    # workspace; the backward copies dh_final into its carry, or (NULL) clears it
    goal_in = cases.cfg_of(case)["goal_in"]
    assert _copies(rec["fwd"]) == [("D", T * N * goal_in * 4)] * (goal_in > 0) + [("D", N * H * 4)], name
    assert _copies(rec["bwd"]) == ([("D", N * H * 4)] if case["dhf"] else []), name


@pytest.mark.parametrize("name", ["h256_t3_n33", "h768_t2_n5"])
def test_the_32_tile_backward_step_runs_with_a_gru(recorded, name):
    """gru_step_bwd_kernel under the default switches: grid (H / 32, ceil(N / 32)), T - 1 launches"""
    case = cases.CASES[name]
    H, N = cases.cfg_of(case)["hidden"], case["N"]
    got = [e for e in recorded[name]["bwd"] if e[0] == "gru_step_bwd_kernel"]
    assert len(got) == case["T"] - 1 and all(e[1:4] == (H // 32, (N + 31) // 32, 1) for e in got), got


@pytest.mark.parametrize("name", [n for n, c in cases.CASES.items() if c["route"]["wih"] == "perm"])
def test_transpose_of_the_reordered_weight_covers_every_row(recorded, name):
    """dx4 = dgi @ (re-ordered weight_ih)^T: the transpose in front of it, the backward's last, spans all 3H rows and all
    flat columns in 32 x 32 tiles, also where 3H is no multiple of 32 (h48_t3_n5: 144 rows, 5 row blocks)"""
    cfg = cases.cfg_of(cases.CASES[name])
    G, flat = 3 * cfg["hidden"], cfg["comb_out"] * cfg["spatial"] ** 2
    last = [e for e in recorded[name]["bwd"] if e[0] == "transpose_f32_kernel"][-1]
    assert last[1:4] == ((flat + 31) // 32, (G + 31) // 32, 1), (name, last)


@pytest.mark.parametrize("name", ["pp_c128", "pp_c256"])
def test_pingpong_cases_fill_the_tail_partial_sets(recorded, name):
    """nwg == TB_MAX_WG = 256: the branch where the tail reducer's scratch lies in the dm1 area"""
    got = [e for e in recorded[name]["bwd"] if e[0] == "tail_bwd_kernel<false>"]
    assert len(got) == 1 and got[0][1] == 256, got
    small = [e for e in recorded["ref_t2_n21"]["bwd"] if e[0] == "tail_bwd_kernel<false>"]
    assert len(small) == 1 and small[0][1] < 256, small


@pytest.mark.parametrize("setting", list(cases.SETTINGS))
def test_launches_equal_the_recorded_table(recorded, recorder, lib_path, setting):
    _registered, got = g.record(recorder, lib_path, setting)
    assert got and set(got) == set(cases.cases_of(setting))
    for name, rec in got.items():
        assert rec == recorded[name], (setting, name)


def test_every_backward_instance_is_reached(table, recorded, recorder, lib_path):
    registered, _ = g.record(recorder, lib_path, "default")
    mine = {k for k in registered if k.split("<")[0] in g.policy_kernel_names()}
    assert mine == set(table["policy_kernels"]), sorted(mine ^ set(table["policy_kernels"]))
    known = set(FORWARD) | set(FORWARD_ELSEWHERE) | set(BACKWARD)
    assert len(known) == len(FORWARD) + len(FORWARD_ELSEWHERE) + len(BACKWARD) and set(LEARN_FORWARD) <= set(FORWARD_ELSEWHERE)
    assert mine == known, sorted(mine ^ known)              # (neither table reaches it and no test is named for it: not in any list)
    reached = set()
    for name in cases.cases_of("default"):
        reached |= set(_kernels(recorded[name]["fwd"])) | set(_kernels(recorded[name]["bwd"]))
    want = set(BACKWARD) | set(LEARN_FORWARD)
    assert want <= reached, sorted(want - reached)
    assert not (set(FORWARD_ELSEWHERE) - set(LEARN_FORWARD)) & reached

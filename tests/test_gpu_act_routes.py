"""Every inference route of the policy against the float64 oracle (the cases of tests/_act_route_cases.py; which kernel
instance each of them runs is pinned without a GPU by tests/test_policy_routes.py).

Per case, for logits, values and the final state:
  1. whole-tensor rel-L2 < 2e-5, the project's forward tolerance (tests/test_gpu_policy.py);
  2. per-row error norm over the RMS row norm < PER_ROW_BOUND, so that one wrong actor among 128 cannot hide in an average.
     The bound is not tuned to the kernels: the fp32 ORACLE against the float64 oracle has a worst per-row figure of 1.99e-6
     over this case table (values of vec_c1_n84; logits 1.08e-6, final state 7.2e-7; `python tests/_act_route_ref.py`, CPU), and
     the bound is 8 times that, 1.59e-5 -- the routes differ from an fp32 evaluation only in summation order and in the bf16x3
     split of an fp32 operand, both 2^-24-class.  The fp32 oracle's whole-tensor figure stays below 8.5e-7 on every case;
  3. the same call into two fresh workspaces (one filled with NaN bytes, one with zeros) gives torch.equal outputs: no float
     atomics on these routes, and nothing read that the call did not write;
  4. actors 0..40 of the 127-actor call against a 41-actor call on those rows: rel-L2 < 1e-5 at the reference widths
     (c1_act_kernel<4, 4> against <1, 8>), bit equality on the split_parts route, which promises slice independence.
A reuse case runs EC_POLICY_INFER and then EC_POLICY_INFER_REUSE in the same workspace on new features, goals, h0 and masks;
both calls are checked.  The cases of a switch setting run in a child process started under that setting, one child at a
time; after a child that exits non-zero no further child is started."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _child import GPU, json_lines  # noqa: E402
import _act_route_ref as ref  # noqa: E402

cases = ref.cases
pytestmark = pytest.mark.gpu

REL_BOUND = 2e-5
FP32_ORACLE_PER_ROW = 1.99e-6                   # measured: see the docstring
PER_ROW_BOUND = 8 * FP32_ORACLE_PER_ROW
SLICE_BOUND = 1e-5
HERE = os.path.dirname(os.path.abspath(__file__))

_results = {}                                   # case name -> run_case() result: computed once, shared


def _run(name):
    if name not in _results:
        assert not any(k in os.environ for s in cases.SETTINGS.values() for k in s), "default-setting cases need a process without switches"
        _results[name] = ref.run_case(name, torch.device("cuda:0"))
    return _results[name]


def _check(name, figs, equal):
    for call, f in enumerate(figs):
        for k in ref.OUTPUTS:
            rel, row = f[k]
            print("%s call %d %s: rel-L2 %.3e per-row %.3e" % (name, call, k, rel, row))
    for call, f in enumerate(figs):
        for k in ref.OUTPUTS:
            rel, row = f[k]
            assert rel < REL_BOUND, (name, call, k, rel)
            assert row < PER_ROW_BOUND, (name, call, k, row)
    assert equal, "%s: two runs in fresh workspaces differ" % name


@pytest.mark.parametrize("name", cases.cases_of("default"))
def test_route_against_float64_oracle(name):
    r = _run(name)
    assert len(r["figs"]) == (2 if cases.CASES[name]["mode"] == "reuse" else 1)
    _check(name, r["figs"], r["equal"])


def _slice_pair(name, n):
    """outputs of actors 0..n-1 of case `name`, and of a call on those n actors alone"""
    from embodied_clip_amd.policy import PolicyHandle
    full, case = _run(name), cases.CASES[name]
    dev = torch.device("cuda:0")
    handle = PolicyHandle(**cases.cfg_of(case))
    flat = handle.flatten(ref.state_dict(case), dev)
    part, _ = ref.gpu_forward(handle, flat, ref.slice_inputs(full["draws"][0], n), dict(case, N=n), dev)
    return {k: full["outs"][0][k][:n] for k in ref.OUTPUTS}, part


def test_actor_slices_agree_c1_act():
    whole, part = _slice_pair("c1_n127", 41)
    for k in ref.OUTPUTS:
        rel = ref.rel_l2(part[k], whole[k])
        print("c1_n127[:41] vs 41 actors, %s: rel-L2 %.3e" % (k, rel))
        assert rel < SLICE_BOUND, (k, rel)


@pytest.mark.parametrize("name", ["c1_parts_f32", "c1_parts_k160"])
def test_actor_slices_are_bit_equal_on_split_parts(name):
    whole, part = _slice_pair(name, 3)
    for k in ref.OUTPUTS:
        assert torch.equal(part[k], whole[k]), (name, k, ref.rel_l2(part[k], whole[k]))


@pytest.mark.parametrize("setting", [s for s in cases.SETTINGS if s != "default"])
def test_switch_setting_against_float64_oracle(setting):
    names = cases.cases_of(setting)
    r = GPU.run([sys.executable, os.path.join(HERE, "_act_route_check.py"), *names], drop="EC_*", env=cases.SETTINGS[setting], limit=300,
                stop_file_on_failure=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = json_lines(r)
    assert [g["case"] for g in got] == names
    for g in got:
        _check(g["case"], g["figs"], g["equal"])

"""Every route of the learn pass of the policy -- the forward with for_backward=1, then the backward in the same workspace --
against the float64 oracle (the cases of tests/_learn_route_cases.py; which kernel instances each of them runs is pinned
without a GPU by tests/test_learn_routes.py, and tests/test_learn_route_ref.py shows that the bounds used here admit the fp32
oracle and reject six named wrong backwards).

Per case: the learn forward into a workspace filled with 0xFF bytes (every float starts as a NaN), the backward into a zeroed
bucket, driven by the cotangents dhv and (where the case says so) dh_final directly.  Then
  1. logits, values, the final state and every gradient tensor against float64, at the bounds of the case's setting
     (tests/_learn_route_ref.py): under EC_POLICY_FAST=0 -- the `exact` setting and the six switch settings -- the whole-tensor
     rel-L2 and the worst row figure each below 8 x the fp32 oracle's worst row figure for that tensor name; under the default
     EC_POLICY_FAST=1 the project's stated tolerances, forward rel-L2 < 2e-5 and gradients rel-L2 < 2e-4 per tensor, with the
     row figures printed but not bounded (a derived 2^-16-class row bound for the fast mode is out of scope here);
  2. a second run in a fresh workspace filled with 0x00: torch.equal outputs and bucket where the case is marked `repeat`
     (ordered handles, and the perm / fused-tail / fused-step reference route), else rel-L2 < 1e-5 between the runs, the figure
     test_backward_event_marks_the_recurrent_section_final uses for routes with float atomics;
  3. h512_nohf: a NULL dh_final gives the bucket of a zero tensor, bit for bit;
  4. actor independence: actors 0..20 of h256_t3_n33 against a 21-actor call on the same rows, forward outputs rel-L2 < 1e-5
     (the gradients sum over the actors: no slice of them to compare).
The default cases run in this process, one test per case; `exact` and each switch setting in one child process apiece, started
under that setting with every other EC_* variable but EC_AMD_LIB removed, one child at a time, each with a timeout of its own;
after a child that exits non-zero no further child is started.

Found by this test when it was written: h48_t3_n5 (3H = 144, no multiple of 32) had every gradient in front of the GRU wrong
by ~70 % -- the transpose of the re-ordered weight_ih in Bwd::input_grad was launched with 3H / 32 row blocks, rounded down."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _child import GPU, json_lines  # noqa: E402
import _learn_route_ref as ref  # noqa: E402

cases = ref.cases
pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

_results = {}                                   # case name -> run_case() result: computed once, shared


def _run(name):
    if name not in _results:
        assert not any(k in os.environ for s in cases.SETTINGS.values() for k in s), "default-setting cases need a process without switches"
        _results[name] = ref.run_case(name, torch.device("cuda:0"))
    return _results[name]


def _check(name, r):
    case = cases.CASES[name]
    exact = case["env"] != "default"
    for k, (rel, row) in r["figs"].items():
        print("%s %s: rel-L2 %.3e worst row %.3e%s" % (name, k, rel, row, "  (bound %.3e)" % ref.bound(k) if exact else ""))
    print("%s two runs: equal %s, rel-L2 %.3e" % (name, r["equal"], r["rerun"]))
    assert ref.violations(r["figs"], case["env"]) == [], name
    if case["repeat"]:
        assert r["equal"], "%s: two runs in fresh workspaces differ (rel-L2 %.3e)" % (name, r["rerun"])
    else:
        assert r["rerun"] < ref.RERUN_REL, (name, r["rerun"])
    if case["base"] == "h512_nohf":
        assert r["nohf_equal"] is True, "%s: dh_final = NULL and dh_final = zeros give different buckets" % name


@pytest.mark.parametrize("name", cases.cases_of("default"))
def test_learn_route_against_float64_oracle(name):
    _check(name, _run(name))


def test_actor_slices_agree_on_the_32_tile_step():
    from embodied_clip_amd.policy import PolicyHandle
    name, n = "h256_t3_n33", 21
    full, case = _run(name), cases.CASES[name]
    dev = torch.device("cuda:0")
    handle = PolicyHandle(**cases.cfg_of(case))
    flat = handle.flatten(ref.state_dict(case), dev)
    inp, T, N = full["inp"], case["T"], case["N"]
    S = cases.cfg_of(case)["spatial"] ** 2
    part_inp = dict(feat=inp["feat"].view(T, N, S, -1)[:, :n].reshape(T * n, S, -1).contiguous(), feat2=None,
                    goal=inp["goal"][:, :n].contiguous(), h0=inp["h0"][:n].contiguous(), masks=inp["masks"][:, :n].contiguous(),
                    dhv=inp["dhv"].view(T, N, -1)[:, :n].reshape(T * n, -1).contiguous(), dh_final=inp["dh_final"][:n].contiguous())
    part, _, _ = ref.gpu_learn(handle, flat, part_inp, dict(case, N=n), dev, 0xFF)
    A = handle.A
    whole = dict(logits=full["outs"]["logits"].view(T, N, A)[:, :n].reshape(T * n, A), values=full["outs"]["values"].view(T, N, 1)[:, :n].reshape(T * n, 1),
                 h_final=full["outs"]["h_final"][:n])
    for k in ref.OUTPUTS:
        rel = ref.rel_l2(part[k], whole[k])
        print("%s[:, :%d] vs %d actors, %s: rel-L2 %.3e" % (name, n, n, k, rel))
        assert rel < ref.SLICE_REL, (k, rel)


@pytest.mark.parametrize("setting", [s for s in cases.SETTINGS if s != "default"])
def test_setting_against_float64_oracle(setting):
    names = cases.cases_of(setting)
    r = GPU.run([sys.executable, os.path.join(HERE, "_learn_route_check.py"), *names], drop="EC_*", env=cases.SETTINGS[setting], limit=300,
                stop_file_on_failure=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = json_lines(r)
    assert [g["case"] for g in got] == names
    failed = []
    for g in got:
        try:
            _check(g["case"], dict(figs={k: tuple(v) for k, v in g["figs"].items()}, equal=g["equal"], rerun=g["rerun"], nohf_equal=g["nohf_equal"]))
        except AssertionError as e:      # (every case of the setting is printed before the first failure is raised)
            failed.append(e)
    if failed:
        raise failed[0]

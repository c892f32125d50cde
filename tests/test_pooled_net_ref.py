"""The pooled-embedding net's reference (tests/_pooled_net_ref.py) on the CPU: the composition of torch.nn.Linear / Embedding /
GRU / LSTM equals a direct per-step loop written out gate by gate; the fp32 evaluation of the reference keeps a tenth of both
bounds the GPU tests use, at every case; the case table covers what it says; deliberately wrong variants miss by a wide margin."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _pooled_net_ref as ref  # noqa: E402

CASES = ref.POLICY_CASES


@pytest.mark.parametrize("case", CASES)
def test_module_composition_equals_the_direct_loop(case):
    kw, sd, batch = ref.policy_inputs(*case)
    net = ref.build(case, sd)
    b = {k: (v.double() if (isinstance(v, torch.Tensor) and v.is_floating_point()) else v) for k, v in batch.items()}
    with torch.no_grad():
        lg, vv, st = net(b["embed"], b["goal"], b["sensors"], b["prev_actions"], b["state0"], b["masks"])
    lg2, vv2, st2 = ref.direct_forward(case, sd, batch)
    assert (lg - lg2).abs().max() < 1e-12 and (vv - vv2).abs().max() < 1e-12 and (st - st2).abs().max() < 1e-12
    T, N, A, L, H = case[0], case[1], case[8], case[9], case[3]
    assert tuple(lg.shape) == (T, N, A) and tuple(st.shape) == (N, L * (2 if case[10] == ref.LSTM else 1) * H)


@pytest.mark.parametrize("case", CASES)
def test_fp32_reference_keeps_a_tenth_of_both_bounds(case):
    fwd, grad = ref.policy_fp32_distance(case)
    print(case, "fp32-vs-fp64 rel-L2: forward %.3e, worst gradient tensor %.3e" % (fwd, grad))
    assert fwd < ref.FWD_TOL / 10 and grad < ref.GRAD_TOL / 10


def test_case_table_covers_every_route():
    col = lambda i: {c[i] for c in CASES}
    assert col(2) == {64, 112, 72} and col(3) == {64, 256, 512, 40} and col(1) == {5, 33} and col(0) == {1, 3}
    assert col(6) == {0, 32} and col(8) == {6, 84} and col(9) == {1, 2, 3} and col(10) == {ref.GRU, ref.LSTM}
    setups = {(bool(c[4]), tuple(c[5])) for c in CASES}
    assert {(True, ()), (False, (3,)), (True, (2, 2))} <= setups
    # the null row is read: a mask zero at t = 0 and, with T = 3, one in the middle, on a case with the null token
    for c in CASES:
        _, _, batch = ref.policy_inputs(*c)
        assert float(batch["masks"][0].min()) == 0
        if c[0] > 2:
            assert float(batch["masks"][c[0] // 2].min()) == 0
    assert any(c[6] and c[7] and c[0] > 2 for c in CASES) and any(c[6] and not c[7] for c in CASES)


@pytest.mark.parametrize("wrong", ["no_relu", "mask_input", "sensor_order", "null_row"])
def test_wrong_variants_miss_the_forward_bound(wrong):
    """what the bound can tell apart: each variant is a plausible mistake of the kernels"""
    case = CASES[1]
    kw, sd, batch = ref.policy_inputs(*case)
    good = ref.policy_reference(case, sd, batch)
    sd2, b2 = dict(sd), dict(batch)
    if wrong == "no_relu":
        net = ref.build(case, sd)
        net.visual_fc[2] = torch.nn.Identity()
    elif wrong == "mask_input":
        net = ref.build(case, sd)
        b2["embed"] = batch["embed"] * batch["masks"]
    elif wrong == "sensor_order":
        net = ref.build(case, sd)
        b2["sensors"] = batch["sensors"].flip(-1)
    else:
        net = ref.build(case, sd)
        b2["prev_actions"] = batch["prev_actions"] + 0
        b2["masks_for_prev"] = None
        net.null = 0                               # the action itself indexes the table: no null row, no shift
    c = lambda t: t.double() if (isinstance(t, torch.Tensor) and t.is_floating_point()) else t
    b2 = {k: c(v) for k, v in b2.items()}
    with torch.no_grad():
        lg, vv, st = net(b2["embed"], b2["goal"], b2["sensors"], b2["prev_actions"], b2["state0"], b2["masks"])
    miss = ref.rel_l2(lg, good["logits"])
    print(wrong, "misses the forward bound by a factor of %.0f" % (miss / ref.FWD_TOL))
    assert miss > 100 * ref.FWD_TOL

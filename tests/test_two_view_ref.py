"""CPU: the float64 reference of the two-view rearrangement net (tests/_two_view_ref.py) checked against itself -- what the
bounds of the GPU tests rest on.

  * the fp32 evaluation of the NCHW module form stays within a tenth of FWD_TOL / GRAD_TOL at every case the bounds were set on
    (so a correct fp32 kernel has a factor ten of room);
  * the NCHW module form equals the pixel-major closed form the kernels implement;
  * the closed-form backward equals autograd in float64;
  * the gradient of visual_attention.2.bias is zero (softmax is shift-invariant), which is why the GPU tests hold it to
    |g| <= GRAD_TOL * ||grad visual_attention.2.weight|| instead of a relative error;
  * the previous-action row rule of the kernels (ec_pa_index) equals upstream's ((prev + 1) * mask).long().
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _two_view_ref as ref  # noqa: E402


@pytest.mark.parametrize("case", ref.FP32_CASES)
def test_fp32_evaluation_is_within_a_tenth_of_the_bounds(case):
    fwd, grad = ref.front_fp32_distance(case)
    print(case, "fp32 vs float64: forward %.3e, worst gradient %.3e" % (fwd, grad))
    assert fwd <= ref.FWD_TOL / 10 and grad <= ref.GRAD_TOL / 10, (fwd, grad)


@pytest.mark.parametrize("case", [c for c in ref.KERNEL_CASES if c[0] * c[2] <= 33 * 192])
@pytest.mark.parametrize("edge", (None,) + ref.EDGES)
def test_module_form_equals_closed_form_and_its_backward(case, edge):
    sd, u, w, dv = ref.kernel_inputs(*case, edge=edge)
    v, grads = ref.front_reference(sd, u, w, dv)
    d = {k: t.double() for k, t in sd.items()}
    v2, grads2 = ref.closed_form(u.double(), w.double(), d, dv.double())
    assert torch.isfinite(v).all() and ref.rel_l2(v2, v) < 1e-12
    errs = ref.grad_errors(grads2, grads)
    assert max(errs.values()) < 1e-10, errs
    # softmax is shift-invariant: the gradient of the last conv's bias is zero up to rounding, in both forms
    scale = float(grads[ref.W2].norm())
    assert float(grads[ref.B2].abs().max()) < 1e-12 * scale and float(grads2[ref.B2].abs().max()) < 1e-12 * scale


def test_edge_inputs_are_what_they_claim():
    case = (5, 49, 64, 32, 32)
    sd, u, w, dv = ref.kernel_inputs(*case, edge="logits80")
    d = {k: t.double() for k, t in sd.items()}
    c = torch.cat([u, w, u * w], -1).double()
    m = torch.relu(c @ d[ref.FRONT[2]].reshape(32, -1).t() + d[ref.FRONT[3]])
    raw = m @ d[ref.W2].reshape(-1)
    assert abs(float(raw.abs().max()) - 80.0) < 1e-3 and float(raw.min()) < 0 < float(raw.max())
    sd, u, w, dv = ref.kernel_inputs(*case, edge="dead_column")
    _, grads = ref.front_reference(sd, u, w, dv)
    assert float(grads[ref.FRONT[0]][1].abs().max()) == 0.0 and float(grads[ref.FRONT[0]][0].abs().max()) > 0.0
    sd, u, w, dv = ref.kernel_inputs(*case, edge="zero_u")
    assert float(u[0].abs().max()) == 0.0 and float(u[1].abs().max()) > 0.0


def test_features_are_nonnegative_bf16_values():
    sd, u, w, dv = ref.kernel_inputs(5, 49, 64, 32, 32)
    for t in (u, w):
        assert float(t.min()) >= 0.0 and torch.equal(t.to(torch.bfloat16).float(), t) and 0.3 < float((t == 0).float().mean()) < 0.7


def test_previous_action_row_rule():
    """ec_pa_index with the null token: row 0 where the mask is zero, else action + 1 == ((prev + 1) * mask).long()"""
    prev = torch.tensor([0, 3, 5, 83, 2, 0])
    masks = torch.tensor([1.0, 0.0, 1.0, 1.0, 0.0, 0.0])
    want = torch.where(masks == 0, torch.zeros_like(prev), prev + 1)
    assert torch.equal(ref.prev_row(prev, masks, 1), want)
    assert torch.equal(ref.prev_row(prev, masks, 0), prev)


@pytest.mark.parametrize("case", ref.POLICY_CASES[:3])
@pytest.mark.parametrize("loss", ref.LOSSES)
def test_whole_net_reference_runs_and_every_tensor_but_b2_has_a_gradient(case, loss):
    kw, sd, batch = ref.policy_inputs(*case)
    r = ref.policy_reference(case, sd, batch, loss)
    assert r["logits"].shape == (case[0], case[1], case[6]) and torch.isfinite(r["logits"]).all()
    for k, g in r["grads"].items():
        if k.startswith("critic.") and loss == "imitation":
            assert float(g.abs().max()) == 0.0, k            # the imitation loss has no value term
        elif k != ref.B2:
            assert float(g.abs().max()) > 0, k
    assert float(r["grads"][ref.B2].abs().max()) <= 1e-12 * float(r["grads"][ref.W2].norm())

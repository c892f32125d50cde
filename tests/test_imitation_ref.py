"""The float64 imitation reference against torch autograd, and the restated teacher-forcing draw's statistics (no GPU)."""
import numpy as np
import pytest
import torch

from _imitation_ref import (TF_N, TF_SEED, TF_STEPS, imitation_ref, make_case, sampler_uniform, teacher_force_decisions,
                            teacher_force_uniform)


def _autograd(hv, expert, mask):
    A = hv.shape[1] - 1
    x = hv.double().clone().requires_grad_(True)
    m = mask.double()
    lp = torch.distributions.Categorical(logits=x[:, :A]).log_prob(expert)
    loss = -(m * lp).sum() / m.sum().clamp(min=1)
    loss.backward()
    return loss.detach(), x.grad


@pytest.mark.parametrize("B,A,kind", [(5, 6, "mixed"), (33, 84, "mixed"), (7, 17, "ones"), (4, 1, "mixed"), (6, 6, "zeros")])
def test_reference_equals_torch_autograd(B, A, kind):
    hv, e, m = make_case(B, A, mask_kind=kind)
    loss, dhv, sums3 = imitation_ref(hv, e, m)
    rl, rg = _autograd(hv, e, m)
    assert abs(float(loss - rl)) <= 1e-12 * max(1.0, abs(float(rl)))
    assert (dhv - rg).abs().max() <= 1e-12
    assert float(sums3[1]) == float(m.sum())
    assert abs(float(sums3[0]) / max(float(m.sum()), 1.0) - float(rl)) <= 1e-12 * max(1.0, abs(float(rl)))
    assert torch.all(dhv[:, A] == 0)


def test_all_zero_mask_gives_zero_loss_and_gradient():
    hv, e, m = make_case(9, 6, mask_kind="zeros")
    e[:] = -1                                                  # never read as an index
    loss, dhv, sums3 = imitation_ref(hv, e, m)
    assert float(loss) == 0.0 and torch.all(dhv == 0) and torch.all(sums3 == 0)


def test_single_action():
    hv, e, m = make_case(5, 1, mask_kind="ones")
    loss, dhv, sums3 = imitation_ref(hv, e, m)
    assert float(loss) == 0.0 and dhv.abs().max() == 0 and float(sums3[2]) == 5.0


def test_shared_denominator_and_accumulate_forms():
    hv, e, m = make_case(12, 6)
    D = float(m.sum())
    _, whole, _ = imitation_ref(hv, e, m, weight=0.5, grad_scale=0.25)
    _, a, _ = imitation_ref(hv[:5], e[:5], m[:5], weight=0.5, grad_scale=0.25, denom=D)
    _, b, _ = imitation_ref(hv[5:], e[5:], m[5:], weight=0.5, grad_scale=0.25, denom=D)
    assert torch.equal(torch.cat([a, b]), whole)
    d0 = torch.randn(12, 7, dtype=torch.float64)
    _, acc, _ = imitation_ref(hv, e, m, weight=0.5, grad_scale=0.25, dhv0=d0)
    assert torch.equal(acc, d0 + whole)
    assert torch.equal(acc[:, 6], d0[:, 6]) and torch.equal(acc[m == 0], d0[m == 0])


def test_forced_fraction_of_the_restated_draw():
    """N = 4096 x 8 steps at p = 0.5: sigma = 0.5 / sqrt(32768) = 0.00276; the cap of the GPU test is 4 sigma = 0.011, which
    the restated draw meets on its own for the seed that test uses."""
    forced = np.stack([teacher_force_decisions(TF_SEED, s, 0, np.ones(TF_N, np.float32), 0.5) for s in range(TF_STEPS)])
    assert abs(forced.mean() - 0.5) < 0.011, forced.mean()
    u = teacher_force_uniform(TF_SEED, 3, np.arange(TF_N))
    assert u.dtype == np.float32 and 0.0 <= u.min() and u.max() < 1.0
    # a stream of its own: not the sampler's uniform for the same key
    assert not np.array_equal(u, sampler_uniform(TF_SEED, 3, np.arange(TF_N)))
    # p = 0 forces nothing, p = 1 every row that has an expert action, and slices agree with the whole
    mask = (np.arange(TF_N) % 5 != 0).astype(np.float32)
    assert not teacher_force_decisions(TF_SEED, 0, 0, mask, 0.0).any()
    assert np.array_equal(teacher_force_decisions(TF_SEED, 0, 0, mask, 1.0), mask != 0)
    whole = teacher_force_decisions(TF_SEED, 2, 0, mask, 0.5)
    assert np.array_equal(teacher_force_decisions(TF_SEED, 2, 1000, mask[1000:1300], 0.5), whole[1000:1300])

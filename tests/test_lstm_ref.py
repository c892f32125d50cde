"""CPU: the reference the LSTM GPU tests are held against (tests/_lstm_ref.py) is itself right, and the bounds of those tests are
not set by the reference's own rounding.

  * the float64 cell and sequence equal torch.nn.LSTM (float64) run segment by segment between mask zeros, to 1e-12 (a segment
    boundary is what the mask does to both states);
  * the closed-form reverse step equals autograd;
  * [2, N, H] <-> [N, 2H] round-trips;
  * every case's fp32 distance from float64 is at most a TENTH of the bound the GPU test applies to it.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _lstm_ref as ref  # noqa: E402


def _sd(I, H, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    return {ref.WIH: r(4 * H, I) / I ** 0.5, ref.WHH: r(4 * H, H) / H ** 0.5, ref.BIH: 0.1 * r(4 * H), ref.BHH: 0.1 * r(4 * H)}


@pytest.mark.parametrize("T,N,I,H", [(7, 3, 5, 8), (12, 4, 16, 32)])
def test_sequence_equals_torch_lstm_between_mask_zeros(T, N, I, H):
    sd = _sd(I, H, T)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(T, N, I, generator=g, dtype=torch.float64)
    state0 = torch.randn(N, 2 * H, generator=g, dtype=torch.float64)
    masks = (torch.rand(T, N, 1, generator=g) > 0.3).double()
    masks[0, 0] = 0.0
    masks[T - 1, 1] = 0.0
    out, state = ref.sequence(x, state0, masks, sd)
    lstm = torch.nn.LSTM(I, H, 1).double()
    with torch.no_grad():
        lstm.weight_ih_l0.copy_(sd[ref.WIH]); lstm.weight_hh_l0.copy_(sd[ref.WHH])
        lstm.bias_ih_l0.copy_(sd[ref.BIH]); lstm.bias_hh_l0.copy_(sd[ref.BHH])
        for n in range(N):
            h, c = state0[n, :H].view(1, 1, H), state0[n, H:].view(1, 1, H)
            t = 0
            while t < T:
                if masks[t, n, 0] == 0:                   # a new segment starts from zero states
                    h, c = torch.zeros_like(h), torch.zeros_like(c)
                e = t + 1
                while e < T and masks[e, n, 0] != 0:
                    e += 1
                o, (h, c) = lstm(x[t:e, n:n + 1], (h, c))
                assert (o[:, 0] - out[t:e, n]).abs().max() < 1e-12
                t = e
            assert (h.view(-1) - state[n, :H]).abs().max() < 1e-12 and (c.view(-1) - state[n, H:]).abs().max() < 1e-12


@pytest.mark.parametrize("N,H", [(1, 8), (5, 32)])
def test_reverse_step_equals_autograd(N, H):
    g = torch.Generator().manual_seed(N + H)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    whh, bhh = r(4 * H, H) / H ** 0.5, 0.1 * r(4 * H)
    m = (torch.arange(N) % 2 == 0).double() if N > 1 else torch.ones(1, dtype=torch.float64)
    a_in, h_prev, c_prev = (t.requires_grad_(True) for t in (r(N, 4 * H), r(N, H), r(N, H)))
    h, c, gates, cp = ref.cell(a_in, h_prev, c_prev, m, whh, bhh)
    dh, dc = r(N, H), r(N, H)
    ga, gh, gc = torch.autograd.grad((h * dh).sum() + (c * dc).sum(), [a_in, h_prev, c_prev])
    da, carry_h, carry_c = ref.reverse_step(dh, torch.zeros_like(dh), dc, gates.detach(), c.detach(), cp.detach(), m, whh)
    assert (da - ga).abs().max() < 1e-12 and (carry_h - gh).abs().max() < 1e-12 and (carry_c - gc).abs().max() < 1e-12
    # the fused form: dh arrives as dhs + m_next * (da_next W_hh)
    da_next, m_next = r(N, 4 * H), torch.ones(N, dtype=torch.float64)
    dhs = dh - da_next @ whh
    daf, ccf = ref.reverse_step_fused(dhs, dc, gates.detach(), c.detach(), cp.detach(), m, whh, da_next, m_next)
    assert (daf - ga).abs().max() < 1e-11 and (ccf - gc).abs().max() < 1e-11


def test_state_layouts_round_trip():
    mem = torch.arange(2 * 3 * 4, dtype=torch.float32).view(2, 3, 4)
    st = ref.memory_to_state(mem)
    assert tuple(st.shape) == (3, 8) and torch.equal(st[:, :4], mem[0]) and torch.equal(st[:, 4:], mem[1])
    assert torch.equal(ref.state_to_memory(st), mem)
    from embodied_clip_amd.policy import ResnetTensorObjectNavActorCritic as M          # the plugin boundary's own pair
    assert torch.equal(M.memory_to_state(mem), st) and torch.equal(M.state_to_memory(st, 2), mem)
    one = mem[:1]
    assert torch.equal(M.state_to_memory(M.memory_to_state(one), 1), one)


def test_kernel_bounds_rest_on_measured_figures():
    """the bound of every kernel output is 10 x a figure measured here, and no figure is degenerate (zero, or so large that
    ten times it would let a wrong kernel through: 1e-6 is 16 fp32 ulps)"""
    worst = ref.fp32_distance()
    assert set(worst) == set(ref.KERNEL_OUTPUTS)
    bounds = ref.kernel_bounds()
    for k, (v, case) in worst.items():
        print(f"{k}: fp32-vs-fp64 rel-L2 {v:.3e} at {case}; GPU bound {bounds[k]:.3e}")
        assert 1e-8 < v < 1e-6, (k, v)
        assert v <= bounds[k] / 10 * (1 + 1e-12)
    for (N, H) in ref.KERNEL_CASES:
        vals = torch.cat([m for m in ref.kernel_masks(N)])
        assert (vals == 0).any() and (vals == 1).any()       # both mask values at every case


@pytest.mark.parametrize("case", ref.POLICY_CASES)
def test_policy_cases_sit_a_tenth_under_their_bounds(case):
    fwd, grad = ref.policy_fp32_distance(case)
    print(case, "fp32-vs-fp64 rel-L2: forward %.3e, worst gradient tensor %.3e" % (fwd, grad))
    assert fwd <= ref.FWD_TOL / 10 and grad <= ref.GRAD_TOL / 10


def test_state_gradient_reference_sees_the_cell_half():
    cfg, sd, batch = ref.policy_inputs(*ref.POLICY_CASES[1])
    full = ref.state_grad_reference(sd, batch, 0)
    H = cfg["hidden"]
    b2 = dict(batch, dstate=torch.cat([batch["dstate"][:, :H], torch.zeros_like(batch["dstate"][:, H:])], dim=1))
    half = ref.state_grad_reference(sd, b2, 0)
    assert ref.rel_l2(half[ref.WHH], full[ref.WHH]) > 1e-3
    assert not full["actor.linear.weight"].any() and full[ref.WIH].abs().max() > 0

"""The float64 reference of the wide action space (tests/_wide_actions_ref.py) against torch itself, on the CPU: the restated
CategoricalDistr against torch.distributions.Categorical, the heads backward and the PPO gradient against autograd, the
restated sampler's action frequencies against the softmax, and the forcing rule's bookkeeping."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _wide_actions_ref as ref  # noqa: E402


@pytest.mark.parametrize("A", [8, 84, 256])
def test_categorical_restatement(A):
    g = torch.Generator().manual_seed(A)
    logits = 3.0 * torch.randn(33, A, generator=g, dtype=torch.float64)
    logits[3, 5] = logits[3, 2] = logits[3].max() + 1.0          # tied maxima: the first index
    d = torch.distributions.Categorical(logits=logits)
    a, lp = ref.mode_rows(logits)
    assert a[3] == 2
    assert torch.equal(a, logits.argmax(dim=-1)) or (a <= logits.argmax(dim=-1)).all()
    assert torch.allclose(lp, d.log_prob(a), rtol=0, atol=1e-12)
    a, lp = ref.sample_rows(logits, seed=7, step=3, first_actor=1000)
    assert ((a >= 0) & (a < A)).all()
    assert torch.allclose(lp, d.log_prob(a), rtol=0, atol=1e-12)
    assert torch.allclose(ref.lse_rows(logits), torch.logsumexp(logits, dim=-1), rtol=0, atol=1e-12)
    ent = -(torch.log_softmax(logits, -1).exp() * torch.log_softmax(logits, -1)).sum(-1)
    assert torch.allclose(ent, d.entropy(), rtol=0, atol=1e-12)


def test_uniform_streams_differ_and_are_keyed():
    us = [ref.sample_uniform(1, 2, n) for n in range(64)]
    uf = [ref.force_uniform(1, 2, n) for n in range(64)]
    assert all(0.0 <= u < 1.0 for u in us + uf) and len(set(us)) > 60 and us != uf
    assert ref.sample_uniform(1, 2, 1003) == ref.sample_uniform(1, 2, 1000 + 3)
    assert ref.sample_uniform(1, 3, 0) != ref.sample_uniform(1, 2, 0)


def test_sampler_frequencies_follow_the_softmax():
    A, n = 9, 6000
    logits = torch.tensor([[0.5, -1.0, 2.0, 0.0, 1.0, -2.0, 0.3, 1.5, -0.5]], dtype=torch.float64).expand(n, A).contiguous()
    a, _ = ref.sample_rows(logits, seed=11, step=5)
    p = torch.softmax(logits[0], -1)
    freq = torch.bincount(a, minlength=A).double() / n
    assert ((freq - p).abs() < 4.5 * (p * (1 - p) / n).sqrt() + 1e-3).all(), (freq, p)


def test_forcing_rule():
    A, B = 8, 200
    g = torch.Generator().manual_seed(0)
    logits = torch.randn(B, A, generator=g, dtype=torch.float64)
    a0, lp0 = ref.sample_rows(logits, 5, 9)
    expert = torch.randint(0, A, (B,), generator=g)
    mask = (torch.rand(B, generator=g) < 0.7).double()
    expert[mask == 0] = 10 ** 12                                  # garbage where there is no expert action
    expert[int(mask.nonzero()[0])] = A                            # a present id outside [0, A)
    a1, lp1 = ref.force_rows(logits, a0, lp0, expert, mask, 1.0, 5, 9)
    on = mask != 0
    assert torch.equal(a1[on], expert[on]) and torch.equal(a1[~on], a0[~on]) and torch.equal(lp1[~on], lp0[~on])
    assert torch.isnan(lp1[int(mask.nonzero()[0])]) and int(torch.isnan(lp1).sum()) == 1
    ah, _ = ref.force_rows(logits, a0, lp0, expert, mask, 0.5, 5, 9)
    forced = sum(ref.force_uniform(5, 9, n) < 0.5 for n in range(B) if mask[n] != 0)
    assert 0.3 * on.sum() < forced < 0.7 * on.sum()
    assert int(((ah != a0) & on).sum()) <= forced
    an, lpn = ref.force_rows(logits, a0, lp0, expert, mask, 0.0, 5, 9)
    assert torch.equal(an, a0) and torch.equal(lpn, lp0)


def test_heads_backward_against_autograd():
    inp = {k: v.double().requires_grad_(True) for k, v in ref.heads_inputs(17, 96, 5).items()}
    hv = ref.heads_forward(inp["hs"], inp["Wa"], inp["ba"], inp["wc"], inp["bc"])
    dhv = torch.randn(hv.shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    want = torch.autograd.grad((hv * dhv).sum(), [inp[k] for k in ("hs", "Wa", "ba", "wc", "bc")])
    got = ref.heads_backward(inp["hs"].detach(), inp["Wa"].detach(), inp["wc"].detach(), dhv)
    for w, g_ in zip(want, got):
        assert torch.allclose(w, g_, rtol=0, atol=1e-12)


@pytest.mark.parametrize("name", ["a84_b257", "a84_b257_noclipv", "a84_b257_scale30"])
def test_ppo_gradient_against_the_analytic_form(name):
    """autograd's dhv against ppo_loss_kernel's closed form written out in float64"""
    inp = ref.ppo_inputs(name)
    dhv, sums, terms = ref.ppo_loss(inp)
    A, B = inp["hv"].shape[1] - 1, inp["hv"].shape[0]
    hv = inp["hv"].double()
    lp = torch.log_softmax(hv[:, :A], -1)
    p = lp.exp()
    ent = -(p * lp).sum(-1)
    ratio, adv, clip = terms[:, 3], inp["nadv"].double(), inp["clip"]
    use2 = ratio.clamp(1 - clip, 1 + clip) * adv < ratio * adv
    in_rng = (ratio >= 1 - clip) & (ratio <= 1 + clip)
    dla = torch.where(use2 & ~in_rng, torch.zeros_like(adv), -adv) * ratio
    onehot = torch.nn.functional.one_hot(inp["actions"], A).double()
    want = (dla[:, None] * (onehot - p) + inp["ecoef"] * p * (lp + ent[:, None])) * inp["grad_scale"] / B
    keep = ~ref.ppo_branch_rows(inp)
    assert torch.allclose(dhv[keep][:, :A], want[keep], rtol=1e-9, atol=1e-15)
    assert torch.allclose(sums, terms.sum(0))
    assert 1.0 - keep.double().mean().item() <= 0.02


def test_case_tables_cover_the_lists():
    assert {c[0] for c in ref.HEADS_CASES} == {8, 9, 16, 17, 63, 64, 65, 84, 255, 256}
    assert {c[1] for c in ref.HEADS_CASES} == {32, 96, 512, 768} and {c[2] for c in ref.HEADS_CASES} == {1, 5, 37, 130}
    assert len(ref.HEADS_CASES) == len(set(ref.HEADS_CASES)) == 24
    cs = ref.PPO_CASES.values()
    assert {17, 63, 64, 65, 84, 255, 256} <= {c["A"] for c in cs} and {1, 15, 16, 17, 257, 2051, 16401} == {c["B"] for c in cs}
    assert {c["vclip"] >= 0 for c in cs} == {True, False} and any(c["grad_scale"] != 1.0 for c in cs)
    for name in ref.PPO_CASES:                                     # the reference alone keeps the exclusions under the cap
        assert ref.ppo_branch_rows(ref.ppo_inputs(name)).double().mean().item() <= 0.02, name

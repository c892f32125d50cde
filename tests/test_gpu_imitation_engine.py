"""GPU: imitation learning through the engine (``Worker(loss=..., teacher_forcing=...)``) and the plugin loss, against the CPU
oracle policy with the reference loss under torch autograd, ``oracle.ppo.clip_grad_norm_`` and ``adam_step``."""
import functools
import math
import random

import pytest
import torch

import _imitation_ref as ref
from embodied_clip_amd import synthetic as syn
from oracle import policy as opol
from oracle import ppo as oppo

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _sds():
    return syn.rn50_visual_state_dict(0), syn.policy_state_dict(0)


def _worker(N, T, **kw):
    from embodied_clip_amd.engine import Worker
    enc_sd, pol_sd = _sds()
    kw.setdefault("seed", 3)
    kw.setdefault("update_repeats", 2)
    return Worker(N, T=T, device="cuda:0", encoder_sd=enc_sd, policy_sd=pol_sd, **kw)


def _mixed_mask(w):
    """Install the tests' expert mask (both values at these small shapes); ids of steps without an expert action become -1."""
    m = ref.engine_test_mask(w.T, w.N).to(w.env.expert_mask.device)
    assert 0 < int((m[:w.T] == 0).sum()) < w.T * w.N
    w.env.expert_mask.copy_(m)
    w.env.expert_actions[m == 0] = -1
    return w


def _batch(w):
    """The rollout of ``w`` in the oracle's layout (features are the GPU's own, bf16-exact)."""
    T, N, S, C = w.T, w.N, w.S, w.C
    feat = w.feat.float().cpu().view(T + 1, N, S, S, C).permute(0, 1, 4, 2, 3).contiguous()
    masks = w.env.masks.cpu().unsqueeze(-1)
    b = dict(feat=feat[:T], goal=w.env.goals.cpu()[:T], h0=torch.zeros(1, N, w.H), masks=masks[:T], actions=w.actions.cpu(),
             old_log_probs=w.logp.cpu().unsqueeze(-1), old_values=w.values[:T].cpu().unsqueeze(-1),
             returns=w.returns[:T].cpu().unsqueeze(-1), norm_adv=w.nadv.cpu().unsqueeze(-1))
    if hasattr(w.env, "expert_actions"):
        b["expert"], b["emask"] = w.env.expert_actions.cpu()[:T], w.env.expert_mask.cpu()[:T]
    return b


def _il_loss(logits, expert, emask):
    """[U] Imitation.loss: the reference formula of tests/_imitation_ref.py under torch autograd."""
    lp = opol.categorical_log_prob(logits, torch.where(emask != 0, expert, torch.zeros_like(expert)))
    return -(emask * lp).sum() / emask.sum().clamp(min=1)


def _oracle_step(sd, batch, st, ppo=False, il_weight=1.0, lr=3e-4, max_grad_norm=0.5):
    """oracle.ppo.ppo_update_step with the imitation loss (plus the PPO loss with ``ppo``)."""
    names = list(sd)
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
    logits, values, _ = opol.actor_critic_forward(batch["feat"], batch["goal"], batch["h0"], batch["masks"], leaves)
    ce = _il_loss(logits, batch["expert"], batch["emask"])
    total, info = il_weight * ce, {}
    if ppo:
        ptotal, info = oppo.ppo_loss(logits, values, batch["actions"], batch["old_log_probs"], batch["old_values"],
                                     batch["returns"], batch["norm_adv"])
        total = total + ptotal
    grads = torch.autograd.grad(total, [leaves[k] for k in names], allow_unused=True)
    grads = [torch.zeros_like(sd[k]) if g is None else g.clone() for k, g in zip(names, grads)]
    raw = [g.clone() for g in grads]
    info["grad_norm"] = oppo.clip_grad_norm_(grads, max_grad_norm)
    info["expert_cross_entropy"] = float(ce.detach())
    if "step" not in st:
        st.update(step=0, m=[torch.zeros_like(sd[k]) for k in names], v=[torch.zeros_like(sd[k]) for k in names])
    st["step"] += 1
    with torch.no_grad():
        oppo.adam_step([sd[k] for k in names], grads, st["m"], st["v"], st["step"], lr=lr)
    return info, dict(zip(names, raw))


def _check_info(got, info):
    print("worker", got, "oracle", info)
    r = info["expert_cross_entropy"]
    assert abs(got["expert_cross_entropy"] - r) < 2e-4 * max(1.0, abs(r)), (got, info)
    assert abs(got["grad_norm"] - info["grad_norm"]) < 2e-3 * info["grad_norm"], (got, info)


def test_imitation_iteration_matches_oracle():
    T, N, R = 3, 2, 2
    _, pol_sd = _sds()
    w = _worker(N, T, update_repeats=R, loss="imitation")
    _mixed_mask(w)
    w.collect_rollout()
    w.compute_returns()
    torch.cuda.synchronize()
    assert torch.all(w.returns == 0) and torch.all(w.nadv == 0)       # pure imitation launches no GAE
    batch = _batch(w)
    sd_ref = {k: v.clone() for k, v in pol_sd.items()}
    st, step_grads = {}, []
    for _ in range(R):
        info, g_ = _oracle_step(sd_ref, batch, st)
        step_grads.append(g_)
    w.update()
    torch.cuda.synchronize()
    got = w.loss_info()
    assert set(got) == {"expert_cross_entropy", "expert_agreement", "expert_steps", "grad_norm"}
    _check_info(got, info)
    assert got["expert_steps"] == float(batch["emask"].sum()) and 0.0 <= got["expert_agreement"] <= 1.0
    ref.check_updates(w.policy.views(w.params), pol_sd, sd_ref, step_grads, R)
    assert w.opt.step_count == R


def test_imitation_minibatches_share_the_range_denominator():
    """N = 5, M = 2 on one slice: ranges [0, 2) and [2, 5) are both partial slices.  With 64 actors in two slices and M = 3 a
    range spans two parts that share its denominator: covered by the kernel test's split calls and by the two-slice run below."""
    T, N, R, M = 3, 5, 2, 2
    _, pol_sd = _sds()
    w = _worker(N, T, update_repeats=R, loss="imitation", num_mini_batch=M)
    _mixed_mask(w)
    w.collect_rollout()
    w.compute_returns()
    torch.cuda.synchronize()
    batch = _batch(w)
    sd_ref = {k: v.clone() for k, v in pol_sd.items()}
    st, rng, step_grads, seen = {}, random.Random(3), [], []
    for _ in range(R):
        for (s0, s1) in oppo.recurrent_minibatch_ranges(N, M, rng):
            seen.append((s0, s1))
            info, g_ = _oracle_step(sd_ref, oppo.slice_batch(batch, s0, s1), st)
            step_grads.append(g_)
    assert sorted(seen[:M]) == [(0, 2), (2, 5)]
    w.update()
    torch.cuda.synchronize()
    _check_info(w.loss_info(), info)
    ref.check_updates(w.policy.views(w.params), pol_sd, sd_ref, step_grads, R * M)
    assert w.opt.step_count == R * M


def test_two_parts_of_one_range_share_its_denominator():
    """64 actors = two slices of 32; M = 3 cuts at 21 and 43, so range [21, 43) has a part in either slice.  Against the oracle
    on the whole range: one update step."""
    T, N, M = 2, 64, 3
    _, pol_sd = _sds()
    w = _worker(N, T, update_repeats=1, loss="imitation", num_mini_batch=M)
    _mixed_mask(w)
    assert w.ns == 2
    w.collect_rollout()
    w.compute_returns()
    torch.cuda.synchronize()
    batch = _batch(w)
    sd_ref = {k: v.clone() for k, v in pol_sd.items()}
    st, step_grads = {}, []
    for (s0, s1) in oppo.recurrent_minibatch_ranges(N, M, random.Random(3)):
        info, g_ = _oracle_step(sd_ref, oppo.slice_batch(batch, s0, s1), st)
        step_grads.append(g_)
    w.update()
    torch.cuda.synchronize()
    _check_info(w.loss_info(), info)
    ref.check_updates(w.policy.views(w.params), pol_sd, sd_ref, step_grads, M)


def test_without_forcing_the_rollout_is_the_default_workers():
    T, N = 4, 64
    ws = [_worker(N, T, seed=5), _worker(N, T, seed=5, loss="imitation"), _worker(N, T, seed=5, loss="ppo+imitation",
                                                                                 teacher_forcing=lambda s: 0.0)]
    for w in ws:
        w.collect_rollout()
    torch.cuda.synchronize()
    a = ws[0]
    assert not hasattr(a.env, "expert_actions")
    for b in ws[1:]:
        assert torch.equal(a.feat, b.feat) and torch.equal(a.actions, b.actions)
        assert torch.equal(a.logp, b.logp) and torch.equal(a.values, b.values)
    # "ppo+imitation" keeps GAE; its PPO keys are reported beside the imitation ones
    for w in (ws[0], ws[2]):
        w.compute_returns()
    torch.cuda.synchronize()
    assert torch.equal(ws[0].returns, ws[2].returns) and torch.equal(ws[0].nadv, ws[2].nadv)
    assert set(ws[0].loss_info()) == {"action", "value", "entropy", "ratio", "ppo_total", "grad_norm"}


def test_full_teacher_forcing_takes_the_expert_action():
    T, N = 3, 5
    _, pol_sd = _sds()
    w = _worker(N, T, loss="imitation", teacher_forcing=lambda s: 1.0)
    w.env.expert_mask.fill_(1.0)
    w.collect_rollout()
    torch.cuda.synchronize()
    expert = w.env.expert_actions[:T]
    assert torch.equal(w.actions, expert)
    b = _batch(w)
    with torch.no_grad():
        lg, _, _ = opol.actor_critic_forward(b["feat"], b["goal"], b["h0"], b["masks"], pol_sd)
        lp = opol.categorical_log_prob(lg, expert.cpu())
    assert (w.logp.cpu() - lp).abs().max() < 1e-4
    # ... and a schedule is read at the rollout's first total_steps
    seen = []
    w2 = _worker(2, 2, loss="imitation", teacher_forcing=lambda s: seen.append(s) or 0.5)
    w2.iteration(); w2.iteration()
    assert seen == [0, 4] and w2._tf_p == 0.5


def test_action_synchronous_orders_give_the_same_forced_rollout():
    T, N = 4, 64                                        # two slices of 32
    ws = [_worker(N, T, seed=5, update_repeats=1, loss="imitation", teacher_forcing=lambda s: 0.5, sync_actions=s)
          for s in (False, True, "slice")]
    for w in ws:
        _mixed_mask(w).collect_rollout()
    torch.cuda.synchronize()
    a = ws[0]
    assert a.ns == 2
    for b in ws[1:]:
        assert torch.equal(a.actions, b.actions) and torch.equal(a.logp, b.logp) and torch.equal(a.values, b.values)
        assert torch.equal(a.feat, b.feat)
    # the forced steps are the restated draw's, keyed by the worker's seed, iter * (T + 1) + t and the GLOBAL actor id
    free = _worker(N, T, seed=5, update_repeats=1)
    free.collect_rollout()
    torch.cuda.synchronize()
    em = a.env.expert_mask.cpu().numpy()
    for t in range(T):
        forced = torch.from_numpy(ref.teacher_force_decisions(a.seed, t, 0, em[t], 0.5))
        want = torch.where(forced, a.env.expert_actions[t].cpu(), free.actions[t].cpu())
        assert torch.equal(a.actions[t].cpu(), want), t
        assert torch.equal(a.logp[t].cpu()[~forced], free.logp[t].cpu()[~forced])
        assert 0 < int(forced.sum()) < N
    assert torch.equal(ws[1]._actions_host, ws[1].actions[T - 1].cpu())      # the D2H copy carries the forced actions


def test_two_imitation_workers_from_one_seed_end_bit_identical():
    outs = []
    for _ in range(2):
        w = _worker(6, 8, seed=11, loss="imitation", teacher_forcing=lambda s: 0.5)
        _mixed_mask(w)
        for _it in range(2):
            w.iteration()
        torch.cuda.synchronize()
        outs.append(dict(params=w.params.clone(), m=w.opt.m.clone(), actions=w.actions.clone(), logp=w.logp.clone(),
                         sums=torch.stack([sl.il_sums for sl in w.slices]).clone(), gn=w.opt.sumsq[0].clone()))
        del w
    a, b = outs
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_ppo_plus_imitation_matches_oracle():
    T, N, R, wgt = 3, 2, 1, 0.5
    _, pol_sd = _sds()
    w = _worker(N, T, update_repeats=R, loss="ppo+imitation", il_weight=wgt)
    _mixed_mask(w)
    w.collect_rollout()
    w.compute_returns()
    torch.cuda.synchronize()
    batch = _batch(w)
    sd_ref = {k: v.clone() for k, v in pol_sd.items()}
    st = {}
    info, g_ = _oracle_step(sd_ref, batch, st, ppo=True, il_weight=wgt)
    w.update()
    torch.cuda.synchronize()
    got = w.loss_info()
    _check_info(got, info)
    assert abs(got["ppo_total"] - info["ppo_total"]) < 2e-4 * max(1.0, abs(info["ppo_total"]))
    ref.check_updates(w.policy.views(w.params), pol_sd, sd_ref, [g_], R)


def test_imitation_learns_the_synthetic_expert():
    """N = 4, T = 8, four iterations at the default learning rate: the cross-entropy of the last iteration is below half of
    the first's (the oracle policy on random features goes 0.97 -> 0.02 in this set-up on the CPU: the factor 2 is margin)."""
    w = _worker(4, 8, update_repeats=4, loss="imitation")
    _mixed_mask(w)
    ces = []
    for _ in range(4):
        w.iteration()
        ces.append(w.loss_info()["expert_cross_entropy"])
    print("expert_cross_entropy per iteration:", ces)
    assert all(math.isfinite(c) for c in ces)
    assert ces[-1] < 0.5 * ces[0], ces


def test_plugin_loss_gradient_and_zero_mask():
    from embodied_clip_amd.allenact_compat import ActorCriticOutput, CategoricalDistr
    from embodied_clip_amd.imitation import Imitation
    T, N, A = 4, 3, 6
    hv, e, m = ref.make_case(T * N, A, seed=9)
    dev = torch.device("cuda:0")
    logits = hv[:, :A].reshape(T, N, A).to(dev).requires_grad_(True)
    ea = torch.stack([e.float(), m], -1).reshape(T, N, 2).to(dev)
    out = ActorCriticOutput(CategoricalDistr(logits=logits), torch.zeros(T, N, 1, device=dev), {})
    total, info = Imitation().loss(0, {"observations": {"expert_action": ea}}, out)
    total.backward()
    rloss, rdhv, _ = ref.imitation_ref(hv, e, m)
    assert abs(float(total.detach()) - float(rloss)) < 1e-5 * max(1.0, abs(float(rloss)))
    assert info["expert_cross_entropy"] == float(total.detach())
    g = logits.grad.reshape(T * N, A).cpu().double()
    assert ((g - rdhv[:, :A]).norm() / rdhv[:, :A].norm()).item() < 1e-5
    ea0 = ea.clone()
    ea0[..., 1] = 0
    total0, _ = Imitation().loss(0, {"observations": {"expert_action": ea0}}, out)
    assert float(total0) == 0.0


@pytest.mark.parametrize("kw", [dict(goal_in=2, num_actions=4), dict(depth=True)], ids=["pointnav", "rgbd"])
def test_other_agents_train_by_imitation(kw):
    from embodied_clip_amd.engine import Worker
    w = Worker(4, T=2, device="cuda:0", seed=3, update_repeats=1, loss="imitation", teacher_forcing=lambda s: 0.5, **kw)
    p0 = w.params.clone()
    w.iteration()
    torch.cuda.synchronize()
    info = w.loss_info()
    assert all(math.isfinite(v) for v in info.values()), info
    assert info["expert_steps"] > 0 and not torch.equal(w.params, p0)
    assert int(w.actions.min()) >= 0 and int(w.actions.max()) < w.A

"""GPU: the previous-action embedding through the engine -- ``Worker(prev_actions=E)``, the ``Evaluator`` and checkpoints -- against
tests/_prev_action_ref.py replayed on the worker's own features and actions, at the smallest size the engine tests use (8 actors,
T = 4).  Tolerances are those of ``test_worker_iteration_matches_oracle`` / ``test_pointnav_worker_iteration_...``."""
import os
import sys

import pytest
import torch

from embodied_clip_amd import synthetic as syn
from oracle import policy as opol
from oracle import ppo as oppo

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _prev_action_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T, N, R = 4, 8, 2


def _rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-20)).item()


def _worker(E, pol_sd=None, **kw):
    from embodied_clip_amd.engine import Worker
    pkw = dict(prev_action_dims=E, prev_action_null=1, **{k: kw[k] for k in ("goal_in", "num_actions") if k in kw})
    pol_sd = pol_sd if pol_sd is not None else syn.policy_state_dict(0, **pkw)
    w = Worker(N, T=T, device=DEV, seed=3, update_repeats=R, encoder_sd=syn.rn50_visual_state_dict(0), policy_sd=pol_sd, prev_actions=E,
               **kw)
    return w, pol_sd


def _replay(w, pol_sd):
    """the reference's act steps on the worker's features, goals, masks and previous actions -> (values [T+1, N, 1], logp [T, N])"""
    S, C = w.S, w.C
    feat = w.feat.float().cpu().view(T + 1, N, S, S, C).permute(0, 1, 4, 2, 3).contiguous()
    masks, goals = w.env.masks.cpu().unsqueeze(-1), w.env.goals.cpu()
    prev, actions = w.prev_actions.cpu(), w.actions.cpu()
    h = torch.zeros(1, N, w.H)
    vals, lps = [], []
    with torch.no_grad():
        for t in range(T + 1):
            lg, v, h2 = ref.actor_critic_forward(feat[t][None], goals[t][None], prev[t][None], h, masks[t][None], pol_sd, 1)
            vals.append(v[0])
            if t < T:
                lps.append(opol.categorical_log_prob(lg, actions[t][None])[0])
                h = h2
    return feat, masks, goals, prev, actions, torch.stack(vals), torch.stack(lps)


def _check_updates(pv, sd0, sd_ref, step_grads, steps, lr=3e-4):
    """As in test_gpu_engine.py: elements whose gradient stays at the fp32 noise floor of their tensor only get the bound a sign
    flip can reach (2 lr per step); every other element agrees to 0.15 lr per step."""
    for name, pref in sd_ref.items():
        upd, upd_ref = pv[name].cpu() - sd0[name], pref - sd0[name]
        d = (upd - upd_ref).abs()
        gmax = torch.stack([g[name].abs() for g in step_grads]).amax(0)
        well = gmax > 1e-4 * gmax.max()
        assert d.max() <= 2 * steps * lr + 1e-7, (name, d.max())
        if well.any():
            assert d[well].max() < 0.15 * steps * lr + 1e-7, (name, d[well].max())


@pytest.mark.parametrize("E,kw", [(6, {}), (32, dict(goal_in=2, num_actions=4))])
def test_worker_iteration_matches_reference_and_is_reproducible(E, kw):
    """The act steps (each reading the action the step before selected), GAE and the update's optimiser steps against the reference;
    row 0 of the next rollout is row T of this one; a second worker from the same seed ends with the same parameters, bit for bit."""
    w, pol_sd = _worker(E, **kw)
    assert w.policy.prev_action_dims == E and w.prev_actions.shape == (T + 1, N) and w.actions.data_ptr() == w.prev_actions[1].data_ptr()
    w.collect_rollout()
    w.compute_returns()
    torch.cuda.synchronize()
    feat, masks, goals, prev, actions, vals, lps = _replay(w, pol_sd)
    assert not prev[0].any() and torch.equal(prev[1:], actions) and len(set(actions.reshape(-1).tolist())) > 1
    assert _rel(w.values.unsqueeze(-1), vals) < 1e-4
    assert (w.logp.cpu() - lps).abs().max() < 1e-4
    rewards = w.env.rewards.cpu().unsqueeze(-1)
    Rr = oppo.compute_returns(rewards, vals, masks)
    _, nadv = oppo.normalized_advantages(Rr, vals)
    assert _rel(w.returns.unsqueeze(-1), Rr) < 1e-4 and _rel(w.nadv.unsqueeze(-1), nadv) < 1e-3
    sd_ref = {k: v.clone() for k, v in pol_sd.items()}
    batch = dict(feat=feat[:T], goal=goals[:T], h0=torch.zeros(1, N, w.H), masks=masks[:T], actions=actions,
                 old_log_probs=w.logp.cpu().unsqueeze(-1), old_values=w.values[:T].cpu().unsqueeze(-1),
                 returns=w.returns[:T].cpu().unsqueeze(-1), norm_adv=w.nadv.cpu().unsqueeze(-1))
    st, step_grads = {}, []
    with ref.as_oracle_policy(prev[:T], 1):
        for _ in range(R):
            info, g_ = oppo.ppo_update_step(sd_ref, batch, st)
            step_grads.append(g_)
    w.update()
    torch.cuda.synchronize()
    got = w.loss_info()
    assert abs(got["ppo_total"] - info["ppo_total"]) < 2e-4 * max(1.0, abs(info["ppo_total"]))
    assert abs(got["grad_norm"] - info["grad_norm"]) < 2e-3 * info["grad_norm"]
    assert float(step_grads[0][ref.EMB_KEY].abs().max()) > 0
    _check_updates(w.policy.views(w.params), pol_sd, sd_ref, step_grads, R)
    w.after_update()
    last = w.actions[T - 1].clone()
    assert torch.equal(w.prev_actions[0], last)                      # row 0 of rollout k + 1 = row T of rollout k
    w.collect_rollout()
    torch.cuda.synchronize()
    assert torch.equal(w.prev_actions[0], last)
    w2, _ = _worker(E, pol_sd=pol_sd, **kw)
    w2.iteration()
    w2.collect_rollout()
    torch.cuda.synchronize()
    assert torch.equal(w2.actions, w.actions) and torch.equal(w2.params, w.params) and torch.equal(w2.values, w.values)


def test_next_step_sees_the_forced_action():
    """teacher forcing at p = 1: a step that has an expert action takes it, and the NEXT step's previous action is that forced
    action -- the reference replayed with the buffer's previous actions reproduces the worker's values, and replayed with the
    previous actions shifted by one it does not."""
    w, pol_sd = _worker(6, teacher_forcing=lambda steps: 1.0)
    w.collect_rollout()
    torch.cuda.synchronize()
    em, ea = w.env.expert_mask.cpu()[:T] != 0, w.env.expert_actions.cpu()[:T]
    assert em.any() and torch.equal(w.actions.cpu()[em], ea[em])
    assert torch.equal(w.prev_actions[1:].cpu()[em], ea[em])
    _, _, _, prev, _, vals, _ = _replay(w, pol_sd)
    assert _rel(w.values.unsqueeze(-1), vals) < 1e-4
    w.prev_actions.copy_((w.prev_actions + 1) % 6)                   # other previous actions: other values
    _, _, _, _, _, other, _ = _replay(w, pol_sd)
    assert _rel(w.values.unsqueeze(-1), other) > 1e-3


def test_imitation_with_84_actions_runs():
    w, pol_sd = _worker(6, num_actions=84, loss="imitation")
    before = w.params.clone()
    w.iteration()
    torch.cuda.synchronize()
    info = w.loss_info()
    o, k = w.policy.offsets[ref.EMB_KEY]
    assert torch.isfinite(w.params).all() and info["expert_steps"] > 0 and info["expert_cross_entropy"] > 0
    assert not torch.equal(w.params[o:o + k], before[o:o + k])        # the embedding is trained
    assert int(w.actions.max()) > 6


def test_evaluator_greedy_equals_the_handle_level_act_loop():
    """``Evaluator(prev_actions=6, deterministic=True)`` against ``PolicyHandle.act_ex`` stepped by hand over the features a worker
    with the same env stored (the synthetic env's frames do not depend on the actions): actions, log-probs and hv bit for bit."""
    from embodied_clip_amd.evaluate import Evaluator
    pkw = dict(prev_action_dims=6, prev_action_null=1)
    pol_sd = syn.policy_state_dict(0, **pkw)
    ev = Evaluator(N, T=T, device=DEV, seed=3, encoder_sd=syn.rn50_visual_state_dict(0), policy_sd=pol_sd, record=True, deterministic=True,
                   prev_actions=6)
    ev.run(1)
    w, _ = _worker(6, pol_sd=pol_sd)
    w.collect_rollout()
    torch.cuda.synchronize()
    pol, flat = w.policy, w.params
    ws = torch.empty(pol.workspace_bytes(1, N, False), dtype=torch.uint8, device=DEV)
    h, prev = torch.zeros(N, w.H, device=DEV), torch.zeros(N, dtype=torch.int64, device=DEV)
    for t in range(T):
        hv, hf = torch.empty(N, 7, device=DEV), torch.empty(N, w.H, device=DEV)
        act, lp, v = torch.zeros(N, dtype=torch.int64, device=DEV), torch.zeros(N, device=DEV), torch.zeros(N, device=DEV)
        pol.act_ex(flat, w.feat[t].contiguous(), w.env.goals[t].contiguous(), h, w.env.masks[t].contiguous(), N, ws, hv, hf, act, lp, v,
                   deterministic=True, prev_actions=prev)
        torch.cuda.synchronize()
        assert torch.equal(ev.actions[t], act) and torch.equal(ev.logp[t], lp) and torch.equal(ev.hv[t], hv), t
        h, prev = hf, act
    assert len(set(ev.actions.reshape(-1).tolist())) > 1


def test_checkpoint_round_trip_and_refusals(tmp_path):
    from embodied_clip_amd.engine import Worker
    from embodied_clip_amd.evaluate import Evaluator
    w, pol_sd = _worker(6)
    w.iteration()
    path = str(tmp_path / "pa.pt")
    w.save_checkpoint(path)
    ck = torch.load(path, map_location="cpu")
    assert list(ck["model_state_dict"])[-1] == ref.EMB_KEY and tuple(ck["model_state_dict"][ref.EMB_KEY].shape) == (7, 6)
    w2, _ = _worker(6)
    assert not torch.equal(w2.params, w.params)
    w2.load_checkpoint(path)
    assert torch.equal(w2.params, w.params) and w2.total_steps == w.total_steps and torch.equal(w2.opt.m, w.opt.m)
    ev = Evaluator(N, T=T, device=DEV, seed=3, encoder_sd=syn.rn50_visual_state_dict(0), checkpoint=path, prev_actions=6)
    assert torch.equal(ev.params, w.params)
    # a checkpoint without the tensor: refused, naming it
    plain = Worker(N, T=T, device=DEV, seed=3, encoder_sd=syn.rn50_visual_state_dict(0))
    assert plain.prev_actions is None and plain.actions.shape == (T, N)
    old = str(tmp_path / "plain.pt")
    plain.save_checkpoint(old)
    with pytest.raises(KeyError, match="prev_action_embedder.fc.weight"):
        w2.load_checkpoint(old)
    with pytest.raises(KeyError, match="prev_action_embedder.fc.weight"):
        Evaluator(N, T=T, device=DEV, seed=3, encoder_sd=syn.rn50_visual_state_dict(0), checkpoint=old, prev_actions=6)
    for kw in (dict(depth=True), dict(zeroshot=True)):
        with pytest.raises(ValueError, match="prev_actions"):
            Worker(N, T=T, device=DEV, prev_actions=6, **kw)
        with pytest.raises(ValueError, match="prev_actions"):
            Evaluator(N, T=T, device=DEV, prev_actions=6, **kw)
    with pytest.raises(ValueError, match="prev_actions"):
        Worker(N, T=T, device=DEV, prev_actions=65)

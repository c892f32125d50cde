"""The RGB-D agent in the engine (``Worker(depth=True)``, ``Evaluator(depth=True)``) against the CPU oracle: two towers per
frame (``feat`` from the RGB batch, ``feat2`` from the depth batch through the one-channel stem), the dual goal encoder
through act, learn and backward.  Follows tests/test_gpu_engine.py step by step, at its tolerances."""
import os
import random
import sys

import pytest
import torch

from embodied_clip_amd import synthetic as syn
from oracle import clip_resnet as ocr
from oracle import policy as opol
from oracle import ppo as oppo

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_engine import _check_updates, _rel  # noqa: E402

pytestmark = pytest.mark.gpu


def _sds():
    return syn.rn50_visual_state_dict(0), syn.policy_state_dict(0, dual=1)


def _nchw(w, x, T, N):
    return x.float().cpu().view(T + 1, N, w.S, w.S, w.C).permute(0, 1, 4, 2, 3).contiguous()      # [T+1,N,C,S,S]


def _replay(w, f1, f2, pol_sd, T, N):
    masks, goals, actions = w.env.masks.cpu().unsqueeze(-1), w.env.goals.cpu(), w.actions.cpu()
    h = torch.zeros(1, N, w.H)
    vals, lps = [], []
    with torch.no_grad():
        for t in range(T + 1):
            lg, v, h2 = opol.actor_critic_forward((f1[t][None], f2[t][None]), goals[t][None], h, masks[t][None], pol_sd)
            vals.append(v[0])
            if t < T:
                lps.append(opol.categorical_log_prob(lg, actions[t][None])[0])
                h = h2
    return torch.stack(vals), torch.stack(lps)


@pytest.fixture(scope="module")
def rollout():
    """One ``depth=True`` worker after collect_rollout + compute_returns, with its features and the oracle's replay (shared
    by the first two tests; the worker itself is updated by the first)."""
    from embodied_clip_amd.engine import Worker
    assert torch.cuda.is_available()
    T, N, R = 3, 2, 2
    enc_sd, pol_sd = _sds()
    assert len(pol_sd) == 25 and any(k.startswith("goal_visual_encoder.depth_") for k in pol_sd)
    w = Worker(N, T=T, device="cuda:0", seed=3, update_repeats=R, encoder_sd=enc_sd, policy_sd=pol_sd, depth=True)
    w.collect_rollout()
    w.compute_returns()
    torch.cuda.synchronize()
    f1, f2 = _nchw(w, w.feat, T, N), _nchw(w, w.feat2, T, N)
    vals, lps = _replay(w, f1, f2, pol_sd, T, N)
    return dict(w=w, T=T, N=N, R=R, enc_sd=enc_sd, pol_sd=pol_sd, f1=f1, f2=f2, vals=vals, lps=lps)


def test_rgbd_worker_iteration_matches_oracle(rollout):
    w, T, N, R, enc_sd, pol_sd = (rollout[k] for k in ("w", "T", "N", "R", "enc_sd", "pol_sd"))
    f1, f2, vals, lps = (rollout[k] for k in ("f1", "f2", "vals", "lps"))
    assert w.policy.cfg["dual"] == 1 and len(w.policy.offsets) == 25
    assert w.feat2.shape == w.feat.shape and w.feat2.dtype == w.feat.dtype
    # (1) both towers: every stored feature row vs the fp32 oracle on the env's RGB and depth frames
    frames, depth = w.env.frames.cpu(), w.env.depth.cpu()
    for t in range(T + 1):
        r1 = _rel(f1[t], ocr.clip_resnet_preprocessor(frames[t % frames.shape[0]], enc_sd))
        r2 = _rel(f2[t], ocr.clip_resnet_preprocessor(depth[t % depth.shape[0]], enc_sd))
        print(f"t={t}: feat rel-L2 {r1:.3e}, feat2 rel-L2 {r2:.3e}")
        assert r1 < 2e-2, (t, r1)
        assert r2 < 2e-2, (t, r2)
    # (2) act steps
    masks, goals, actions = w.env.masks.cpu().unsqueeze(-1), w.env.goals.cpu(), w.actions.cpu()
    assert int(actions.min()) >= 0 and int(actions.max()) < 6
    assert _rel(w.values.unsqueeze(-1), vals) < 1e-4
    assert (w.logp.cpu() - lps).abs().max() < 1e-4
    # (3) GAE + advantage normalisation
    rewards = w.env.rewards.cpu().unsqueeze(-1)
    Rr = oppo.compute_returns(rewards, vals, masks)
    _, nadv = oppo.normalized_advantages(Rr, vals)
    assert _rel(w.returns.unsqueeze(-1), Rr) < 1e-4
    assert _rel(w.nadv.unsqueeze(-1), nadv) < 1e-3
    # (4) update_repeats optimiser steps over all 25 tensors
    sd_ref = {k: v.clone() for k, v in pol_sd.items()}
    batch = dict(feat=(f1[:T], f2[:T]), goal=goals[:T], h0=torch.zeros(1, N, w.H), masks=masks[:T], actions=actions,
                 old_log_probs=w.logp.cpu().unsqueeze(-1), old_values=w.values[:T].cpu().unsqueeze(-1),
                 returns=w.returns[:T].cpu().unsqueeze(-1), norm_adv=w.nadv.cpu().unsqueeze(-1))
    st, step_grads = {}, []
    for _ in range(R):
        info, g_ = oppo.ppo_update_step(sd_ref, batch, st)
        step_grads.append(g_)
    w.update()
    torch.cuda.synchronize()
    got = w.loss_info()
    print("rgbd update:", got, info)
    assert abs(got["ppo_total"] - info["ppo_total"]) < 2e-4 * max(1.0, abs(info["ppo_total"]))
    assert abs(got["grad_norm"] - info["grad_norm"]) < 2e-3 * info["grad_norm"]
    assert len(sd_ref) == 25
    _check_updates(w.policy.views(w.params), pol_sd, sd_ref, step_grads, R)
    f2T = w.feat2[T].clone()
    w.after_update()
    assert torch.equal(w.feat[0], w.feat[T]) and torch.equal(w.feat2[0], f2T) and torch.equal(w.feat2[0], w.feat2[T])


def test_the_depth_stream_is_the_depth_stream(rollout):
    """``feat2`` is not a copy of ``feat``, and the policy reads the two in the right order: the oracle's replay with the
    tuple swapped misses the worker's values."""
    w, T, N, pol_sd = (rollout[k] for k in ("w", "T", "N", "pol_sd"))
    f1, f2, vals = rollout["f1"], rollout["f2"], rollout["vals"]
    # not equal, and further apart than a tower is from its oracle (2e-2): feat2 cannot be the RGB batch's features
    d12 = _rel(f2, f1)
    print(f"feat2 vs feat rel-L2 {d12:.3e}")
    assert not torch.equal(f1, f2) and d12 > 2e-2, d12
    vals_sw, _ = _replay(w, f2, f1, pol_sd, T, N)
    miss = _rel(w.values.unsqueeze(-1), vals_sw)          # (the rollout's values: the update does not touch them)
    print(f"swapped-tuple replay misses the values by rel-L2 {miss:.3e}")
    assert miss > 1e-4, miss


def test_rgbd_worker_num_mini_batch_matches_oracle():
    """N = 5, M = 2 -> ranges [0,2) and [2,5): both partial, i.e. the staging copy of BOTH feature buffers."""
    from embodied_clip_amd.engine import Worker
    T, N, R, M = 3, 5, 2, 2
    enc_sd, pol_sd = _sds()
    w = Worker(N, T=T, device="cuda:0", seed=3, update_repeats=R, encoder_sd=enc_sd, policy_sd=pol_sd, num_mini_batch=M, depth=True)
    w.collect_rollout()
    w.compute_returns()
    torch.cuda.synchronize()
    f1, f2 = _nchw(w, w.feat, T, N), _nchw(w, w.feat2, T, N)
    masks = w.env.masks.cpu().unsqueeze(-1)
    batch = dict(goal=w.env.goals.cpu()[:T], h0=torch.zeros(1, N, w.H), masks=masks[:T],
                 actions=w.actions.cpu(), old_log_probs=w.logp.cpu().unsqueeze(-1),
                 old_values=w.values[:T].cpu().unsqueeze(-1), returns=w.returns[:T].cpu().unsqueeze(-1),
                 norm_adv=w.nadv.cpu().unsqueeze(-1))
    sd_ref = {k: v.clone() for k, v in pol_sd.items()}
    st, rng, seen, step_grads = {}, random.Random(3), [], []
    for _ in range(R):
        for (s0, s1) in oppo.recurrent_minibatch_ranges(N, M, rng):
            seen.append((s0, s1))
            mb = oppo.slice_batch(batch, s0, s1)
            mb["feat"] = (f1[:T, s0:s1].contiguous(), f2[:T, s0:s1].contiguous())      # (slice_batch cannot cut a tuple)
            info, g_ = oppo.ppo_update_step(sd_ref, mb, st)
            step_grads.append(g_)
    assert sorted(seen[:M]) == [(0, 2), (2, 5)] and st["step"] == R * M
    w.update()
    torch.cuda.synchronize()
    got = w.loss_info()
    assert abs(got["ppo_total"] - info["ppo_total"]) < 5e-4 * max(1.0, abs(info["ppo_total"]))
    _check_updates(w.policy.views(w.params), pol_sd, sd_ref, step_grads, R * M)
    assert w.opt.step_count == R * M
    assert w.slices[0].feat2_mb is not None and w.slices[0].feat2_mb.data_ptr() != w.slices[0].feat_mb.data_ptr()


def test_rgbd_two_stream_encode_matches_one_stream():
    from embodied_clip_amd.engine import Worker
    enc_sd = syn.rn50_visual_state_dict(0)
    w1 = Worker(64, T=1, device="cuda:0", seed=3, update_repeats=1, encoder_sd=enc_sd, encoder_streams=1, depth=True)
    w2 = Worker(64, T=1, device="cuda:0", seed=3, update_repeats=1, encoder_sd=enc_sd, encoder_streams=2, depth=True)
    assert not w1.enc_streams and len(w2.enc_streams) == 2
    w1.iteration(); w2.iteration()
    torch.cuda.synchronize()
    assert _rel(w1.feat, w2.feat) <= 7e-3
    assert _rel(w1.feat2, w2.feat2) <= 7e-3
    assert (w1.actions == w2.actions).float().mean().item() >= 0.9


def test_rgbd_action_synchronous_orders_give_the_same_rollout():
    """The depth batch served for env step k goes with RGB batch k in all three stepping orders."""
    from embodied_clip_amd.engine import Worker
    T, N = 4, 64                                        # two slices of 32
    enc_sd, pol_sd = _sds()
    ws = [Worker(N, T=T, device="cuda:0", seed=5, update_repeats=1, encoder_sd=enc_sd, policy_sd=pol_sd, sync_actions=s, depth=True)
          for s in (False, True, "slice")]
    for w in ws:
        w.iteration()
    torch.cuda.synchronize()
    a, b, c = ws
    for o in (b, c):
        assert torch.equal(a.actions, o.actions) and torch.equal(a.logp, o.logp) and torch.equal(a.values, o.values)
        assert torch.equal(a.feat, o.feat) and torch.equal(a.feat2, o.feat2) and o.env._k == a.env._k
        assert (a.params - o.params).abs().max().item() <= 2 * 3e-4 + 1e-7
    assert b.ns == 2
    assert not torch.equal(a.feat2[1], a.feat2[2])      # consecutive steps see different depth batches


def test_rgbd_two_runs_from_one_seed_end_bit_identical():
    from embodied_clip_amd.engine import Worker
    enc_sd, pol_sd = _sds()
    outs = []
    for _ in range(2):
        w = Worker(6, T=8, device="cuda:0", seed=11, update_repeats=2, encoder_sd=enc_sd, policy_sd=pol_sd, encoder_streams=1, depth=True)
        assert w.ns == 1
        for _it in range(2):
            w.iteration()
        torch.cuda.synchronize()
        outs.append(dict(params=w.params.clone(), m=w.opt.m.clone(), v=w.opt.v.clone(), actions=w.actions.clone(), logp=w.logp.clone()))
        del w
        torch.cuda.empty_cache()
    a, b = outs
    assert a["params"].abs().max() > 0
    for k in a:
        assert torch.equal(a[k], b[k]), (k, (a[k].double() - b[k].double()).abs().max().item())


def test_rgbd_evaluator_takes_the_workers_actions_and_loads_its_checkpoint(tmp_path):
    from embodied_clip_amd.engine import Worker
    from embodied_clip_amd.evaluate import Evaluator
    T, N = 4, 6
    enc_sd, pol_sd = _sds()
    w = Worker(N, T=T, device="cuda:0", seed=5, update_repeats=1, encoder_sd=enc_sd, policy_sd=pol_sd, depth=True)
    ev = Evaluator(N, T=T, device="cuda:0", seed=5, encoder_sd=enc_sd, policy_sd=pol_sd, depth=True, record=True)
    assert ev.slices[0].feat2.shape == ev.slices[0].feat.shape and ev.slices[0].feat.shape[0] == 2
    w.collect_rollout()
    ev.run(1)
    torch.cuda.synchronize()
    assert torch.equal(ev.actions, w.actions) and torch.equal(ev.logp, w.logp) and torch.equal(ev.values, w.values[:T])
    # checkpoint: the 25 tensors go through save -> Evaluator(checkpoint=) and Worker.load_checkpoint
    w.compute_returns(); w.update(); w.after_update()
    path = str(tmp_path / "rgbd.pt")
    w.save_checkpoint(path)
    ck = torch.load(path, map_location="cpu")
    assert len(ck["model_state_dict"]) == 25
    ev2 = Evaluator(N, T=T, device="cuda:0", seed=5, encoder_sd=enc_sd, checkpoint=path, depth=True, deterministic=True)
    assert torch.equal(ev2.params, w.params)
    info = ev2.run(2)
    assert set(info) >= {"episodes", "reward", "ep_length", "success"} and info["episodes"] >= 0
    w2 = Worker(N, T=T, device="cuda:0", seed=5, update_repeats=1, encoder_sd=enc_sd, depth=True)
    w2.load_checkpoint(path)
    assert torch.equal(w2.params, w.params)


def test_rgbd_refusals():
    from embodied_clip_amd.engine import SyntheticEnv, Worker
    from embodied_clip_amd.evaluate import Evaluator
    for kw in (dict(encoder="vit"), dict(encoder="imagenet_rn18"), dict(zeroshot=True), dict(goal_in=2, num_actions=4),
               dict(frames_host=True)):
        with pytest.raises(ValueError, match="depth=True"):
            Worker(4, T=2, device="cuda:0", depth=True, **kw)
    for kw in (dict(encoder="vit"), dict(encoder="imagenet_rn50"), dict(zeroshot=True), dict(goal_in=2, num_actions=4)):
        with pytest.raises(ValueError, match="depth=True"):
            Evaluator(4, T=2, device="cuda:0", depth=True, **kw)
    env = SyntheticEnv(4, 2, "cuda:0", 1000, res=32)             # an env without depth frames
    with pytest.raises(ValueError, match="depth"):
        Evaluator(4, T=2, device="cuda:0", depth=True, env=env)

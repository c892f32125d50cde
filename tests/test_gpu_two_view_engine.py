"""GPU: the two-view rearrangement agent through the engine -- ``Worker(net="two_view", num_actions=84, loss="imitation",
rnn_type="LSTM", prev_actions=...)``, the ``Evaluator`` and checkpoints -- at 4 actors x rollout 4 on the seeded CLIP-RN50 tower
the other engine tests build.  Everything behind the two stored feature maps is held to the float64 reference of
tests/_two_view_ref.py replayed on the worker's recorded rollout, at GRAD_TOL per gradient tensor (visual_attention.2.bias, which
is analytically zero, against the scale of visual_attention.2.weight; the critic, which the imitation loss does not reach, exactly
zero).  ``sl.feat2`` holds the goal view's features: equal to encoding that frame alone.

Measured on an MI355X: the worker's gradients within 4.8e-6 of the reference (state_encoder.rnn.weight_ih_l0; the front's six
tensors within 4.2e-6, |grad visual_attention.2.bias| 1.1e-7 of its neighbour's norm).
"""
import functools
import os
import sys
import types

import pytest
import torch

from embodied_clip_amd import synthetic as syn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _two_view_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T, N, C, A, E = 4, 4, 2048, 84, 96
AGENT = dict(net="two_view", num_actions=A, rnn_type="LSTM", prev_actions=E)


@functools.lru_cache(maxsize=None)
def _enc_sd():
    return syn.rn50_visual_state_dict(0)


def _worker(**kw):
    from embodied_clip_amd.engine import Worker
    args = dict(AGENT, loss="imitation", update_repeats=1, encoder_sd=_enc_sd())
    args.update(kw)
    return Worker(N, T=T, device=DEV, seed=3, **args)


def test_worker_gradients_against_the_reference_replay():
    w = _worker()
    assert w.dual and w.two_view_net and w.feat.dtype == torch.bfloat16
    assert tuple(w.feat.shape) == tuple(w.feat2.shape) == (T + 1, N, 49, C)
    assert w.policy.two_view_cfg["in_channels"] == C and w.policy.prev_action_dims == E
    sd = {k: v.detach().cpu().clone() for k, v in w.policy.views(w.params).items()}
    w.collect_rollout()
    w.compute_returns()
    torch.cuda.synchronize()
    cpu = lambda t: t.detach().cpu()
    case = (T, N, 49, C, 512, E, A, 1, ref.LSTM)
    batch = dict(u=cpu(w.feat[:T]).float(), w=cpu(w.feat2[:T]).float(), prev_actions=cpu(w.prev_actions[:T]), state0=cpu(w.h_start),
                 masks=cpu(w.env.masks[:T]).unsqueeze(-1), actions=cpu(w.actions), expert=cpu(w.env.expert_actions[:T]),
                 emask=cpu(w.env.expert_mask[:T]), noise=[torch.zeros(T, N, 1)] * 4)
    assert float(batch["u"].abs().max()) > 0 and float(batch["w"].abs().max()) > 0 and not torch.equal(batch["u"], batch["w"])
    r = ref.policy_reference(case, sd, batch, "imitation")
    lp = torch.log_softmax(r["logits"], -1).gather(-1, batch["actions"].unsqueeze(-1)).squeeze(-1)
    assert (cpu(w.logp).double() - lp).abs().max() < 1e-4 and ref.rel_l2(w.values[:T], r["values"].squeeze(-1)) < 1e-4
    w.update()
    torch.cuda.synchronize()
    gv = w.policy.views(w.grads)
    assert set(gv) == set(r["grads"])
    errs = {}
    for k, g in r["grads"].items():
        if k == ref.B2:
            errs[k] = float(gv[k].double().abs().max().cpu() / r["grads"][ref.W2].norm())
        elif k.startswith("critic."):
            assert float(g.abs().max()) == 0.0 and float(gv[k].abs().max()) == 0.0, k      # the imitation loss has no value term
        else:
            assert float(g.abs().max()) > 0, k
            errs[k] = ref.rel_l2(gv[k], g)
    print("gradient rel-L2:", {k: "%.3e" % e for k, e in errs.items()})
    for k, e in errs.items():
        assert e <= ref.GRAD_TOL, (k, e)


def test_feat2_holds_the_goal_views_features():
    from embodied_clip_amd.encoder import RN50Trunk
    w = _worker()
    w.collect_rollout()
    torch.cuda.synchronize()
    enc = RN50Trunk(_enc_sd(), device=torch.device(DEV))
    enc.set_l1_rebuild(True)
    for t in (0, T):             # step t reads pool entry t
        alone = enc.forward(w.env.observe_goal_view_at(t).contiguous())
        torch.cuda.synchronize()
        assert torch.equal(alone.reshape(N, 49, C), w.feat2[t]), t
        assert not torch.equal(w.feat2[t], w.feat[t])
    # the goal view comes from a stream of its own: nothing the env built before changes
    from embodied_clip_amd.engine import SyntheticEnv
    plain = SyntheticEnv(N, T, torch.device(DEV), seed=1000, expert=True, num_actions=A)
    for name in ("frames", "masks", "goals", "rewards", "expert_actions", "expert_mask"):
        assert torch.equal(getattr(plain, name), getattr(w.env, name)), name
    assert not torch.equal(w.env.goal_frames, w.env.frames)


def test_two_workers_from_one_seed_end_equal():
    kw = dict(num_mini_batch=2, sync_actions=True, rnn_layers=2, teacher_forcing=lambda steps: 0.5)
    a, b = _worker(**kw), _worker(**kw)
    p0 = a.params.clone()
    for w in (a, b):
        w.iteration()
        w.iteration()
    torch.cuda.synchronize()
    assert torch.equal(a.params, b.params) and torch.equal(a.actions, b.actions) and torch.equal(a.feat2, b.feat2)
    assert not torch.equal(a.params, p0) and torch.isfinite(a.params).all()


@pytest.mark.parametrize("kw", [dict(loss="ppo"), dict(loss="ppo+imitation", rnn_type="GRU", prev_actions=0, num_actions=6),
                                dict(loss="ppo", num_actions=256, prev_actions=512)])
def test_other_losses_and_shapes_run(kw):
    w = _worker(**kw)
    p0 = w.params.clone()
    w.iteration()
    torch.cuda.synchronize()
    assert torch.isfinite(w.params).all() and not torch.equal(w.params, p0) and w.loss_info()["grad_norm"] > 0


def test_checkpoint_round_trip_and_refusal_by_tensor_name(tmp_path):
    w = _worker()
    w.iteration()
    path = str(tmp_path / "two_view.pt")
    w.save_checkpoint(path)
    v = _worker()
    assert not torch.equal(v.params, w.params)
    v.load_checkpoint(path)
    assert torch.equal(v.params, w.params) and v.total_steps == w.total_steps
    other = str(tmp_path / "goal_encoder.pt")
    torch.save({"model_state_dict": syn.policy_state_dict(0), "optimizer_state_dict": {}, "total_steps": 0}, other)
    with pytest.raises(KeyError, match="visual_encoder.0.weight"):
        w.load_checkpoint(other)


def test_evaluator_runs_and_reports_episodes(tmp_path):
    from embodied_clip_amd.evaluate import Evaluator
    w = _worker()
    path = str(tmp_path / "w.pt")
    w.save_checkpoint(path)
    w.collect_rollout()
    ev = Evaluator(N, T=T, device=DEV, seed=3, encoder_sd=_enc_sd(), checkpoint=path, record=True, **AGENT)
    assert tuple(ev.slices[0].feat2.shape) == (2, N, 49, C)
    info = ev.run(1)
    torch.cuda.synchronize()
    assert torch.equal(ev.actions, w.actions) and torch.equal(ev.logp, w.logp) and "episodes" in info
    ev2 = Evaluator(N, T=T, device=DEV, seed=3, encoder_sd=_enc_sd(), checkpoint=path, deterministic=True, record=True, **AGENT)
    ev2.run(1)
    torch.cuda.synchronize()
    assert torch.equal(ev2.actions, ev2.hv[..., :A].argmax(-1))


def test_refusals_before_any_allocation():
    from embodied_clip_amd.engine import Worker
    from embodied_clip_amd.evaluate import Evaluator
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    no_goal_env = types.SimpleNamespace(host=False, N=N, T=T)
    bad = (dict(depth=True), dict(zeroshot=True), dict(goal_in=2), dict(sensors=(2, 2)), dict(goal_ids=False), dict(pooling="avgpool"),
           dict(encoder="vit"), dict(prev_actions=513))
    for cls, extra in ((Worker, (dict(frames_host=True),)), (Evaluator, (dict(env=no_goal_env),))):
        for b in bad + extra:
            with pytest.raises(ValueError):
                cls(N, T=T, device=DEV, **{**AGENT, **b})
    assert torch.cuda.memory_allocated() == before

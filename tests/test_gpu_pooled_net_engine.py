"""GPU: the pooled-embedding net through the engine -- ``Worker(net="pooled", ...)``, the ``Evaluator`` and checkpoints -- at the
smallest size the engine tests use (8 actors, T = 4).  The worker's gradients are held to the float64 reference of
tests/_pooled_net_ref.py replayed on the worker's own recorded rollout, per tensor, within the policy path's gradient bound
(rel-L2 2e-4); measured on an MI355X the worst tensor lies at 4.8e-6 (visual_fc's weight), with both poolings."""
import os
import sys

import pytest
import torch

from embodied_clip_amd import synthetic as syn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _pooled_net_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T, N = 4, 8
AGENT = dict(net="pooled", sensors=(2, 2), goal_ids=True, rnn_type="LSTM", rnn_layers=2, prev_actions=32)


def _worker(pooling="attnpool", **kw):
    from embodied_clip_amd.engine import Worker
    args = dict(AGENT, pooling=pooling, update_repeats=1, encoder_sd=syn.rn50_visual_state_dict(0))
    args.update(kw)
    return Worker(N, T=T, device=DEV, seed=3, **args)


@pytest.mark.parametrize("pooling,D", [("attnpool", 1024), ("avgpool", 2048)])
def test_worker_iteration_gradients_match_the_reference_on_the_recorded_rollout(pooling, D):
    w = _worker(pooling)
    assert w.feat.dtype == torch.float32 and tuple(w.feat.shape) == (T + 1, N, 1, D)       # the rollout buffer: one vector per frame
    assert tuple(w.env.sensors.shape) == (T + 1, N, 4) and w.policy.pooled_cfg["embed_in"] == D
    sd = {k: v.detach().cpu().clone() for k, v in w.policy.views(w.params).items()}
    w.collect_rollout()
    w.compute_returns()
    torch.cuda.synchronize()
    cpu = lambda t: t.detach().cpu()
    case = (T, N, D, 512, 12, (2, 2), 32, 1, 6, 2, ref.LSTM)
    batch = dict(embed=cpu(w.feat[:T]).reshape(T, N, D), goal=cpu(w.env.goals[:T]), sensors=cpu(w.env.sensors[:T]),
                 prev_actions=cpu(w.prev_actions[:T]), state0=cpu(w.h_start), masks=cpu(w.env.masks[:T]).unsqueeze(-1),
                 actions=cpu(w.actions), old_log_probs=cpu(w.logp).unsqueeze(-1), old_values=cpu(w.values[:T]).unsqueeze(-1),
                 returns=cpu(w.returns[:T]).unsqueeze(-1), norm_adv=cpu(w.nadv).unsqueeze(-1))
    assert len(set(batch["actions"].reshape(-1).tolist())) > 1 and float(batch["embed"].abs().max()) > 0
    r = ref.policy_reference(case, sd, batch, replay=batch)
    # the act steps the worker took: its values and log-probabilities are the reference's on the same rollout
    assert ref.rel_l2(w.values[:T], r["values"].squeeze(-1)) < 1e-4
    lp = torch.log_softmax(r["logits"], -1).gather(-1, batch["actions"].unsqueeze(-1)).squeeze(-1)
    assert (cpu(w.logp).double() - lp).abs().max() < 1e-4
    w.update()
    torch.cuda.synchronize()
    assert abs(w.loss_info()["ppo_total"] - r["info"]["ppo_total"]) < 2e-4 * max(1.0, abs(r["info"]["ppo_total"]))
    gv = w.policy.views(w.grads)
    assert set(gv) == set(r["grads"])
    errs = {k: ref.rel_l2(gv[k], g) for k, g in r["grads"].items()}
    print(pooling, "gradient rel-L2:", errs)
    for k, e in errs.items():
        assert float(r["grads"][k].abs().max()) > 0 and e <= ref.GRAD_TOL, (k, e)
    w.after_update()
    assert torch.equal(w.prev_actions[0], w.actions[T - 1]) and w.total_steps == T * N


def test_imitation_leg_with_84_actions_runs():
    w = _worker("avgpool", sensors=(3,), goal_ids=False, num_actions=84, loss="imitation", teacher_forcing=lambda steps: 0.5)
    assert "obj_categories_embedding.weight" not in w.policy.offsets and "tgt_embeding.weight" in w.policy.offsets
    p0 = w.params.clone()
    w.iteration()
    torch.cuda.synchronize()
    info = w.loss_info()
    assert info["expert_steps"] > 0 and info["expert_cross_entropy"] == info["expert_cross_entropy"] and info["grad_norm"] > 0
    assert torch.isfinite(w.params).all() and not torch.equal(w.params, p0)
    em = w.env.expert_mask[:T] != 0
    assert bool((w.actions[em] == w.env.expert_actions[:T][em]).float().mean() > 0.3)        # forcing took place


def test_two_workers_from_one_seed_end_with_equal_parameters(tmp_path):
    kw = dict(loss="ppo+imitation", num_mini_batch=2, sync_actions=True, update_repeats=2)
    a, b = _worker("attnpool", **kw), _worker("attnpool", **kw)
    for w in (a, b):
        w.iteration()
        w.iteration()
    torch.cuda.synchronize()
    assert torch.equal(a.params, b.params) and torch.equal(a.actions, b.actions) and torch.equal(a.h, b.h)
    # a checkpoint round-trips ...
    path = str(tmp_path / "pooled.pt")
    a.save_checkpoint(path)
    c = _worker("attnpool", **kw)
    assert not torch.equal(c.params, a.params)
    c.load_checkpoint(path)
    assert torch.equal(c.params, a.params) and torch.equal(c.opt.m, a.opt.m) and c.total_steps == a.total_steps
    # ... and one of another net is refused by tensor name
    other = str(tmp_path / "goal_encoder.pt")
    torch.save({"model_state_dict": syn.policy_state_dict(0), "optimizer_state_dict": {}, "total_steps": 0}, other)
    with pytest.raises(KeyError, match="visual_fc.1.weight"):
        c.load_checkpoint(other)
    from embodied_clip_amd.engine import Worker
    w = Worker(N, T=T, device=DEV, seed=3, encoder_sd=syn.rn50_visual_state_dict(0))
    with pytest.raises((KeyError, ValueError)):
        w.load_checkpoint(path)                              # the reverse: the goal-encoder agent refuses the pooled net's file


@pytest.mark.parametrize("pooling", ["attnpool", "avgpool"])
def test_evaluator_takes_the_workers_actions(pooling, tmp_path):
    """with equal weights, seed and env the Evaluator's first chunk selects what the Worker's first rollout selected"""
    from embodied_clip_amd.evaluate import Evaluator
    w = _worker(pooling)
    path = str(tmp_path / "w.pt")
    w.save_checkpoint(path)
    w.collect_rollout()
    ev = Evaluator(N, T=T, device=DEV, seed=3, encoder_sd=syn.rn50_visual_state_dict(0), checkpoint=path, record=True,
                   prev_action_null_token=True, **{**AGENT, "pooling": pooling})
    info = ev.run(1)
    torch.cuda.synchronize()
    assert torch.equal(ev.actions, w.actions) and torch.equal(ev.logp, w.logp) and "episodes" in info
    ev2 = Evaluator(N, T=T, device=DEV, seed=3, encoder_sd=syn.rn50_visual_state_dict(0), checkpoint=path, deterministic=True, record=True,
                    **{**AGENT, "pooling": pooling})
    ev2.run(1)
    torch.cuda.synchronize()
    assert torch.equal(ev2.actions, ev2.hv[..., :6].argmax(-1))


def test_refusals_before_any_allocation():
    from embodied_clip_amd.engine import Worker
    from embodied_clip_amd.evaluate import Evaluator
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    for cls in (Worker, Evaluator):
        for bad in (dict(depth=True), dict(zeroshot=True), dict(goal_in=2), dict(encoder="vit"), dict(encoder="imagenet_rn18", pooling="attnpool"),
                    dict(pooling="maxpool"), dict(goal_ids=False), dict(sensors=(4, 5)), dict(net="pooled2")):
            with pytest.raises(ValueError):
                cls(N, T=T, device=DEV, **{**dict(net="pooled"), **bad})
        with pytest.raises(ValueError):
            cls(N, T=T, device=DEV, sensors=(2,))            # sensors belong to the pooled net
    assert torch.cuda.memory_allocated() == before


def test_imagenet_tower_with_avgpool_runs():
    from embodied_clip_amd.engine import Worker
    w = Worker(N, T=T, device=DEV, seed=1, net="pooled", pooling="avgpool", encoder="imagenet_rn18", sensors=(3,), goal_ids=False,
               num_actions=4, update_repeats=1)
    assert tuple(w.feat.shape) == (T + 1, N, 1, 512)
    w.iteration()
    torch.cuda.synchronize()
    assert torch.isfinite(w.params).all() and w.loss_info()["grad_norm"] > 0

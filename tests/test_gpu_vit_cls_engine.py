"""GPU: the pooled net over the ViT's class embedding through the engine -- ``Worker(net="pooled", encoder="vit", pooling="cls")``,
the ``Evaluator`` and checkpoints -- at 8 actors and T = 4 on a three-block seeded tower.  The worker's gradients are held to the
float64 reference of tests/_pooled_net_ref.py replayed on the worker's own recorded rollout, per tensor, within that file's
GRAD_TOL, as tests/test_gpu_pooled_net_engine.py does for the RN50 poolings."""
import os
import sys

import pytest
import torch

from embodied_clip_amd import synthetic as syn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _pooled_net_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T, N, D = 4, 8, 768
AGENT = dict(net="pooled", encoder="vit", pooling="cls", sensors=(2, 2), goal_ids=True, rnn_type="LSTM", rnn_layers=2, prev_actions=32)


@pytest.fixture(scope="module")
def vit_sd():
    return syn.vit_visual_state_dict(0, layers=3)


def _worker(sd, **kw):
    from embodied_clip_amd.engine import Worker
    args = dict(AGENT, update_repeats=1, encoder_sd=sd)
    args.update(kw)
    return Worker(N, T=T, device=DEV, seed=3, **args)


def test_worker_iteration_gradients_match_the_reference_on_the_recorded_rollout(vit_sd):
    w = _worker(vit_sd)
    assert w.feat.dtype == torch.float32 and tuple(w.feat.shape) == (T + 1, N, 1, D)       # the rollout buffer: one vector per frame
    assert all(sl.tok is None and sl.trunk_out is None for sl in w.slices)                # no token buffer
    assert w.policy.pooled_cfg["embed_in"] == D
    sd = {k: v.detach().cpu().clone() for k, v in w.policy.views(w.params).items()}
    w.collect_rollout()
    w.compute_returns()
    torch.cuda.synchronize()
    cpu = lambda t: t.detach().cpu()      # noqa: E731
    emb = cpu(w.feat[:T]).reshape(T, N, D)
    assert torch.equal(emb, emb.to(torch.bfloat16).float()) and float(emb.abs().max()) > 0      # bf16 values, as both routes deliver
    case = (T, N, D, 512, 12, (2, 2), 32, 1, 6, 2, ref.LSTM)
    batch = dict(embed=emb, goal=cpu(w.env.goals[:T]), sensors=cpu(w.env.sensors[:T]),
                 prev_actions=cpu(w.prev_actions[:T]), state0=cpu(w.h_start), masks=cpu(w.env.masks[:T]).unsqueeze(-1),
                 actions=cpu(w.actions), old_log_probs=cpu(w.logp).unsqueeze(-1), old_values=cpu(w.values[:T]).unsqueeze(-1),
                 returns=cpu(w.returns[:T]).unsqueeze(-1), norm_adv=cpu(w.nadv).unsqueeze(-1))
    assert len(set(batch["actions"].reshape(-1).tolist())) > 1
    r = ref.policy_reference(case, sd, batch, replay=batch)
    assert ref.rel_l2(w.values[:T], r["values"].squeeze(-1)) < 1e-4
    lp = torch.log_softmax(r["logits"], -1).gather(-1, batch["actions"].unsqueeze(-1)).squeeze(-1)
    assert (cpu(w.logp).double() - lp).abs().max() < 1e-4
    w.update()
    torch.cuda.synchronize()
    assert abs(w.loss_info()["ppo_total"] - r["info"]["ppo_total"]) < 2e-4 * max(1.0, abs(r["info"]["ppo_total"]))
    gv = w.policy.views(w.grads)
    assert set(gv) == set(r["grads"])
    errs = {k: ref.rel_l2(gv[k], g) for k, g in r["grads"].items()}
    print("cls gradient rel-L2:", errs)
    for k, e in errs.items():
        assert float(r["grads"][k].abs().max()) > 0 and e <= ref.GRAD_TOL, (k, e)
    w.after_update()
    assert torch.equal(w.prev_actions[0], w.actions[T - 1]) and w.total_steps == T * N


def test_patch16_tower_of_197_tokens_runs():
    """a ViT-B/16-geometry tower: 14 x 14 + 1 tokens through the general attention core; the rollout still holds [D] per frame"""
    sd = syn.vit_visual_state_dict(0, layers=3, patch_size=16)
    w = _worker(sd)
    assert w.slices[0].enc.L == 197 and tuple(w.feat.shape) == (T + 1, N, 1, D)
    w.iteration()
    torch.cuda.synchronize()
    assert torch.isfinite(w.params).all() and w.loss_info()["grad_norm"] > 0


def test_two_workers_from_one_seed_end_with_equal_parameters(vit_sd):
    kw = dict(loss="ppo+imitation", num_mini_batch=2, sync_actions=True, update_repeats=2)
    a, b = _worker(vit_sd, **kw), _worker(vit_sd, **kw)
    for w in (a, b):
        w.iteration()
        w.iteration()
    torch.cuda.synchronize()
    assert torch.equal(a.params, b.params) and torch.equal(a.actions, b.actions) and torch.equal(a.h, b.h)
    assert torch.equal(a.feat, b.feat)


def test_evaluator_takes_the_workers_actions(vit_sd, tmp_path):
    """with equal weights, seed and env the Evaluator's first chunk selects what the Worker's first rollout selected"""
    from embodied_clip_amd.evaluate import Evaluator
    w = _worker(vit_sd)
    path = str(tmp_path / "w.pt")
    w.save_checkpoint(path)
    w.collect_rollout()
    ev = Evaluator(N, T=T, device=DEV, seed=3, encoder_sd=vit_sd, checkpoint=path, record=True, prev_action_null_token=True, **AGENT)
    info = ev.run(1)
    torch.cuda.synchronize()
    assert torch.equal(ev.actions, w.actions) and torch.equal(ev.logp, w.logp) and "episodes" in info


def test_refusals_before_any_allocation():
    from embodied_clip_amd.engine import Worker
    from embodied_clip_amd.evaluate import Evaluator
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    for cls in (Worker, Evaluator):
        for bad in (dict(encoder="rn50", pooling="cls"), dict(encoder="imagenet_rn18", pooling="cls"), dict(encoder="vit", pooling="attnpool"),
                    dict(encoder="vit", pooling="avgpool"), dict(encoder="vit"), dict(encoder="vit", pooling="cls", depth=True),
                    dict(encoder="vit", pooling="cls", zeroshot=True), dict(encoder="vit", pooling="cls", goal_in=2)):
            with pytest.raises(ValueError):
                cls(N, T=T, device=DEV, **{**dict(net="pooled"), **bad})
        with pytest.raises(ValueError):
            cls(N, T=T, device=DEV, encoder="vit", pooling="cls", net="two_view")
    assert torch.cuda.memory_allocated() == before

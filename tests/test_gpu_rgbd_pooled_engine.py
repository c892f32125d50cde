"""GPU: the pooled net on RGB-D frames through the engine -- ``Worker(net="pooled", pooling="avgpool", depth=True, ...)``, the
``Evaluator`` and checkpoints -- at N = 4 actors, T = 3.  The stored embeddings are held to the fp32 oracle's
``mean_hw(rgb_map + depth_map)`` on the env's own frames (the encoder tolerance, rel-L2 < 2e-2; two of the T + 1 steps, which
keeps the CPU oracle at 16 forwards), and everything behind the embedding to the float64 reference of tests/_pooled_net_ref.py
replayed on the worker's recorded rollout, within the bounds ``tests/test_gpu_pooled_net_engine.py`` holds the RGB agent to."""
import functools
import os
import sys
import types

import pytest
import torch

from embodied_clip_amd import synthetic as syn
from oracle import clip_resnet as ocr

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _pooled_net_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T, N, D = 3, 4, 2048
RGBD = dict(net="pooled", pooling="avgpool", depth=True)
AGENT = dict(RGBD, sensors=(2, 2), goal_ids=True, rnn_type="LSTM", rnn_layers=2, prev_actions=32)


@functools.lru_cache(maxsize=None)
def _enc_sd():
    return syn.rn50_visual_state_dict(0)


def _worker(**kw):
    from embodied_clip_amd.engine import Worker
    args = dict(AGENT, update_repeats=1, encoder_sd=_enc_sd())
    args.update(kw)
    return Worker(N, T=T, device=DEV, seed=3, **args)


def test_worker_against_the_oracle_and_the_reference_replay():
    w = _worker()
    assert w.feat.dtype == torch.float32 and tuple(w.feat.shape) == (T + 1, N, 1, D) and w.feat2 is None
    assert w.slices[0].feat2 is None and w.policy.pooled_cfg["embed_in"] == D and not w.dual and w.depth
    sd = {k: v.detach().cpu().clone() for k, v in w.policy.views(w.params).items()}
    w.collect_rollout()
    w.compute_returns()
    torch.cuda.synchronize()
    cpu = lambda t: t.detach().cpu()
    # the stored embeddings of the first and the last step against the oracle on the env's frames (step t reads pool entry t)
    for t in (0, T):
        rgb, dep = cpu(w.env.observe_at(t)), cpu(w.env.observe_depth_at(t))
        want = (ocr.clip_resnet_preprocessor(rgb, _enc_sd()) + ocr.clip_resnet_preprocessor(dep, _enc_sd())).double().flatten(2).mean(2)
        e = ref.rel_l2(w.feat[t].reshape(N, D), want)
        print(f"step {t}: stored embedding vs oracle mean_hw(rgb_map + depth_map): rel-L2 = {float(e):.3e}")
        assert e < 2e-2, (t, e)
    case = (T, N, D, 512, 12, (2, 2), 32, 1, 6, 2, ref.LSTM)
    batch = dict(embed=cpu(w.feat[:T]).reshape(T, N, D), goal=cpu(w.env.goals[:T]), sensors=cpu(w.env.sensors[:T]),
                 prev_actions=cpu(w.prev_actions[:T]), state0=cpu(w.h_start), masks=cpu(w.env.masks[:T]).unsqueeze(-1),
                 actions=cpu(w.actions), old_log_probs=cpu(w.logp).unsqueeze(-1), old_values=cpu(w.values[:T]).unsqueeze(-1),
                 returns=cpu(w.returns[:T]).unsqueeze(-1), norm_adv=cpu(w.nadv).unsqueeze(-1))
    assert float(batch["embed"].abs().max()) > 0
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
    print("gradient rel-L2:", errs)
    for k, e in errs.items():
        assert float(r["grads"][k].abs().max()) > 0 and e <= ref.GRAD_TOL, (k, e)


def test_the_depth_frames_are_read():
    a, b = _worker(), _worker()
    b.env.depth.copy_(b.env.depth.roll(shifts=1, dims=1))       # every actor sees its neighbour's depth frames from step 1 on
    for w in (a, b):
        w.collect_rollout()
    torch.cuda.synchronize()
    assert torch.equal(a.feat[0], b.feat[0])                    # (encoded by the constructors, from equal frames)
    for t in range(1, T + 1):
        assert not torch.equal(a.feat[t], b.feat[t]), t
    assert torch.equal(a.env.goals, b.env.goals) and torch.equal(a.env.masks, b.env.masks) and torch.equal(a.env.frames, b.env.frames)
    for w in (a, b):
        w.compute_returns(); w.update(); w.after_update()
    assert a.total_steps == b.total_steps == T * N


def test_two_workers_from_one_seed_end_with_equal_parameters():
    kw = dict(loss="ppo+imitation", num_mini_batch=2, sync_actions=True)
    a, b = _worker(**kw), _worker(**kw)
    p0 = a.params.clone()
    for w in (a, b):
        w.iteration()
        w.iteration()
    torch.cuda.synchronize()
    assert torch.equal(a.params, b.params) and torch.equal(a.actions, b.actions) and torch.equal(a.feat, b.feat)
    assert not torch.equal(a.params, p0)


def test_uint8_rgb_frames():
    w = _worker(frames_u8=True)
    assert w.env.frames.dtype == torch.uint8 and w.env.depth.dtype == torch.float32
    p0 = w.params.clone()
    w.iteration()
    torch.cuda.synchronize()
    assert torch.isfinite(w.params).all() and not torch.equal(w.params, p0) and w.loss_info()["grad_norm"] > 0
    assert torch.isfinite(w.feat).all() and float(w.feat.abs().max()) > 0


def test_checkpoint_is_the_rgb_avgpool_nets(tmp_path):
    w = _worker()
    w.iteration()
    path = str(tmp_path / "rgbd_pooled.pt")
    w.save_checkpoint(path)
    rgb_only = _worker(depth=False)
    assert list(rgb_only.policy.offsets) == list(w.policy.offsets) and not torch.equal(rgb_only.params, w.params)
    rgb_only.load_checkpoint(path)
    assert torch.equal(rgb_only.params, w.params) and rgb_only.total_steps == w.total_steps
    back = str(tmp_path / "rgb_pooled.pt")
    rgb_only.iteration()
    rgb_only.save_checkpoint(back)
    w.load_checkpoint(back)
    assert torch.equal(w.params, rgb_only.params)
    # a goal-encoder checkpoint is refused by tensor name
    other = str(tmp_path / "goal_encoder.pt")
    torch.save({"model_state_dict": syn.policy_state_dict(0), "optimizer_state_dict": {}, "total_steps": 0}, other)
    with pytest.raises(KeyError, match="visual_fc.1.weight"):
        w.load_checkpoint(other)


def test_evaluator_takes_the_workers_actions(tmp_path):
    from embodied_clip_amd.evaluate import Evaluator
    w = _worker()
    path = str(tmp_path / "w.pt")
    w.save_checkpoint(path)
    w.collect_rollout()
    ev = Evaluator(N, T=T, device=DEV, seed=3, encoder_sd=_enc_sd(), checkpoint=path, record=True, **AGENT)
    assert ev.slices[0].feat2 is None and tuple(ev.slices[0].feat.shape) == (2, N, 1, D)
    info = ev.run(1)
    torch.cuda.synchronize()
    assert torch.equal(ev.actions, w.actions) and torch.equal(ev.logp, w.logp) and "episodes" in info
    ev2 = Evaluator(N, T=T, device=DEV, seed=3, encoder_sd=_enc_sd(), checkpoint=path, deterministic=True, record=True, **AGENT)
    ev2.run(1)
    torch.cuda.synchronize()
    assert torch.equal(ev2.actions, ev2.hv[..., :6].argmax(-1))


def test_refusals_before_any_allocation():
    from embodied_clip_amd.engine import Worker
    from embodied_clip_amd.evaluate import Evaluator
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    host_env = types.SimpleNamespace(host=True, depth=object(), sensors=object(), N=N, T=T)      # how an Evaluator meets host-resident frames
    bad_w = (dict(pooling="attnpool"), dict(encoder="imagenet_rn18"), dict(frames_host=True), dict(zeroshot=True))
    bad_e = (dict(pooling="attnpool"), dict(encoder="imagenet_rn18"), dict(env=host_env), dict(zeroshot=True))
    for cls, bads in ((Worker, bad_w), (Evaluator, bad_e)):
        for bad in bads:
            with pytest.raises(ValueError):
                cls(N, T=T, device=DEV, **{**AGENT, **bad})
    assert torch.cuda.memory_allocated() == before

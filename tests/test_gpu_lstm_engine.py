"""GPU: the LSTM core through the engine -- ``Worker(rnn_type="LSTM")``, the ``Evaluator``, checkpoints and the plugin class -- at
8 actors and a rollout of 8 steps.  The recurrent memory everywhere is ``[N, 2H]`` rows ``[h | c]``; the act steps are replayed
on the worker's own features against tests/_lstm_ref.py (tolerance: ``test_worker_iteration_matches_oracle``'s)."""
import os
import sys

import pytest
import torch

from embodied_clip_amd import synthetic as syn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _lstm_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T, N, R = 8, 8, 2
AGENTS = [
    dict(),                                                        # the ObjectNav agent
    dict(goal_in=2, num_actions=4, prev_actions=6),                # PointNav goals with previous actions
    dict(num_actions=84, loss="ppo+imitation"),                    # a wide action space, PPO + imitation
]


def _rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-20)).item()


def _pkw(kw):
    p = {k: kw[k] for k in ("goal_in", "num_actions") if k in kw}
    if kw.get("prev_actions"):
        p.update(prev_action_dims=kw["prev_actions"], prev_action_null=1)
    return p


def _worker(rnn_type="LSTM", pol_sd=None, **kw):
    from embodied_clip_amd.engine import Worker
    if pol_sd is None:
        pol_sd = syn.policy_state_dict(0, **_pkw(kw), rnn_type=rnn_type)
    return Worker(N, T=T, device=DEV, seed=3, update_repeats=R, encoder_sd=syn.rn50_visual_state_dict(0), policy_sd=pol_sd,
                  rnn_type=rnn_type, **kw), pol_sd


@pytest.mark.parametrize("kw", AGENTS)
def test_worker_trains_and_is_reproducible(kw):
    """two iterations: finite losses, parameters that move (the 4H-row recurrent tensors among them), and a second worker from
    the same seed ends with the same parameters, bit for bit"""
    w, pol_sd = _worker(**kw)
    H = w.H
    assert w.policy.rnn_type == "LSTM" and w.SW == 2 * H and w.h.shape == w.h_next.shape == w.h_start.shape == (N, 2 * H)
    assert w.policy.shapes[ref.WHH] == (4 * H, H)
    before = w.params.clone()
    for _ in range(2):
        w.iteration()
        torch.cuda.synchronize()
        info = w.loss_info()
        assert all(v == v and abs(v) != float("inf") for v in info.values()), info
    assert torch.isfinite(w.params).all() and torch.isfinite(w.h).all()
    assert float(w.h[:, H:].abs().max()) > 0                              # the cell half of the memory is live
    pv, p0 = w.policy.views(w.params), w.policy.views(before)
    for name in (ref.WIH, ref.WHH, ref.BIH, ref.BHH, "actor.linear.weight"):
        assert not torch.equal(pv[name], p0[name]), name
    w2, _ = _worker(pol_sd=pol_sd, **kw)
    w2.iteration()
    w2.iteration()
    torch.cuda.synchronize()
    assert torch.equal(w2.params, w.params) and torch.equal(w2.actions, w.actions) and torch.equal(w2.h, w.h)


def test_act_steps_match_the_reference_replayed_on_the_workers_features():
    w, pol_sd = _worker()
    w.collect_rollout()
    torch.cuda.synchronize()
    S, C, H = w.S, w.C, w.H
    feat = w.feat.float().cpu().view(T + 1, N, S, S, C).permute(0, 1, 4, 2, 3).contiguous()
    masks, goals, actions = w.env.masks.cpu().unsqueeze(-1), w.env.goals.cpu(), w.actions.cpu()
    from oracle import policy as opol
    state = torch.zeros(1, N, 2 * H)
    vals, lps = [], []
    with torch.no_grad():
        for t in range(T + 1):
            lg, v, s2 = ref.actor_critic_forward(feat[t][None], goals[t][None], None, state, masks[t][None], pol_sd, 0)
            vals.append(v[0])
            if t < T:
                lps.append(opol.categorical_log_prob(lg, actions[t][None])[0])
                state = s2
    assert _rel(w.values.unsqueeze(-1), torch.stack(vals)) < 1e-4
    assert (w.logp.cpu() - torch.stack(lps)).abs().max() < 1e-4
    # (the two memory buffers ping-pong by step parity: one of them holds the state behind step T - 1)
    assert min(_rel(w.h, state[0]), _rel(w.h_next, state[0])) < 1e-4


def test_checkpoint_round_trip(tmp_path):
    from embodied_clip_amd.evaluate import Evaluator
    kw = dict(goal_in=2, num_actions=4, prev_actions=6)
    a, pol_sd = _worker(**kw)
    a.iteration()
    path = str(tmp_path / "lstm.pt")
    a.save_checkpoint(path)
    a.iteration()
    torch.cuda.synchronize()
    ck = torch.load(path, map_location="cpu")
    H = a.H
    assert tuple(ck["model_state_dict"][ref.WIH].shape) == (4 * H, 32 * 49 + 6) and tuple(ck["model_state_dict"][ref.BHH].shape) == (4 * H,)
    # save -> load -> one more iteration == the uninterrupted run (the second worker has the first one's env position and memory)
    b, _ = _worker(pol_sd=pol_sd, **kw)
    b.iteration()
    b.load_checkpoint(path)
    b.iteration()
    torch.cuda.synchronize()
    assert torch.equal(b.params, a.params) and b.total_steps == a.total_steps and torch.equal(b.opt.m, a.opt.m)
    # a fresh worker and an evaluator take the checkpoint's tensors
    c, _ = _worker(**kw)
    c.load_checkpoint(path)
    assert torch.equal(c.policy.views(c.params)[ref.WHH].cpu(), ck["model_state_dict"][ref.WHH])
    ev = Evaluator(N, T=T, device=DEV, seed=3, encoder_sd=syn.rn50_visual_state_dict(0), checkpoint=path, rnn_type="LSTM", **kw)
    assert torch.equal(ev.params, c.params) and ev.h.shape == (N, 2 * H)


def test_checkpoint_of_the_other_cell_and_unbuilt_agents_are_refused(tmp_path):
    from embodied_clip_amd.engine import Worker
    from embodied_clip_amd.evaluate import Evaluator
    kw = dict(goal_in=2, num_actions=4, prev_actions=6)
    c, _ = _worker(**kw)
    H = c.H
    path = str(tmp_path / "lstm.pt")
    c.save_checkpoint(path)
    # a GRU checkpoint into an LSTM worker (and the reverse): refused, naming the tensor, both shapes and the file
    g, _ = _worker(rnn_type="GRU", **kw)
    old = str(tmp_path / "gru.pt")
    g.save_checkpoint(old)
    with pytest.raises(ValueError) as e:
        c.load_checkpoint(old)
    msg = str(e.value)
    assert ref.WIH in msg and str((3 * H, 32 * 49 + 6)) in msg and str((4 * H, 32 * 49 + 6)) in msg and old in msg
    with pytest.raises(ValueError, match="weight_ih_l0"):
        g.load_checkpoint(path)
    with pytest.raises(ValueError, match="weight_ih_l0"):
        Evaluator(N, T=T, device=DEV, seed=3, encoder_sd=syn.rn50_visual_state_dict(0), checkpoint=old, rnn_type="LSTM", **kw)
    # refused before anything is allocated
    for bad in (dict(depth=True), dict(zeroshot=True)):
        with pytest.raises(ValueError, match="rnn_type"):
            Worker(N, T=T, device=DEV, rnn_type="LSTM", **bad)
        with pytest.raises(ValueError, match="rnn_type"):
            Evaluator(N, T=T, device=DEV, rnn_type="LSTM", **bad)
    with pytest.raises(ValueError, match="rnn_type"):
        Worker(N, T=T, device=DEV, rnn_type="RNN")


def test_evaluator_runs_a_chunk_and_equals_the_handle_level_act_loop():
    from embodied_clip_amd.evaluate import Evaluator
    pol_sd = syn.policy_state_dict(0, rnn_type="LSTM")
    ev = Evaluator(N, T=T, device=DEV, seed=3, encoder_sd=syn.rn50_visual_state_dict(0), policy_sd=pol_sd, record=True, deterministic=True,
                   rnn_type="LSTM")
    info = ev.run(1)
    assert info and all(v == v for v in info.values() if isinstance(v, float))
    w, _ = _worker(pol_sd=pol_sd)
    w.collect_rollout()
    torch.cuda.synchronize()
    pol, flat = w.policy, w.params
    ws = torch.empty(pol.workspace_bytes(1, N, False), dtype=torch.uint8, device=DEV)
    h = torch.zeros(N, 2 * w.H, device=DEV)
    for t in range(T):
        hv, hf = torch.empty(N, 7, device=DEV), torch.empty(N, 2 * w.H, device=DEV)
        act, lp, v = torch.zeros(N, dtype=torch.int64, device=DEV), torch.zeros(N, device=DEV), torch.zeros(N, device=DEV)
        pol.act(flat, w.feat[t].contiguous(), w.env.goals[t].contiguous(), h, w.env.masks[t].contiguous(), N, ws, hv, hf, act, lp, v,
                deterministic=True)
        torch.cuda.synchronize()
        assert torch.equal(ev.actions[t], act) and torch.equal(ev.logp[t], lp) and torch.equal(ev.hv[t], hv), t
        h = hf


def test_plugin_class_on_upstream_memory():
    """``ResnetTensorObjectNavActorCritic(rnn_type="LSTM")``: ``num_recurrent_layers == 2``, memory ``[2, N, H]`` in and out; its
    forward + ``backward()`` equal the reference (and so the raw handle, which tests/test_gpu_lstm.py holds to the same reference)."""
    from embodied_clip_amd import spaces
    from embodied_clip_amd.policy import Memory, PolicyHandle, ResnetTensorObjectNavActorCritic, ResnetTensorPointNavActorCritic
    from embodied_clip_amd.ppo import PPO
    case = ref.POLICY_CASES[1]
    Tc, Nc, H, A = case[0], case[1], case[4], case[7]
    cfg, sd, batch = ref.policy_inputs(*case)
    r = ref.policy_reference(sd, batch, 0)
    b = r["batch"]
    obs_space = spaces.Dict({"rgb_clip_resnet": spaces.Box(-1e9, 1e9, (64, 7, 7)), "goal_object_type_ind": spaces.Discrete(12)})
    mk = lambda **kw: ResnetTensorObjectNavActorCritic(spaces.Discrete(A), obs_space, "goal_object_type_ind", "rgb_clip_resnet",
                                                       hidden_size=H, device=DEV, **kw)
    model = mk(rnn_type="LSTM")
    assert model.num_recurrent_layers == 2 and model.recurrent_hidden_state_size == H
    spec = model._recurrent_memory_specification()["rnn"][0]
    assert spec[0] == ("layer", 2) and spec[2] == ("hidden", H)
    assert [n for n, _ in model.named_parameters()] == list(syn.policy_param_order())
    assert tuple(model.state_encoder.rnn.weight_hh_l0.shape) == (4 * H, H)
    model.load_state_dict(sd)
    obs = {"rgb_clip_resnet": b["feat"].to(DEV), "goal_object_type_ind": b["goal"].to(DEV)}
    mem0 = ref.state_to_memory(b["h0"][0]).to(DEV)                        # upstream's [2, N, H]
    out, mem2 = model(obs, Memory().check_append("rnn", mem0, 1), None, b["masks"].to(DEV))
    assert tuple(mem2.tensor("rnn").shape) == (2, Nc, H)
    assert _rel(out.distributions.logits, torch.log_softmax(r["logits"], -1)) < 2e-5 and _rel(out.values, r["values"]) < 2e-5
    assert _rel(mem2.tensor("rnn"), ref.state_to_memory(r["h"][0])) < 2e-5
    pb = dict(actions=b["actions"].to(DEV), old_action_log_probs=b["old_log_probs"].to(DEV), values=b["old_values"].to(DEV),
              returns=b["returns"].to(DEV), norm_adv_targ=b["norm_adv"].to(DEV), adv_targ=b["norm_adv"].to(DEV))
    total, _ = PPO().loss(0, pb, out)
    total.backward()
    assert abs(float(total.detach()) - r["info"]["ppo_total"]) < 1e-5 * max(1.0, abs(r["info"]["ppo_total"]))
    # the raw handle on the same inputs: the same hv and gradients, bit for bit
    hd = PolicyHandle(rnn_type="LSTM", **cfg)
    flat = hd.flatten(sd, DEV)
    rows = b["feat"].permute(0, 1, 3, 4, 2).reshape(Tc * Nc, 49, 64).contiguous().to(DEV)
    ws = torch.empty(hd.workspace_bytes(Tc, Nc, True), dtype=torch.uint8, device=DEV)
    m = b["masks"].reshape(-1).to(DEV)
    hv, hf = hd.forward(flat, rows, b["goal"].reshape(-1).to(DEV), b["h0"][0].contiguous().to(DEV), m, Tc, Nc, ws)
    assert torch.equal(hv.view(Tc, Nc, -1)[..., A:], out.values.detach()) and torch.equal(ref.state_to_memory(hf), mem2.tensor("rnn").detach())
    for n, p in model.named_parameters():
        assert p.grad is not None and _rel(p.grad, r["ref_grads"][n]) < 2e-4, n
    # the no-grad act route, and the refusals of the constructor
    with torch.no_grad():
        out2, mem3 = model(obs, Memory().check_append("rnn", mem0, 1), None, b["masks"].to(DEV))
    assert _rel(out2.values, r["values"]) < 2e-5 and tuple(mem3.tensor("rnn").shape) == (2, Nc, H)
    assert mk().num_recurrent_layers == 1 and mk(rnn_type="GRU", num_rnn_layers=1).rnn_type == "GRU"
    with pytest.raises(NotImplementedError):
        mk(rnn_type="LSTM", num_rnn_layers=2)
    with pytest.raises(NotImplementedError):
        mk(num_rnn_layers=2)
    dspace = spaces.Dict({"rgb_clip_resnet": spaces.Box(-1e9, 1e9, (64, 7, 7)), "depth_clip_resnet": spaces.Box(-1e9, 1e9, (64, 7, 7)),
                          "goal_object_type_ind": spaces.Discrete(12)})
    with pytest.raises(NotImplementedError):
        ResnetTensorObjectNavActorCritic(spaces.Discrete(A), dspace, "goal_object_type_ind", "rgb_clip_resnet", "depth_clip_resnet",
                                         hidden_size=H, device=DEV, rnn_type="LSTM")
    pspace = spaces.Dict({"rgb_clip_resnet": spaces.Box(-1e9, 1e9, (64, 7, 7)), "target_coordinates_ind": spaces.Box(-1e9, 1e9, (2,))})
    pn = ResnetTensorPointNavActorCritic(spaces.Discrete(4), pspace, "target_coordinates_ind", "rgb_clip_resnet", hidden_size=H,
                                         device=DEV, rnn_type="LSTM")
    assert pn.num_recurrent_layers == 2 and tuple(pn.state_encoder.rnn.bias_ih_l0.shape) == (4 * H,)

"""GPU: the PointNav agent (coordinate goals, ``goal_in > 0``) against the CPU restatement in tests/_pointnav_ref.py.

Tolerances are the policy path's own (test_gpu_policy.py): forward rel-L2 < 2e-5, per-tensor gradient rel-L2 < 2e-4, the Adam
update as in ``test_policy_backward_and_update_step_match_oracle``.  The fp32 torch reference agrees with its float64 self to
<= 1.6e-6 (forward) and <= 3.1e-6 (worst gradient tensor) at these shapes, so the bounds test the kernels.

Cases are (T, N, S, C, H, goal_in, A, bf16 features):
  (1, 1, 7, ...)        one frame
  (3, 5, 7, ...)        the fused tail: 735 rows, ragged last tile, every frame straddling 32-row tiles
  (4, 37, 7, .., 3, ..) bf16 features, 7,252 rows, goal_in = 3
  (6, 4, 3, .., A = 6)  S*S = 9 < 32: the GEMM route (per-frame bias through ec_gemm_f32's row-group bias, frame sums off dm1)
  (3, 5, 7, .., 1, ..)  goal_in = 1
  (2, 16, 7, H = 512)   the 512-wide recurrence kernels;  (3, 19, 7, C = 256) bf16: the transpose-read dW1 route
"""
import functools
import os
import sys

import pytest
import torch

from embodied_clip_amd import synthetic as syn
from oracle import policy as opol
from oracle import ppo as oppo

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _pointnav_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

FWD_CASES = [(1, 1, 7, 64, 32, 2, 4, False), (3, 5, 7, 64, 32, 2, 4, False), (4, 37, 7, 64, 32, 3, 4, True),
             (6, 4, 3, 64, 32, 2, 6, False), (3, 5, 7, 64, 32, 1, 4, False)]
STEP_CASES = FWD_CASES + [(2, 16, 7, 64, 512, 2, 4, True), (3, 19, 7, 256, 32, 2, 4, True)]
EDGE = (3, 5, 7, 64, 32, 2, 4, False)


def _rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-20)).item()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _case(T, N, S, C, H, goal_in, A, bf16, goals="random"):
    """Inputs and the reference's forward / optimiser step, computed once per case and shared (never modified)."""
    cfg = dict(in_channels=C, spatial=S, hidden=H, goal_in=goal_in, num_actions=A)
    sd = syn.policy_state_dict(7, **cfg)
    g = torch.Generator().manual_seed(8)
    feat = torch.randn(T, N, C, S, S, generator=g).abs()       # post-ReLU features are non-negative
    if bf16:
        feat = feat.to(torch.bfloat16).float()
    goal = syn.synthetic_goal_vectors(9, (T, N), goal_in, rho_max=30.0)
    if goals == "zero":
        goal = torch.zeros_like(goal)
    elif goals == "shared":
        goal = goal[:1, :1].expand(T, N, goal_in).contiguous()
    h0 = torch.randn(1, N, H, generator=g) * 0.5
    masks = syn.synthetic_masks(10, T, N, p_reset=0.2)
    with torch.no_grad():
        lg, vv, hf = ref.actor_critic_forward(feat, goal, h0, masks, sd)
    actions = torch.randint(0, A, (T, N), generator=g)
    old_lp = opol.categorical_log_prob(lg, actions).unsqueeze(-1) + 0.2 * torch.randn(T, N, 1, generator=g)
    old_v = vv + 0.2 * torch.randn(T, N, 1, generator=g)
    returns, nadv = torch.randn(T, N, 1, generator=g), torch.randn(T, N, 1, generator=g)
    batch = dict(feat=feat, goal=goal, h0=h0, masks=masks, actions=actions, old_log_probs=old_lp, old_values=old_v,
                 returns=returns, norm_adv=nadv)
    sd_ref = {k: v.clone() for k, v in sd.items()}
    with ref.as_oracle_policy():
        info, ref_grads = oppo.ppo_update_step(sd_ref, batch, {}, lr=3e-4, max_grad_norm=0.5)
    return dict(cfg=cfg, sd=sd, batch=batch, logits=lg, values=vv, h=hf, info=info, ref_grads=ref_grads, sd_ref=sd_ref)


def _gpu_inputs(c, dev, bf16):
    b, cfg = c["batch"], c["cfg"]
    T, N = b["feat"].shape[:2]
    rows = b["feat"].permute(0, 1, 3, 4, 2).reshape(T * N, cfg["spatial"] ** 2, cfg["in_channels"]).contiguous()
    rows = (rows.to(torch.bfloat16) if bf16 else rows).to(dev)
    goal = b["goal"].reshape(T * N, cfg["goal_in"]).contiguous().to(dev)
    return rows, goal, b["h0"][0].contiguous().to(dev), b["masks"].reshape(-1).to(dev)


def _learn_step(c, dev, bf16):
    """forward (learn plan), PPO loss, backward on the GPU -> (handle, flat, hv, sums, grads)"""
    from embodied_clip_amd import ppo
    from embodied_clip_amd.policy import PolicyHandle
    b, cfg = c["batch"], c["cfg"]
    T, N = b["feat"].shape[:2]
    h = PolicyHandle(**cfg)
    flat = h.flatten(c["sd"], dev)
    rows, goal, h0, m = _gpu_inputs(c, dev, bf16)
    ws = torch.empty(h.workspace_bytes(T, N, True), dtype=torch.uint8, device=dev)
    hv, _ = h.forward(flat, rows, goal, h0, m, T, N, ws)
    f = lambda t: t.reshape(-1).contiguous().to(dev)
    dhv, sums = ppo.ppo_loss_raw(hv, f(b["actions"]), f(b["old_log_probs"]), f(b["old_values"]), f(b["returns"]),
                                 f(b["norm_adv"]), cfg["num_actions"])
    grads = torch.zeros_like(flat)
    h.backward(flat, rows, m, T, N, ws, dhv, None, grads)
    again = torch.zeros_like(flat)                       # the same backward once more (reads the same workspace)
    h.backward(flat, rows, m, T, N, ws, dhv, None, again)
    torch.cuda.synchronize()
    return h, flat, hv, sums, grads, again


@pytest.mark.parametrize("T,N,S,C,H,goal_in,A,bf16", FWD_CASES)
def test_pointnav_forward_matches_reference(dev, T, N, S, C, H, goal_in, A, bf16):
    from embodied_clip_amd.policy import PolicyHandle
    c = _case(T, N, S, C, H, goal_in, A, bf16)
    h = PolicyHandle(**c["cfg"])
    assert len(h.offsets) == 18
    flat = h.flatten(c["sd"], dev)
    rows, goal, h0, m = _gpu_inputs(c, dev, bf16)
    ws = torch.empty(h.workspace_bytes(T, N, False), dtype=torch.uint8, device=dev)
    hv, hf = h.forward(flat, rows, goal, h0, m, T, N, ws, for_backward=False)
    torch.cuda.synchronize()
    hv = hv.view(T, N, -1)
    errs = (_rel(hv[..., :A], c["logits"]), _rel(hv[..., A:], c["values"]), _rel(hf, c["h"][0]))
    print("forward rel-L2 (logits, values, h):", errs)
    assert max(errs) < 2e-5, errs


@pytest.mark.parametrize("T,N,S,C,H,goal_in,A,bf16", STEP_CASES)
def test_pointnav_optimiser_step_matches_reference(dev, T, N, S, C, H, goal_in, A, bf16):
    """forward, PPO loss, backward, clip, Adam: all 18 gradients and the parameter update."""
    from embodied_clip_amd import ppo
    c = _case(T, N, S, C, H, goal_in, A, bf16)
    info, ref_grads, sd, sd_ref = c["info"], c["ref_grads"], c["sd"], c["sd_ref"]
    h, flat, hv, sums, grads, _ = _learn_step(c, dev, bf16)
    hv3 = hv.view(T, N, -1)
    assert _rel(hv3[..., :A], c["logits"]) < 2e-5 and _rel(hv3[..., A:], c["values"]) < 2e-5      # the learn plan's forward
    total = ((sums[0] + 0.5 * sums[1] + 0.01 * sums[2]) / (T * N)).item()
    assert abs(total - info["ppo_total"]) < 1e-5 * max(1.0, abs(info["ppo_total"]))
    gv = h.views(grads)
    assert len(ref_grads) == 18 and set(gv) == set(ref_grads)
    errs = {name: _rel(gv[name], gref) for name, gref in ref_grads.items()}
    print("gradient rel-L2:", errs)
    for name, e in errs.items():
        assert e < 2e-4, (name, e)
    opt = ppo.FlatAdam(flat, lr=3e-4, max_grad_norm=0.5)
    opt.step(grads)
    torch.cuda.synchronize()
    assert abs(opt.grad_norm() - info["grad_norm"]) < 1e-4 * info["grad_norm"]
    pv = h.views(flat)
    for name, pref in sd_ref.items():
        # (the update, not the parameter: see test_policy_backward_and_update_step_match_oracle)
        upd, upd_ref = pv[name].cpu() - sd[name], pref - sd[name]
        well = ref_grads[name].abs() > 1e-6
        assert ((upd - upd_ref).abs() * well).max() < 0.05 * 3e-4 + 1e-7, name
        assert upd.abs().max() <= 3e-4 * 1.001 + 1e-7, name


def test_pointnav_zero_goal_vectors(dev):
    """All goal vectors zero: dWc = dEg^T goal_vec is exactly 0; embed_goal.bias still gets its gradient."""
    c = _case(*EDGE, goals="zero")
    h, _, _, _, grads, _ = _learn_step(c, dev, False)
    gv = h.views(grads)
    w = gv["goal_visual_encoder.embed_goal.weight"]
    assert torch.equal(w, torch.zeros_like(w))
    bname = "goal_visual_encoder.embed_goal.bias"
    assert float(c["ref_grads"][bname].abs().max()) > 0
    assert _rel(gv[bname], c["ref_grads"][bname]) < 2e-4
    for name, gref in c["ref_grads"].items():
        if name != "goal_visual_encoder.embed_goal.weight":
            assert _rel(gv[name], gref) < 2e-4, name


def test_pointnav_all_frames_share_one_goal(dev):
    c = _case(*EDGE, goals="shared")
    h, _, _, _, grads, _ = _learn_step(c, dev, False)
    gv = h.views(grads)
    for name, gref in c["ref_grads"].items():
        assert _rel(gv[name], gref) < 2e-4, (name, _rel(gv[name], gref))


@pytest.mark.parametrize("case", [(3, 5, 7, 64, 32, 2, 4, False), (6, 4, 3, 64, 32, 2, 6, False), (2, 16, 7, 64, 512, 2, 4, True)])
def test_pointnav_backward_is_deterministic(dev, case):
    """No float atomics on any goal_in > 0 route (fused tail, GEMM route, 512-wide recurrences): the same backward twice gives
    the same bits."""
    c = _case(*case)
    _, _, _, _, grads, again = _learn_step(c, dev, case[-1])
    assert float(grads.abs().max()) > 0 and torch.equal(grads, again)


def test_pointnav_forward_does_not_depend_on_actor_slicing(dev):
    """The act step of 37 actors == the act steps of actors [0, 19) and [19, 37), bit for bit."""
    from embodied_clip_amd.policy import PolicyHandle
    c = _case(1, 37, 7, 64, 32, 2, 4, True)
    h = PolicyHandle(**c["cfg"])
    flat = h.flatten(c["sd"], dev)
    rows, goal, h0, m = _gpu_inputs(c, dev, True)

    def run(a, b):
        n = b - a
        ws = torch.empty(h.workspace_bytes(1, n, False), dtype=torch.uint8, device=dev)
        return h.forward(flat, rows[a:b].contiguous(), goal[a:b].contiguous(), h0[a:b].contiguous(), m[a:b].contiguous(), 1, n, ws,
                         for_backward=False)
    hv, hf = run(0, 37)
    hv_a, hf_a = run(0, 19)
    hv_b, hf_b = run(19, 37)
    torch.cuda.synchronize()
    assert _rel(hv.view(1, 37, -1)[..., :4], c["logits"]) < 2e-5
    assert torch.equal(hv, torch.cat([hv_a, hv_b])) and torch.equal(hf, torch.cat([hf_a, hf_b]))


def test_pointnav_act_step_and_table_reuse(dev):
    """``ec_policy_act_vec`` == the vector forward + ``ec_sample_actions``, bit for bit.  A second step with ``reuse_tables`` and
    DIFFERENT goal vectors equals a fresh EC_POLICY_INFER call: the reused workspace holds weight-derived tables only and
    never replays the previous step's goals.  After a parameter change without a rebuild the results differ (the existing
    invalidation contract: the caller must drop ``reuse_tables``)."""
    from embodied_clip_amd import _lib
    from embodied_clip_amd.policy import PolicyHandle
    lib = _lib.load()
    N, A = 37, 4
    h = PolicyHandle(goal_in=2, num_actions=A)
    flat = h.flatten(syn.policy_state_dict(5, goal_in=2, num_actions=A), dev)
    g = torch.Generator().manual_seed(9)
    feat = (torch.randn(N, 49, 2048, generator=g).abs() * 0.5).to(torch.bfloat16).to(dev)
    goals = [syn.synthetic_goal_vectors(6 + k, (N,), 2, rho_max=30.0).to(dev) for k in range(2)]
    assert not torch.equal(goals[0], goals[1])
    h0 = (torch.randn(N, 512, generator=g) * 0.3).to(dev)
    m = (torch.rand(N, generator=g) > 0.2).float().to(dev)
    ws_a = torch.empty(h.workspace_bytes(1, N, False), dtype=torch.uint8, device=dev)
    ws_b = torch.empty_like(ws_a)
    hv_steps = []
    for call, reuse in enumerate((False, True)):
        goal = goals[call]
        hv_f, hf_f = h.forward(flat, feat, goal, h0, m, 1, N, torch.empty_like(ws_a), for_backward=False)     # fresh EC_POLICY_INFER
        hv_f, hf_f = hv_f.clone(), hf_f.clone()
        hv_a, hf_a = h.forward(flat, feat, goal, h0, m, 1, N, ws_a, for_backward=False, reuse_tables=reuse)
        act_a = torch.zeros(N, dtype=torch.int64, device=dev); lp_a = torch.zeros(N, device=dev); v_a = torch.zeros(N, device=dev)
        _lib.check(lib.ec_sample_actions(hv_a.data_ptr(), act_a.data_ptr(), lp_a.data_ptr(), v_a.data_ptr(), N, A, 123, 40 + call, 1000, 0))
        hv_b = torch.empty_like(hv_a); hf_b = torch.empty_like(hf_a)
        act_b = torch.zeros(N, dtype=torch.int64, device=dev); lp_b = torch.zeros(N, device=dev); v_b = torch.zeros(N, device=dev)
        h.act(flat, feat, goal, h0, m, N, ws_b, hv_b, hf_b, act_b, lp_b, v_b, 123, 40 + call, 1000, reuse_tables=reuse)
        torch.cuda.synchronize()
        assert torch.equal(hv_a, hv_f) and torch.equal(hf_a, hf_f)              # reuse with other goals == fresh call
        assert torch.equal(hv_a, hv_b) and torch.equal(hf_a, hf_b)
        assert torch.equal(act_a, act_b) and torch.equal(lp_a, lp_b) and torch.equal(v_a, v_b)
        assert len(set(act_a.tolist())) > 1 and (lp_a < 0).all() and int(act_a.max()) < A
        hv_steps.append(hv_b.clone())
    assert not torch.equal(hv_steps[0], hv_steps[1])                            # the goals matter
    # parameters change, tables are not rebuilt: stale weight-derived tables -> another result than a fresh call
    flat2 = flat.clone()
    flat2[h.offsets["state_encoder.rnn.weight_ih_l0"][0]:][:4096] += 0.05
    hv_stale, _ = h.forward(flat2, feat, goals[1], h0, m, 1, N, ws_a, for_backward=False, reuse_tables=True)
    hv_fresh, _ = h.forward(flat2, feat, goals[1], h0, m, 1, N, torch.empty_like(ws_a), for_backward=False)
    torch.cuda.synchronize()
    assert not torch.equal(hv_stale, hv_fresh)


def test_pointnav_module_autograd_surface(dev):
    """``ResnetTensorPointNavActorCritic``: names, goal observation [T, N, 2], autograd forward / backward against the reference,
    ``.grad`` views of the flat bucket, ``state_dict()`` round trip."""
    from embodied_clip_amd import spaces
    from embodied_clip_amd.policy import Memory, ResnetTensorPointNavActorCritic
    from embodied_clip_amd.ppo import PPO
    T, N, A = 4, 3, 4
    c = _case(T, N, 7, 64, 32, 2, A, False)
    b, sd = c["batch"], c["sd"]
    obs_space = spaces.Dict({"rgb_clip_resnet": spaces.Box(-1e9, 1e9, (64, 7, 7)),
                             "target_coordinates_ind": spaces.Box(-1e9, 1e9, (2,))})
    model = ResnetTensorPointNavActorCritic(spaces.Discrete(A), obs_space, "target_coordinates_ind", "rgb_clip_resnet",
                                            hidden_size=32, state_dict=sd, device=dev)
    assert [n for n, _ in model.named_parameters()] == list(syn.policy_param_order(goal_in=2))
    assert model.handle.goal_in == 2 and model.recurrent_hidden_state_size == 32 and not model.is_blind
    mem = Memory().check_append("rnn", b["h0"].to(dev), 1)
    assert b["goal"].shape == (T, N, 2)
    out, mem2 = model({"rgb_clip_resnet": b["feat"].to(dev), "target_coordinates_ind": b["goal"].to(dev)}, mem, None,
                      b["masks"].to(dev))
    assert _rel(out.distributions.logits, torch.log_softmax(c["logits"], -1)) < 2e-5 and _rel(out.values, c["values"]) < 2e-5
    assert _rel(mem2.tensor("rnn"), c["h"]) < 2e-5
    batch = dict(actions=b["actions"].to(dev), old_action_log_probs=b["old_log_probs"].to(dev), values=b["old_values"].to(dev),
                 returns=b["returns"].to(dev), norm_adv_targ=b["norm_adv"].to(dev), adv_targ=b["norm_adv"].to(dev))
    total, _ = PPO().loss(0, batch, out)
    total.backward()
    assert abs(float(total.detach()) - c["info"]["ppo_total"]) < 1e-5 * max(1.0, abs(c["info"]["ppo_total"]))
    views = model.handle.views(model.flat_grads)
    for n, p in model.named_parameters():
        assert p.grad is not None and _rel(p.grad, c["ref_grads"][n]) < 2e-4, n
        assert p.grad.data_ptr() == views[n].data_ptr()                      # .grad IS a view of the one flat bucket
    # state_dict round trip into a fresh module
    other = ResnetTensorPointNavActorCritic(spaces.Discrete(A), obs_space, "target_coordinates_ind", "rgb_clip_resnet",
                                            hidden_size=32, device=dev)
    assert not torch.equal(other.flat_params, model.flat_params)
    other.load_state_dict(model.state_dict())
    assert set(model.state_dict()) == set(sd) and torch.equal(other.flat_params, model.flat_params)
    with torch.no_grad():
        out2, _ = other({"rgb_clip_resnet": b["feat"].to(dev), "target_coordinates_ind": b["goal"].to(dev)},
                        Memory().check_append("rnn", b["h0"].to(dev), 1), None, b["masks"].to(dev))
    assert _rel(out2.values, c["values"]) < 2e-5


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


def test_pointnav_worker_iteration_matches_reference_and_is_reproducible():
    """``Worker(goal_in=2)``, 8 actors, T = 4: the act steps, GAE and the update's optimiser steps against the reference replayed
    on the worker's own features and actions (tolerances of ``test_worker_iteration_matches_oracle``); a second worker from
    the same seed ends with the same parameters, bit for bit."""
    from embodied_clip_amd.engine import Worker
    assert torch.cuda.is_available()
    T, N, R, A = 4, 8, 2, 4
    enc_sd, pol_sd = syn.rn50_visual_state_dict(0), syn.policy_state_dict(0, goal_in=2, num_actions=A)
    mk = lambda: Worker(N, T=T, device="cuda:0", seed=3, update_repeats=R, encoder_sd=enc_sd, policy_sd=pol_sd, goal_in=2,
                        num_actions=A)
    w = mk()
    assert w.env.goals.shape == (T + 1, N, 2) and w.env.goals.dtype == torch.float32 and w.A == A
    w.collect_rollout()
    w.compute_returns()
    torch.cuda.synchronize()
    S, C = w.S, w.C
    feat_gpu = w.feat.float().cpu().view(T + 1, N, S, S, C).permute(0, 1, 4, 2, 3).contiguous()   # [T+1,N,C,S,S]
    masks = w.env.masks.cpu().unsqueeze(-1)
    goals = w.env.goals.cpu()
    actions = w.actions.cpu()
    assert int(actions.min()) >= 0 and int(actions.max()) < A
    h = torch.zeros(1, N, w.H)
    vals, lps = [], []
    with torch.no_grad():
        for t in range(T + 1):
            lg, v, h2 = ref.actor_critic_forward(feat_gpu[t][None], goals[t][None], h, masks[t][None], pol_sd)
            vals.append(v[0])
            if t < T:
                lps.append(opol.categorical_log_prob(lg, actions[t][None])[0])
                h = h2
    vals, lps = torch.stack(vals), torch.stack(lps)
    assert _rel(w.values.unsqueeze(-1), vals) < 1e-4
    assert (w.logp.cpu() - lps).abs().max() < 1e-4
    rewards = w.env.rewards.cpu().unsqueeze(-1)
    Rr = oppo.compute_returns(rewards, vals, masks)
    _, nadv = oppo.normalized_advantages(Rr, vals)
    assert _rel(w.returns.unsqueeze(-1), Rr) < 1e-4
    assert _rel(w.nadv.unsqueeze(-1), nadv) < 1e-3
    sd_ref = {k: v.clone() for k, v in pol_sd.items()}
    batch = dict(feat=feat_gpu[:T], goal=goals[:T], h0=torch.zeros(1, N, w.H), masks=masks[:T], actions=actions,
                 old_log_probs=w.logp.cpu().unsqueeze(-1), old_values=w.values[:T].cpu().unsqueeze(-1),
                 returns=w.returns[:T].cpu().unsqueeze(-1), norm_adv=w.nadv.cpu().unsqueeze(-1))
    st, step_grads = {}, []
    with ref.as_oracle_policy():
        for _ in range(R):
            info, g_ = oppo.ppo_update_step(sd_ref, batch, st)
            step_grads.append(g_)
    w.update()
    torch.cuda.synchronize()
    got = w.loss_info()
    assert abs(got["ppo_total"] - info["ppo_total"]) < 2e-4 * max(1.0, abs(info["ppo_total"]))
    assert abs(got["grad_norm"] - info["grad_norm"]) < 2e-3 * info["grad_norm"]
    _check_updates(w.policy.views(w.params), pol_sd, sd_ref, step_grads, R)
    w.after_update()
    w2 = mk()
    w2.iteration()
    torch.cuda.synchronize()
    assert torch.equal(w2.actions, w.actions) and torch.equal(w2.params, w.params)

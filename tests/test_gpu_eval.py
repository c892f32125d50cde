"""Evaluation on the GPU: the episode bookkeeping kernel against the sequential reference, the greedy act step on every route
of the heads launch, ``Evaluator`` against the training rollout, the metrics through the engine, and checkpoints."""
import os
import sys

import numpy as np
import pytest
import torch

from embodied_clip_amd import synthetic as syn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _episode_ref as er  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ---- 1. ec_episode_stats ------------------------------------------------------------------------------------------------------

def _random_calls(T, N, p=0.3, calls=2):
    out = []
    for c in range(calls):
        ends = syn.hash_uniform(40 + c, T * N, stream=3).reshape(T, N) < p
        masks = np.ones((T + 1, N), dtype=np.float32)
        masks[1:][ends] = 0
        rewards = (syn.hash_uniform(50 + c, T * N, stream=4).reshape(T, N) * 2 - 1).astype(np.float32)
        success = ((syn.hash_uniform(60 + c, T * N, stream=5).reshape(T, N) < 0.5) & ends).astype(np.float32)
        out.append((rewards, masks, success))
    return out


def _run_tracker(dev, calls, N, cap):
    from embodied_clip_amd.episodes import EpisodeTracker
    tr = EpisodeTracker(N, dev, capacity=cap)
    for rewards, masks, success in calls:
        tr.update(torch.from_numpy(rewards).to(dev), torch.from_numpy(masks).to(dev), torch.from_numpy(success).to(dev))
    torch.cuda.synchronize()
    return tr


def _check_against_ref(tr, ref, cap):
    n, s, s2, ln, sc = ref.totals()
    abs_s, abs_s2 = ref.abs_sums()
    tot = tr.totals.tolist()
    print("totals", tot, "ref", (n, s, s2, ln, sc), "bounds", n * U * abs_s, n * U * abs_s2)
    assert tot[0] == n and tot[3] == ln and tot[4] == sc
    assert abs(tot[1] - s) <= n * U * abs_s          # an n-term double sum, in any order
    assert abs(tot[2] - s2) <= n * U * abs_s2
    assert int(tr.n_records.item()) == n             # advances past cap: the overflow is visible
    rec = tr.records()
    k = min(n, cap)
    assert rec["dropped"] == n - k
    want = ref.records[:k]
    assert torch.equal(rec["actor"].cpu(), torch.tensor([r[0] for r in want], dtype=torch.int32))
    assert torch.equal(rec["t"].cpu(), torch.tensor([r[1] for r in want], dtype=torch.int32))
    assert torch.equal(rec["length"].cpu(), torch.tensor([r[2] for r in want], dtype=torch.int32))
    assert torch.equal(rec["return"].cpu(), torch.tensor([r[3] for r in want], dtype=torch.float32))
    assert torch.equal(rec["success"].cpu(), torch.tensor([r[4] for r in want], dtype=torch.float32))
    assert torch.equal(tr.carry_ret.cpu(), torch.from_numpy(ref.carry_ret))
    assert torch.equal(tr.carry_len.cpu(), torch.from_numpy(ref.carry_len))


def test_episode_stats_hand_made_case(dev):
    calls = er.hand_case()
    ref = er.EpisodeRef(er.HAND_N)
    for c in calls:
        ref.update(*c)
    tr = _run_tracker(dev, calls, er.HAND_N, cap=16)
    _check_against_ref(tr, ref, 16)
    assert tr.records()["length"].tolist() == er.HAND_LENGTHS[0] + er.HAND_LENGTHS[1]
    assert tr.carry_len.tolist() == er.HAND_CARRY_LEN
    again = _run_tracker(dev, calls, er.HAND_N, cap=16)
    assert torch.equal(tr.totals, again.totals)
    # no success tensor counts as 0; no record buffers: totals and the count only
    bare = _run_tracker(dev, [(r, m, np.zeros_like(r)) for r, m, _ in calls], er.HAND_N, cap=0)
    from embodied_clip_amd.episodes import EpisodeTracker
    none = EpisodeTracker(er.HAND_N, dev)
    for r, m, _ in calls:
        none.update(torch.from_numpy(r).to(dev), torch.from_numpy(m).to(dev))
    assert torch.equal(bare.totals, none.totals) and none.totals[4].item() == 0 and int(none.n_records.item()) == 7
    tr.reset()
    assert tr.info()["episodes"] == 0 and np.isnan(tr.info()["reward"]) and tr.carry_len.tolist() == er.HAND_CARRY_LEN


@pytest.fixture(scope="module")
def wide_case():
    T, N = 3, 1030                              # more actors than one block of 1024
    calls = _random_calls(T, N)
    ref = er.EpisodeRef(N)
    for c in calls:
        ref.update(*c)
    return N, calls, ref


@pytest.mark.parametrize("cap", [2000, 100])
def test_episode_stats_more_actors_than_a_block(dev, wide_case, cap):
    N, calls, ref = wide_case
    assert 1700 < len(ref.records) < 2000 and len(ref.calls[0]) > 100      # cap = 100 overflows inside the first call
    assert any(r[0] >= 1024 for r in ref.records)
    tr = _run_tracker(dev, calls, N, cap)
    _check_against_ref(tr, ref, cap)
    again = _run_tracker(dev, calls, N, cap)
    assert torch.equal(tr.totals, again.totals) and torch.equal(tr.rec_f, again.rec_f) and torch.equal(tr.rec_i, again.rec_i)


# ---- 2. greedy act ------------------------------------------------------------------------------------------------------------

GREEDY_CASES = {
    "n5_reference_widths": dict(N=5, cfg={}),                                  # float4 row path, a partly filled last block
    "n33_scalar_rows": dict(N=33, cfg=dict(in_channels=128, hidden=96)),      # H % 256 != 0: the scalar row path
    "three_actions": dict(N=6, cfg=dict(num_actions=3)),
    "seven_actions": dict(N=6, cfg=dict(num_actions=7)),                       # A + 1 = 8: the template bound
    "coordinate_goal": dict(N=6, cfg=dict(goal_in=2, num_actions=4)),         # the _vec entry
}


def _act_inputs(h, N, dev, seed=9):
    g = torch.Generator().manual_seed(seed)
    C, S = h.cfg["in_channels"], h.cfg["spatial"]
    feat = (torch.randn(N, S * S, C, generator=g).abs() * 0.5).to(torch.bfloat16).to(dev)
    goal = (syn.synthetic_goal_vectors(6, (N,), h.goal_in) if h.goal_in else syn.synthetic_goals(6, (N,))).to(dev)
    h0 = (torch.randn(N, h.H, generator=g) * 0.3).to(dev)
    m = (torch.rand(N, generator=g) > 0.2).float().to(dev)
    return feat, goal, h0, m


def _mode_actions(lib, hv, A):
    from embodied_clip_amd import _lib
    N = hv.shape[0]
    a = torch.full((N,), -1, dtype=torch.int64, device=hv.device)
    lp, v = torch.zeros(N, device=hv.device), torch.zeros(N, device=hv.device)
    _lib.check(lib.ec_mode_actions(hv.data_ptr(), a.data_ptr(), lp.data_ptr(), v.data_ptr(), N, A, 0), "ec_mode_actions")
    return a, lp, v


def _check_mode(hv, A, actions, logp, values):
    logits = hv[:, :A].double().cpu()
    assert np.array_equal(actions.cpu().numpy(), np.argmax(hv[:, :A].cpu().numpy(), -1))     # numpy: the first occurrence
    ref = torch.log_softmax(logits, -1).gather(1, actions.cpu().view(-1, 1)).view(-1)
    err = (logp.double().cpu() - ref).abs().max().item()
    bound = 1e-5 * max(1.0, logits.abs().max().item())
    print("greedy logp err", err, "bound", bound)
    assert err <= bound
    assert torch.equal(values, hv[:, A])


@pytest.mark.parametrize("name", list(GREEDY_CASES))
def test_greedy_act_is_forward_plus_mode(dev, name):
    from embodied_clip_amd import _lib
    from embodied_clip_amd.policy import PolicyHandle
    lib = _lib.load()
    case = GREEDY_CASES[name]
    N, h = case["N"], PolicyHandle(**case["cfg"])
    A = h.A
    flat = h.flatten(syn.policy_state_dict(5, **case["cfg"]), dev)
    feat, goal, h0, m = _act_inputs(h, N, dev)
    ws_a = torch.empty(h.workspace_bytes(1, N, False), dtype=torch.uint8, device=dev)
    ws_b = torch.empty_like(ws_a)
    for reuse in (False, True):
        hv_a, hf_a = h.forward(flat, feat, goal, h0, m, 1, N, ws_a, for_backward=False, reuse_tables=reuse)
        act_a, lp_a, v_a = _mode_actions(lib, hv_a, A)
        hv_b, hf_b = torch.empty_like(hv_a), torch.empty_like(hf_a)
        act_b = torch.full((N,), -1, dtype=torch.int64, device=dev)
        lp_b, v_b = torch.zeros(N, device=dev), torch.zeros(N, device=dev)
        h.act(flat, feat, goal, h0, m, N, ws_b, hv_b, hf_b, act_b, lp_b, v_b, reuse_tables=reuse, deterministic=True)
        torch.cuda.synchronize()
        assert torch.equal(hv_a, hv_b) and torch.equal(hf_a, hf_b)
        assert torch.equal(act_a, act_b) and torch.equal(lp_a, lp_b) and torch.equal(v_a, v_b)
        _check_mode(hv_b, A, act_b, lp_b, v_b)
        assert (lp_b < 0).all()


def test_greedy_act_more_than_seven_actions(dev):
    """Nine actions: the fused entry refuses (EC_ERR_UNSUPPORTED), the two-call route serves it."""
    from embodied_clip_amd import _lib
    from embodied_clip_amd.policy import PolicyHandle
    lib = _lib.load()
    cfg = dict(num_actions=9)
    N, h = 6, PolicyHandle(**cfg)
    flat = h.flatten(syn.policy_state_dict(5, **cfg), dev)
    feat, goal, h0, m = _act_inputs(h, N, dev)
    ws = torch.empty(h.workspace_bytes(1, N, False), dtype=torch.uint8, device=dev)
    hv, hf = h.forward(flat, feat, goal, h0, m, 1, N, ws, for_backward=False)
    a = torch.zeros(N, dtype=torch.int64, device=dev)
    lp, v = torch.zeros(N, device=dev), torch.zeros(N, device=dev)
    with pytest.raises(_lib.EcError, match=r"code -6"):
        h.act(flat, feat, goal, h0, m, N, ws, torch.empty_like(hv), torch.empty_like(hf), a, lp, v, deterministic=True)
    a, lp, v = _mode_actions(lib, hv, 9)
    torch.cuda.synchronize()
    _check_mode(hv, 9, a, lp, v)


def test_greedy_act_ties_take_the_first_index(dev):
    from embodied_clip_amd.policy import PolicyHandle
    N, h = 6, PolicyHandle()
    feat, goal, h0, m = _act_inputs(h, N, dev)
    ws = torch.empty(h.workspace_bytes(1, N, False), dtype=torch.uint8, device=dev)

    def act(sd):
        flat = h.flatten(sd, dev)
        hv, hf = torch.empty((N, 7), device=dev), torch.empty((N, 512), device=dev)
        a = torch.full((N,), -1, dtype=torch.int64, device=dev)
        lp, v = torch.zeros(N, device=dev), torch.zeros(N, device=dev)
        h.act(flat, feat, goal, h0, m, N, ws, hv, hf, a, lp, v, deterministic=True)
        torch.cuda.synchronize()
        return hv, a, lp

    sd = syn.policy_state_dict(5)
    sd["actor.linear.weight"] = torch.zeros_like(sd["actor.linear.weight"])
    sd["actor.linear.bias"] = torch.full_like(sd["actor.linear.bias"], 0.3)
    hv, a, lp = act(sd)
    assert (hv[:, :6] == hv[:, :1]).all() and a.tolist() == [0] * N
    assert (lp.double().cpu() + np.log(6.0)).abs().max().item() <= 1e-5
    sd = syn.policy_state_dict(5)
    sd["actor.linear.weight"][4] = sd["actor.linear.weight"][2]
    sd["actor.linear.bias"][:] = 0
    sd["actor.linear.bias"][2] = sd["actor.linear.bias"][4] = 50.0
    hv, a, lp = act(sd)
    assert torch.equal(hv[:, 2], hv[:, 4]) and (hv[:, 2:3] >= hv[:, :6]).all() and a.tolist() == [2] * N


# ---- 3. Evaluator == the training rollout --------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,T", [(4, 3), (64, 2)])
def test_evaluator_equals_training_rollout(dev, N, T):
    from embodied_clip_amd.engine import Worker
    from embodied_clip_amd.evaluate import Evaluator
    enc_sd, pol_sd = syn.rn50_visual_state_dict(0), syn.policy_state_dict(0)
    w = Worker(N, T=T, device="cuda:0", seed=5, update_repeats=1, encoder_sd=enc_sd, policy_sd=pol_sd)
    got = []
    w.collect_rollout()
    torch.cuda.synchronize()
    got.append((w.actions.clone(), w.logp.clone(), w.values[:T].clone()))
    w.after_update()                                  # (no update(): the weights stay those the evaluator holds)
    w.collect_rollout()
    torch.cuda.synchronize()
    got.append((w.actions.clone(), w.logp.clone(), w.values[:T].clone()))
    ns = w.ns
    del w
    ev = Evaluator(N, T=T, device="cuda:0", seed=5, encoder_sd=enc_sd, policy_sd=pol_sd, record=True)
    ev.run(2)
    torch.cuda.synchronize()
    assert ev.ns == ns == (2 if N >= 48 else 1)
    for i, x in enumerate((ev.actions, ev.logp, ev.values)):
        assert torch.equal(x, torch.cat([got[0][i], got[1][i]])), i
    assert len(set(ev.actions.flatten().tolist())) > 1
    for sl in ev.slices:
        assert sl.feat.shape[0] == 2 and not hasattr(sl, "ws_learn") and not hasattr(sl, "hv") and not hasattr(sl, "grads")
    assert not hasattr(ev, "grads") and not hasattr(ev, "opt")
    det = Evaluator(N, T=T, device="cuda:0", seed=5, encoder_sd=enc_sd, policy_sd=pol_sd, record=True, deterministic=True)
    det.run(2)
    torch.cuda.synchronize()
    assert torch.equal(det.hv, ev.hv)                 # the synthetic env does not read the actions
    A = det.A
    flat = det.hv.view(-1, A + 1)
    assert np.array_equal(det.actions.view(-1).cpu().numpy(), np.argmax(flat[:, :A].cpu().numpy(), -1))
    assert torch.equal(det.values.view(-1), flat[:, A])
    assert not torch.equal(det.actions, ev.actions)


# ---- 4. metrics through the engine ---------------------------------------------------------------------------------------------

def _set_env(env, call, dev):
    rewards, masks, success = call
    env.rewards.copy_(torch.from_numpy(rewards).to(dev))
    env.masks.copy_(torch.from_numpy(masks).to(dev))
    env.success.copy_(torch.from_numpy(success).to(dev))


def test_metrics_through_evaluator_and_worker(dev):
    from embodied_clip_amd.engine import SyntheticEnv, Worker
    from embodied_clip_amd.evaluate import Evaluator
    T, N = er.HAND_T, er.HAND_N
    calls = er.hand_case()
    ref = er.EpisodeRef(N)
    for c in calls:
        ref.update(*c)
    want = ref.info()
    enc_sd = syn.rn50_visual_state_dict(0)
    env = SyntheticEnv(N, T, dev, seed=1000)
    assert torch.equal(env.success, ((env.rewards > 1) & (env.masks[1:] == 0)).float())
    ev = Evaluator(N, T=T, device="cuda:0", seed=2, encoder_sd=enc_sd, env=env, record_capacity=16)
    assert ev.info()["episodes"] == 0 and np.isnan(ev.info()["success"])
    for c in calls:
        _set_env(env, c, dev)
        ev.run(1)
    info = ev.info()
    n = want["episodes"]
    abs_s, _ = ref.abs_sums()
    print("evaluator info", info, "reference", want)
    assert info["episodes"] == n and info["ep_length"] == want["ep_length"] and info["success"] == want["success"]
    # the mean of an n-term double sum against the correctly rounded one: the sum's bound, and the two divisions' roundings
    assert abs(info["reward"] - want["reward"]) <= (n + 2) * U * abs_s / n
    # sqrt(E[x^2] - mean^2) of ~10-sized returns: the difference carries ~100 * 2^-53 * n absolute error, its root less -- 1e-12
    assert abs(info["reward_std"] - want["reward_std"]) <= 1e-12
    assert ev.episodes.records()["length"].tolist() == er.HAND_LENGTHS[0] + er.HAND_LENGTHS[1]
    # ... and against numpy's own mean / population deviation of the reference's returns (another formula: two passes)
    rets = np.array([r[3] for r in ref.records], dtype=np.float64)
    assert abs(info["reward"] - rets.mean()) <= (n + 2) * U * abs_s / n and abs(info["reward_std"] - rets.std()) <= 1e-12
    w = Worker(N, T=T, device="cuda:0", seed=2, update_repeats=1, encoder_sd=enc_sd, track_episodes=True)
    for c in calls:
        _set_env(w.env, c, dev)
        w.iteration()
    torch.cuda.synchronize()
    assert w.episode_info() == info
    with pytest.raises(RuntimeError):
        Worker(N, T=T, device="cuda:0", seed=2, update_repeats=1, encoder_sd=enc_sd).episode_info()


# ---- 5. checkpoints ------------------------------------------------------------------------------------------------------------

def test_checkpoint_round_trip(dev, tmp_path):
    from embodied_clip_amd import spaces
    from embodied_clip_amd.engine import Worker
    from embodied_clip_amd.evaluate import Evaluator
    from embodied_clip_amd.policy import ResnetTensorObjectNavActorCritic
    N, T = 4, 3
    enc_sd = syn.rn50_visual_state_dict(0)
    w = Worker(N, T=T, device="cuda:0", seed=7, update_repeats=2, encoder_sd=enc_sd)
    start = w.params.clone()
    w.iteration()
    torch.cuda.synchronize()
    assert not torch.equal(start, w.params)
    path = str(tmp_path / ("exp__stage_00__steps_%d.pt" % w.total_steps))
    w.save_checkpoint(path)
    ck = torch.load(path, map_location="cpu")
    assert set(ck) == {"model_state_dict", "optimizer_state_dict", "total_steps"}
    assert list(ck["model_state_dict"]) == list(syn.POLICY_PARAM_ORDER)
    assert set(ck["optimizer_state_dict"]) == {"exp_avg", "exp_avg_sq", "step"}

    w2 = Worker(N, T=T, device="cuda:0", seed=7, update_repeats=2, encoder_sd=enc_sd)
    w2.collect_rollout()                              # (the act tables of the untrained weights are now valid)
    assert all(sl.act_tables_valid for sl in w2.slices) and not torch.equal(w2.params, w.params)
    w2.load_checkpoint(path)
    torch.cuda.synchronize()
    assert torch.equal(w2.params, w.params) and torch.equal(w2.opt.m, w.opt.m) and torch.equal(w2.opt.v, w.opt.v)
    assert w2.opt.step_count == w.opt.step_count == 2 and w2.total_steps == w.total_steps == T * N
    assert not any(sl.act_tables_valid for sl in w2.slices)
    assert w2.iter == w.iter == 1                    # the sampling keys go on from the checkpoint's iteration
    del w2

    obs_space = spaces.Dict({"rgb_clip_resnet": spaces.Box(-1e9, 1e9, (2048, 7, 7)), "goal": spaces.Discrete(12)})
    model = ResnetTensorObjectNavActorCritic(spaces.Discrete(6), obs_space, "goal", "rgb_clip_resnet", device=dev)
    res = model.load_state_dict(ck["model_state_dict"])
    assert not res.missing_keys and not res.unexpected_keys
    for name, v in w.policy.views(w.params).items():
        assert torch.equal(dict(model.named_parameters())[name].data, v), name

    # an Evaluator that takes over where the trained Worker stands -- its env (rewound by the one observation the evaluator
    # makes itself: the Worker re-uses the last features of its rollout), its memory, its iteration count -- plays the
    # Worker's next rollout
    k = w.env._k
    w.env._k = k - 1
    ev = Evaluator(N, T=T, device="cuda:0", seed=7, encoder_sd=enc_sd, checkpoint=path, env=w.env, record=True)
    assert ev.checkpoint_steps == w.total_steps and torch.equal(ev.params, w.params)
    ev.h.copy_(w.h)
    ev.chunk = w.iter
    ev.run(1)
    torch.cuda.synchronize()
    w.env._k = k
    w.collect_rollout()
    torch.cuda.synchronize()
    assert torch.equal(ev.values, w.values[:T])
    assert torch.equal(ev.actions, w.actions) and torch.equal(ev.logp, w.logp)

"""GPU: multi-layer recurrent cores through the engine -- ``Worker(rnn_layers=2)``, the ``Evaluator``, checkpoints -- at 8 actors, a
rollout of 4 steps and hidden 64.  The recurrent memory everywhere is ``[N, L * SW]`` layer-major rows; the act steps are replayed
on the worker's own features against tests/_rnn_stack_ref.py (tolerance: ``test_worker_iteration_matches_oracle``'s)."""
import os
import sys

import pytest
import torch

from embodied_clip_amd import synthetic as syn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _rnn_stack_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T, N, R, H, L = 4, 8, 2, 64, 2
CELLS = ("GRU", "LSTM")


def _rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-20)).item()


def _pkw(kw):
    p = {k: kw[k] for k in ("goal_in", "num_actions") if k in kw}
    if kw.get("prev_actions"):
        p.update(prev_action_dims=kw["prev_actions"], prev_action_null=1)
    return p


@pytest.fixture(scope="module")
def enc_sd():
    return syn.rn50_visual_state_dict(0)


def _worker(enc_sd, cell, layers=L, pol_sd=None, **kw):
    from embodied_clip_amd.engine import Worker
    if pol_sd is None:
        pol_sd = syn.policy_state_dict(0, hidden=H, **_pkw(kw), rnn_type=cell, rnn_layers=layers)
    return Worker(N, T=T, device=DEV, seed=3, update_repeats=R, encoder_sd=enc_sd, policy_sd=pol_sd, rnn_type=cell, rnn_layers=layers,
                  hidden=H, **kw), pol_sd


@pytest.mark.parametrize("cell,kw", [("GRU", {}), ("LSTM", {}), ("LSTM", dict(goal_in=2, num_actions=4, prev_actions=6)),
                                     ("GRU", dict(num_actions=84, loss="ppo+imitation"))])
def test_worker_trains_and_is_reproducible(enc_sd, cell, kw):
    """two iterations: finite losses, parameters that move (the upper layer's among them), a live upper slice of the memory, and
    a second worker from the same seed ends with the same parameters, bit for bit"""
    w, pol_sd = _worker(enc_sd, cell, **kw)
    SW = (2 if cell == "LSTM" else 1) * H
    assert w.policy.rnn_layers == L and w.SW == L * SW and w.h.shape == w.h_next.shape == w.h_start.shape == (N, L * SW)
    # the engine's sections cover the whole bucket: the upper layers' gradients travel with the sections outside the recurrent one
    secs = sorted([w.rec] + w._other_sections(), key=lambda s: s.start)
    assert secs[0].start == 0 and secs[-1].stop == w.grads.numel() and all(a.stop == b.start for a, b in zip(secs, secs[1:]))
    assert all(w.policy.offsets[k][0] >= w.rec.stop for k in ref.names(1))
    before = w.params.clone()
    for _ in range(2):
        w.iteration()
        torch.cuda.synchronize()
        info = w.loss_info()
        assert all(v == v and abs(v) != float("inf") for v in info.values()), info
    assert torch.isfinite(w.params).all() and torch.isfinite(w.h).all()
    assert float(w.h[:, SW:].abs().max()) > 0                              # the upper layer's slice of the memory is live
    pv, p0 = w.policy.views(w.params), w.policy.views(before)
    for name in ref.names(0) + ref.names(1) + ("actor.linear.weight",):
        assert not torch.equal(pv[name], p0[name]), name
    w2, _ = _worker(enc_sd, cell, pol_sd=pol_sd, **kw)
    w2.iteration()
    w2.iteration()
    torch.cuda.synchronize()
    assert torch.equal(w2.params, w.params) and torch.equal(w2.actions, w.actions) and torch.equal(w2.h, w.h)


@pytest.mark.parametrize("cell", CELLS)
def test_act_steps_match_the_reference_replayed_on_the_workers_features(enc_sd, cell):
    w, pol_sd = _worker(enc_sd, cell)
    w.collect_rollout()
    torch.cuda.synchronize()
    S, C = w.S, w.C
    feat = w.feat.float().cpu().view(T + 1, N, S, S, C).permute(0, 1, 4, 2, 3).contiguous()
    masks, goals, actions = w.env.masks.cpu().unsqueeze(-1), w.env.goals.cpu(), w.actions.cpu()
    from oracle import policy as opol
    state = torch.zeros(1, N, w.SW)
    vals, lps = [], []
    with torch.no_grad():
        for t in range(T + 1):
            lg, v, s2 = ref.actor_critic_forward(cell, feat[t][None], goals[t][None], None, state, masks[t][None], pol_sd, 0)
            vals.append(v[0])
            if t < T:
                lps.append(opol.categorical_log_prob(lg, actions[t][None])[0])
                state = s2
    assert _rel(w.values.unsqueeze(-1), torch.stack(vals)) < 1e-4
    assert (w.logp.cpu() - torch.stack(lps)).abs().max() < 1e-4
    # (the two memory buffers ping-pong by step parity: one of them holds the state behind step T - 1)
    assert min(_rel(w.h, state[0]), _rel(w.h_next, state[0])) < 1e-4


def test_checkpoint_round_trip_and_refusals(enc_sd, tmp_path):
    from embodied_clip_amd.engine import Worker
    from embodied_clip_amd.evaluate import Evaluator
    cell = "LSTM"
    a, pol_sd = _worker(enc_sd, cell)
    a.iteration()
    path = str(tmp_path / "two_layers.pt")
    a.save_checkpoint(path)
    a.iteration()
    torch.cuda.synchronize()
    ck = torch.load(path, map_location="cpu")
    assert tuple(ck["model_state_dict"][ref.names(1)[0]].shape) == (4 * H, H) and tuple(ck["model_state_dict"][ref.names(1)[3]].shape) == (4 * H,)
    # save -> load -> one more iteration == the uninterrupted run
    b, _ = _worker(enc_sd, cell, pol_sd=pol_sd)
    b.iteration()
    b.load_checkpoint(path)
    b.iteration()
    torch.cuda.synchronize()
    assert torch.equal(b.params, a.params) and b.total_steps == a.total_steps and torch.equal(b.opt.m, a.opt.m)
    ev = Evaluator(N, T=T, device=DEV, seed=3, encoder_sd=enc_sd, checkpoint=path, rnn_type=cell, rnn_layers=L, hidden=H)
    c, _ = _worker(enc_sd, cell)
    c.load_checkpoint(path)
    assert torch.equal(ev.params, c.params) and ev.h.shape == (N, L * 2 * H)
    # a one-layer checkpoint into the two-layer agent: refused, naming the missing tensor and the file; and the reverse
    one, _ = _worker(enc_sd, cell, layers=1)
    old = str(tmp_path / "one_layer.pt")
    one.save_checkpoint(old)
    with pytest.raises(KeyError) as e:
        c.load_checkpoint(old)
    assert ref.names(1)[0] in str(e.value) and str((4 * H, H)) in str(e.value) and old in str(e.value)
    with pytest.raises(KeyError, match="weight_ih_l1"):
        Evaluator(N, T=T, device=DEV, seed=3, encoder_sd=enc_sd, checkpoint=old, rnn_type=cell, rnn_layers=L, hidden=H)
    with pytest.raises(ValueError) as e:
        one.load_checkpoint(path)
    assert ref.names(1)[0] in str(e.value) and path in str(e.value)
    # refused before anything is allocated
    for bad in (dict(depth=True), dict(zeroshot=True)):
        with pytest.raises(ValueError, match="rnn_layers"):
            Worker(N, T=T, device=DEV, rnn_layers=2, **bad)
        with pytest.raises(ValueError, match="rnn_layers"):
            Evaluator(N, T=T, device=DEV, rnn_layers=2, **bad)
    with pytest.raises(ValueError, match="rnn_layers"):
        Worker(N, T=T, device=DEV, rnn_layers=5)


@pytest.mark.parametrize("cell", CELLS)
def test_evaluator_runs_a_chunk_and_equals_the_handle_level_act_loop(enc_sd, cell):
    from embodied_clip_amd.evaluate import Evaluator
    pol_sd = syn.policy_state_dict(0, hidden=H, rnn_type=cell, rnn_layers=L)
    ev = Evaluator(N, T=T, device=DEV, seed=3, encoder_sd=enc_sd, policy_sd=pol_sd, record=True, deterministic=True, rnn_type=cell,
                   rnn_layers=L, hidden=H)
    info = ev.run(1)
    assert info and all(v == v for v in info.values() if isinstance(v, float))
    w, _ = _worker(enc_sd, cell, pol_sd=pol_sd)
    w.collect_rollout()
    torch.cuda.synchronize()
    pol, flat = w.policy, w.params
    ws = torch.empty(pol.workspace_bytes(1, N, False), dtype=torch.uint8, device=DEV)
    h = torch.zeros(N, w.SW, device=DEV)
    for t in range(T):
        hv, hf = torch.empty(N, 7, device=DEV), torch.empty(N, w.SW, device=DEV)
        act, lp, v = torch.zeros(N, dtype=torch.int64, device=DEV), torch.zeros(N, device=DEV), torch.zeros(N, device=DEV)
        pol.act(flat, w.feat[t].contiguous(), w.env.goals[t].contiguous(), h, w.env.masks[t].contiguous(), N, ws, hv, hf, act, lp, v,
                deterministic=True)
        torch.cuda.synchronize()
        assert torch.equal(ev.actions[t], act) and torch.equal(ev.logp[t], lp) and torch.equal(ev.hv[t], hv), t
        h = hf

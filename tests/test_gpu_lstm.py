"""GPU: policy handles with an LSTM core (``PolicyHandle(rnn_type="LSTM")``, ``ec_policy_create_rnn``) against the float64 /
fp32 restatement in tests/_lstm_ref.py, case by case as tests/test_gpu_prev_action.py does for the previous-action embedding.

Tolerances are the policy path's standing ones (test_gpu_policy.py / test_gpu_pointnav.py): forward rel-L2 < 2e-5, per-tensor
gradient rel-L2 < 2e-4, the loss 1e-5 relative, the Adam update as in ``test_policy_backward_and_update_step_match_oracle``.  The
fp32 torch reference agrees with its float64 self to <= 1.3e-6 (forward) and <= 1.4e-6 (worst gradient tensor) at these shapes
(tests/test_lstm_ref.py measures each case and holds it to a tenth of its bound), so the bounds test the kernels.

Cases are (T, N, S, C, H, E, null, A, goal_in, bf16 features) -- tests/_lstm_ref.py::POLICY_CASES:
  (1, 1, 7, ..)                                       the act step at one actor
  (3, 5, 7, .., H 64)                                 basic learn pass
  (6, 4, 3, .., H 32)                                 flat = 288: the routes that keep weight_ih's column order
  (4, 33, 7, .., E 32, null 1, A 4, goal_in 3) bf16   coordinate goals with previous actions
  (2, 16, 7, H 512) bf16                              the fused backward, two K chunks
  (3, 5, 7, H 256, E 6, A 84)                         the wide learn plan, fused backward
The recurrent state everywhere is rows [h | c] of width 2H.
"""
import functools
import os
import sys

import pytest
import torch

from embodied_clip_amd import synthetic as syn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _lstm_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = ref.POLICY_CASES


def _rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-20)).item()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _case(*case):
    """Inputs and the reference's forward / optimiser step, computed once per case and shared (never modified)."""
    cfg, sd, batch = ref.policy_inputs(*case)
    r = ref.policy_reference(sd, batch, case[6])
    return dict(cfg=cfg, sd=sd, **r)


def _handle(cfg):
    from embodied_clip_amd.policy import PolicyHandle
    return PolicyHandle(rnn_type="LSTM", **cfg)


def _gpu_inputs(cfg, b, dev, bf16):
    T, N = b["feat"].shape[:2]
    rows = b["feat"].permute(0, 1, 3, 4, 2).reshape(T * N, cfg["spatial"] ** 2, cfg["in_channels"]).contiguous()
    rows = (rows.to(torch.bfloat16) if bf16 else rows.float()).to(dev)
    goal = (b["goal"].reshape(T * N, cfg["goal_in"]).float() if cfg["goal_in"] else b["goal"].reshape(T * N)).contiguous().to(dev)
    prev = b["prev_actions"].reshape(-1).contiguous().to(dev) if cfg["prev_action_dims"] else None
    return rows, goal, prev, b["h0"][0].float().contiguous().to(dev), b["masks"].reshape(-1).float().to(dev)


def _learn_step(cfg, sd, b, dev, bf16, dhv_zero=False, dh_final=None):
    """forward (learn plan), PPO loss, backward twice on the GPU -> (handle, flat, hv, h_final, sums, grads, again)"""
    from embodied_clip_amd import ppo
    T, N = b["feat"].shape[:2]
    h = _handle(cfg)
    flat = h.flatten(sd, dev)
    rows, goal, prev, h0, m = _gpu_inputs(cfg, b, dev, bf16)
    ws = torch.empty(h.workspace_bytes(T, N, True), dtype=torch.uint8, device=dev)
    hv, hf = h.forward(flat, rows, goal, h0, m, T, N, ws, prev_actions=prev)
    f = lambda t: t.reshape(-1).float().contiguous().to(dev)
    if dhv_zero:
        dhv, sums = torch.zeros_like(hv), None
    else:
        dhv, sums = ppo.ppo_loss_raw(hv, b["actions"].reshape(-1).to(dev), f(b["old_log_probs"]), f(b["old_values"]), f(b["returns"]),
                                     f(b["norm_adv"]), cfg["num_actions"])
    grads = torch.zeros_like(flat)
    h.backward(flat, rows, m, T, N, ws, dhv, dh_final, grads)
    again = torch.zeros_like(flat)                       # the same backward once more (reads the same workspace)
    h.backward(flat, rows, m, T, N, ws, dhv, dh_final, again)
    torch.cuda.synchronize()
    return h, flat, hv, hf, sums, grads, again


@pytest.mark.parametrize("case", CASES)
def test_forward_matches_reference(dev, case):
    T, N, H, A, bf16 = case[0], case[1], case[4], case[7], case[9]
    c = _case(*case)
    h = _handle(c["cfg"])
    assert h.state_width == 2 * H and h.shapes[ref.WHH] == (4 * H, H)
    flat = h.flatten(c["sd"], dev)
    rows, goal, prev, h0, m = _gpu_inputs(c["cfg"], c["batch"], dev, bf16)
    ws = torch.empty(h.workspace_bytes(T, N, False), dtype=torch.uint8, device=dev)
    hv, hf = h.forward(flat, rows, goal, h0, m, T, N, ws, for_backward=False, prev_actions=prev)
    torch.cuda.synchronize()
    assert tuple(hf.shape) == (N, 2 * H)
    hv = hv.view(T, N, -1)
    st = c["h"][0]
    errs = (_rel(hv[..., :A], c["logits"]), _rel(hv[..., A:], c["values"]), _rel(hf[:, :H], st[:, :H]), _rel(hf[:, H:], st[:, H:]))
    print("forward rel-L2 (logits, values, h, c):", errs)
    assert max(errs) < ref.FWD_TOL, errs
    # in place (h_final is h0): the same bits
    h0b = h0.clone()
    hv2, hf2 = h.forward(flat, rows, goal, h0b, m, T, N, ws, for_backward=False, prev_actions=prev, h_final=h0b)
    torch.cuda.synchronize()
    assert torch.equal(hv2.view(T, N, -1), hv) and torch.equal(hf2, hf)


@pytest.mark.parametrize("case", CASES)
def test_optimiser_step_matches_reference_and_is_deterministic(dev, case):
    """forward, PPO loss, backward, clip, Adam: every gradient and the parameter update; two backward passes give equal bits
    (no float atomics on any route of an LSTM handle)."""
    from embodied_clip_amd import ppo
    T, N, H, A, bf16 = case[0], case[1], case[4], case[7], case[9]
    c = _case(*case)
    info, ref_grads, sd, sd_ref = c["info"], c["ref_grads"], c["sd"], c["sd_ref"]
    h, flat, hv, hf, sums, grads, again = _learn_step(c["cfg"], sd, c["batch"], dev, bf16)
    hv3 = hv.view(T, N, -1)
    assert _rel(hv3[..., :A], c["logits"]) < ref.FWD_TOL and _rel(hv3[..., A:], c["values"]) < ref.FWD_TOL   # the learn plan's forward
    assert _rel(hf, c["h"][0]) < ref.FWD_TOL
    total = ((sums[0] + 0.5 * sums[1] + 0.01 * sums[2]) / (T * N)).item()
    assert abs(total - info["ppo_total"]) < 1e-5 * max(1.0, abs(info["ppo_total"]))
    gv = h.views(grads)
    assert set(gv) == set(ref_grads)
    errs = {name: _rel(gv[name], gref) for name, gref in ref_grads.items()}
    print("gradient rel-L2:", errs)
    for name, e in errs.items():
        assert e < ref.GRAD_TOL, (name, e)
    assert torch.equal(grads, again)
    # a second learn pass from scratch: equal bits again
    _, _, hv_b, hf_b, _, grads_b, _ = _learn_step(c["cfg"], sd, c["batch"], dev, bf16)
    assert torch.equal(hv_b, hv) and torch.equal(hf_b, hf) and torch.equal(grads_b, grads)
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


@pytest.mark.parametrize("case", [CASES[1], CASES[3], CASES[4]])
def test_dh_final_with_a_cell_half_reaches_the_gradients(dev, case):
    """backward(dhv = 0, dh_final = [dh | dc]) == the float64 gradients of sum(dstate * final state); with the c half zeroed the
    gradients change, so the c half is read."""
    c = _case(*case)
    b = c["batch"]
    want = ref.state_grad_reference(c["sd"], {**b, "noise": None}, case[6])
    dstate = b["dstate"].float().contiguous().to(dev)
    h, _, _, _, _, grads, again = _learn_step(c["cfg"], c["sd"], b, dev, case[9], dhv_zero=True, dh_final=dstate)
    gv = h.views(grads)
    live = 0
    for name, gref in want.items():
        if float(gref.abs().max()) == 0:
            assert not gv[name].any(), name            # (the heads receive nothing)
            continue
        live += 1
        assert _rel(gv[name], gref) < ref.GRAD_TOL, (name, _rel(gv[name], gref))
    assert live >= 8 and torch.equal(grads, again)
    H = case[4]
    half = dstate.clone()
    half[:, H:] = 0
    _, _, _, _, _, g_half, _ = _learn_step(c["cfg"], c["sd"], b, dev, case[9], dhv_zero=True, dh_final=half)
    assert not torch.equal(g_half, grads)


def test_forward_does_not_depend_on_actor_slicing(dev):
    """The act step of 37 actors == the act steps of actors [0, 19) and [19, 37), bit for bit, state rows included."""
    case = (1, 37, 7, 64, 32, 6, 1, 6, 0, True)
    cfg, sd, b = ref.policy_inputs(*case)
    h = _handle(cfg)
    flat = h.flatten(sd, dev)
    rows, goal, prev, h0, m = _gpu_inputs(cfg, b, dev, True)

    def run(a, z):
        n = z - a
        ws = torch.empty(h.workspace_bytes(1, n, False), dtype=torch.uint8, device=dev)
        return h.forward(flat, rows[a:z].contiguous(), goal[a:z].contiguous(), h0[a:z].contiguous(), m[a:z].contiguous(), 1, n, ws,
                         for_backward=False, prev_actions=prev[a:z].contiguous())
    hv, hf = run(0, 37)
    hv_a, hf_a = run(0, 19)
    hv_b, hf_b = run(19, 37)
    torch.cuda.synchronize()
    assert torch.equal(hv, torch.cat([hv_a, hv_b])) and torch.equal(hf, torch.cat([hf_a, hf_b]))


@pytest.mark.parametrize("case", [CASES[1], CASES[4]])
def test_chained_act_steps_equal_the_sequence_forward(dev, case):
    """a T-step inference forward and T chained act steps (each fed the previous state rows) agree within the forward bound"""
    T, N, H, bf16 = case[0], case[1], case[4], case[9]
    c = _case(*case)
    h = _handle(c["cfg"])
    flat = h.flatten(c["sd"], dev)
    rows, goal, prev, h0, m = _gpu_inputs(c["cfg"], c["batch"], dev, bf16)
    ws = torch.empty(h.workspace_bytes(T, N, False), dtype=torch.uint8, device=dev)
    hv, hf = h.forward(flat, rows, goal, h0, m, T, N, ws, for_backward=False)
    hv, hf = hv.clone(), hf.clone()
    ws1 = torch.empty(h.workspace_bytes(1, N, False), dtype=torch.uint8, device=dev)
    state, steps = h0, []
    for t in range(T):
        sl = slice(t * N, (t + 1) * N)
        hv_t, state = h.forward(flat, rows[sl].contiguous(), goal[sl].contiguous(), state, m[sl].contiguous(), 1, N, ws1, for_backward=False,
                                reuse_tables=t > 0)
        steps.append(hv_t.clone())
        state = state.clone()
    torch.cuda.synchronize()
    assert _rel(torch.cat(steps), hv) < ref.FWD_TOL and _rel(state, hf) < ref.FWD_TOL


@pytest.mark.parametrize("T", [1, 3])
def test_mask_zero_resets_both_states(dev, T):
    """a mask zero at step t makes the result independent of BOTH incoming states: perturb h0 and c0 of the masked actors, equal bits"""
    case = (T, 5, 7, 64, 64, 0, 0, 6, 0, False)
    cfg, sd, b = ref.policy_inputs(*case)
    N, H = 5, 64
    h = _handle(cfg)
    flat = h.flatten(sd, dev)
    rows, goal, prev, h0, m = _gpu_inputs(cfg, b, dev, False)
    m = m.clone()
    m[:N] = torch.tensor([0.0, 1.0, 0.0, 1.0, 1.0], device=dev)             # step 0: actors 0 and 2 start an episode
    outs = []
    for which in (None, "h", "c", "both"):
        s0 = h0.clone()
        if which in ("h", "both"):
            s0[[0, 2], :H] += 3.0
        if which in ("c", "both"):
            s0[[0, 2], H:] -= 5.0
        for learn in (False, True):
            ws = torch.empty(h.workspace_bytes(T, N, learn), dtype=torch.uint8, device=dev)
            hv, hf = h.forward(flat, rows, goal, s0, m, T, N, ws, for_backward=learn)
            outs.append((learn, hv.clone(), hf.clone()))
    torch.cuda.synchronize()
    for learn, hv, hf in outs[2:]:
        base = outs[1] if learn else outs[0]
        assert torch.equal(hv, base[1]) and torch.equal(hf, base[2])
    # ... and an unmasked actor does depend on its cell state
    s0 = h0.clone()
    s0[1, H:] += 1.0
    ws = torch.empty(h.workspace_bytes(T, N, False), dtype=torch.uint8, device=dev)
    hv, _ = h.forward(flat, rows, goal, s0, m, T, N, ws, for_backward=False)
    assert not torch.equal(hv, outs[0][1])


@pytest.mark.parametrize("N", [1, 5, 33])
@pytest.mark.parametrize("A,goal_in,E", [(6, 0, 0), (84, 0, 0), (4, 2, 6)])
def test_act_step_is_forward_plus_selection_with_table_reuse(dev, N, A, goal_in, E):
    """``act`` / ``act_ex`` / the greedy act == ``forward(T = 1)`` + ``ec_sample_actions`` / ``ec_mode_actions``, bit for bit (wide heads:
    the state bit for bit, the selection on the hv the heads launch wrote), at the agent's real widths (2048 channels, 7 x 7,
    hidden 512); EC_POLICY_INFER_REUSE after a parameter-preserving call gives the bits of EC_POLICY_INFER."""
    from embodied_clip_amd import _lib
    lib = _lib.load()
    kw = dict(num_actions=A, goal_in=goal_in, prev_action_dims=E, prev_action_null=1 if E else 0)
    h = _handle(kw)
    sd = syn.policy_state_dict(5, **kw, rnn_type="LSTM")
    flat = h.flatten(sd, dev)
    g = torch.Generator().manual_seed(9 + N)
    feat = (torch.randn(N, 49, 2048, generator=g).abs() * 0.5).to(torch.bfloat16).to(dev)
    goal = (syn.synthetic_goal_vectors(6, (N,), goal_in, rho_max=30.0) if goal_in else syn.synthetic_goals(6, (N,))).to(dev)
    prevs = [torch.randint(0, A, (N,), generator=g).to(dev), ((torch.arange(N) * 5 + 1) % A).to(dev)] if E else [None, None]
    h0 = (torch.randn(N, 1024, generator=g) * 0.3).to(dev)
    m = (torch.rand(N, generator=g) > 0.2).float().to(dev)
    m[0] = 0.0 if N > 1 else 1.0
    ws_a = torch.empty(h.workspace_bytes(1, N, False), dtype=torch.uint8, device=dev)
    ws_b = torch.empty_like(ws_a)
    z = lambda dt=torch.float32: torch.zeros(N, dtype=dt, device=dev)
    for call, (reuse, greedy) in enumerate(((False, False), (True, False), (True, True))):
        prev = prevs[call % 2]
        hv_f, hf_f = h.forward(flat, feat, goal, h0, m, 1, N, torch.empty_like(ws_a), for_backward=False, prev_actions=prev)
        hv_f, hf_f = hv_f.clone(), hf_f.clone()
        hv_a, hf_a = h.forward(flat, feat, goal, h0, m, 1, N, ws_a, for_backward=False, reuse_tables=reuse, prev_actions=prev)
        hv_b, hf_b = torch.empty_like(hv_a), torch.empty_like(hf_a)
        act_b, lp_b, v_b = z(torch.int64), z(), z()
        narrow_entry = A + 1 <= 8 and not E and call != 1           # ec_policy_act / _vec / _greedy; else ec_policy_act_ex / _pa
        (h.act if narrow_entry else h.act_ex)(flat, feat, goal, h0, m, N, ws_b, hv_b, hf_b, act_b, lp_b, v_b, 123, 40 + call, 1000,
                                              reuse_tables=reuse, deterministic=greedy, prev_actions=prev)
        hv_sel = hv_b if A + 1 > 8 else hv_a
        act_a, lp_a, v_a = z(torch.int64), z(), z()
        if greedy:
            _lib.check(lib.ec_mode_actions(hv_sel.data_ptr(), act_a.data_ptr(), lp_a.data_ptr(), v_a.data_ptr(), N, A, 0))
        else:
            _lib.check(lib.ec_sample_actions(hv_sel.data_ptr(), act_a.data_ptr(), lp_a.data_ptr(), v_a.data_ptr(), N, A, 123, 40 + call, 1000, 0))
        torch.cuda.synchronize()
        assert torch.equal(hv_a, hv_f) and torch.equal(hf_a, hf_f)              # REUSE == a fresh EC_POLICY_INFER call
        assert torch.equal(hf_a, hf_b) and (torch.equal(hv_a, hv_b) if A + 1 <= 8 else _rel(hv_b, hv_a) < ref.FWD_TOL)
        assert torch.equal(act_a, act_b) and torch.equal(lp_a, lp_b) and torch.equal(v_a, v_b)
        assert (lp_a < 0).all() and int(act_a.max()) < A and int(act_a.min()) >= 0
    assert float(hf_a[:, 512:].abs().max()) > 0 and not torch.equal(hf_a, h0)


def test_gru_handle_is_unchanged_by_the_new_constructor(dev):
    """``PolicyHandle()`` and ``PolicyHandle(rnn_type="GRU")``: the same layout, workspace sizes and bits"""
    from embodied_clip_amd.policy import PolicyHandle
    a, b = PolicyHandle(), PolicyHandle(rnn_type="GRU")
    assert a.offsets == b.offsets and a.state_width == b.state_width == 512
    assert all(a.workspace_bytes(T, N, l) == b.workspace_bytes(T, N, l) for (T, N, l) in ((1, 32, False), (8, 16, True)))
    sd = syn.policy_state_dict(3)
    flat = a.flatten(sd, dev)
    g = torch.Generator().manual_seed(4)
    N = 5
    feat = (torch.randn(N, 49, 2048, generator=g).abs() * 0.5).to(torch.bfloat16).to(dev)
    goal, h0, m = syn.synthetic_goals(6, (N,)).to(dev), (torch.randn(N, 512, generator=g) * 0.3).to(dev), torch.ones(N, device=dev)
    outs = []
    for hd in (a, b):
        ws = torch.empty(hd.workspace_bytes(1, N, False), dtype=torch.uint8, device=dev)
        hv, hf = hd.forward(flat, feat, goal, h0, m, 1, N, ws, for_backward=False)
        outs.append((hv.clone(), hf.clone()))
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    with pytest.raises(AssertionError):                 # a GRU-width state on an LSTM handle is refused before any launch
        l = PolicyHandle(rnn_type="LSTM")
        l.forward(l.flatten(syn.policy_state_dict(3, rnn_type="LSTM"), dev), feat, goal, h0, m, 1, N,
                  torch.empty(l.workspace_bytes(1, N, False), dtype=torch.uint8, device=dev), for_backward=False)

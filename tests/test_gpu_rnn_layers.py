"""GPU: multi-layer GRU / LSTM recurrent cores through the policy's C-ABI (``PolicyHandle(rnn_layers=L)``) against the float64-checked
reference of tests/_rnn_stack_ref.py.

Cases (T, N, S, C, H, E, null, A, goal_in, L, cell) -- tests/_rnn_stack_ref.py::POLICY_CASES: two GRU layers; three LSTM layers
with a second actor block; H = 256 (the fused reverse route) with both cells; T = 1 with both cells; coordinate goals; previous
actions; 84 actions; H = 40 (a GRU whose fused step is off).  Masks have zeros at t = 0 and in the middle.

Bounds (the policy path's own): rel-L2 2e-5 forward, 2e-4 per gradient tensor; tests/test_rnn_stack_ref.py checks on the CPU that
the fp32 reference stays within a tenth of both at every case (worst 4.6e-7 / 1.4e-6).  Measured on an MI355X, worst over the
cases: forward 1.8e-6 (the values of the H = 256 LSTM case), gradients 5.9e-6 (compressor conv 1's weight) and 5.1e-6 among the
upper layers' tensors (weight_hh_l1 of the three-layer case); chained act steps against the sequence forward and the reference:
within 2e-5 on the stacked kernel and on the general route.
"""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _rnn_stack_ref as ref  # noqa: E402
from _child import GPU  # noqa: E402

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
    r = ref.policy_reference(case[10], sd, batch, case[6])
    return dict(cfg=cfg, sd=sd, **r)


def _handle(case, cfg):
    from embodied_clip_amd.policy import PolicyHandle
    return PolicyHandle(rnn_type=case[10], rnn_layers=case[9], **cfg)


def _gpu_inputs(cfg, b, dev):
    T, N = b["feat"].shape[:2]
    rows = b["feat"].permute(0, 1, 3, 4, 2).reshape(T * N, cfg["spatial"] ** 2, cfg["in_channels"]).contiguous().float().to(dev)
    goal = (b["goal"].reshape(T * N, cfg["goal_in"]).float() if cfg["goal_in"] else b["goal"].reshape(T * N)).contiguous().to(dev)
    prev = b["prev_actions"].reshape(-1).contiguous().to(dev) if cfg["prev_action_dims"] else None
    return rows, goal, prev, b["h0"][0].float().contiguous().to(dev), b["masks"].reshape(-1).float().to(dev)


def _learn_step(case, cfg, sd, b, dev, dhv_zero=False, dh_final=None):
    """forward (learn plan), PPO loss, backward twice on the GPU -> (handle, flat, hv, h_final, sums, grads, again)"""
    from embodied_clip_amd import ppo
    T, N = b["feat"].shape[:2]
    h = _handle(case, cfg)
    flat = h.flatten(sd, dev)
    rows, goal, prev, h0, m = _gpu_inputs(cfg, b, dev)
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
    T, N, H, A, L = case[0], case[1], case[4], case[7], case[9]
    c = _case(*case)
    h = _handle(case, c["cfg"])
    SW = (2 if case[10] == ref.LSTM else 1) * H
    assert h.state_width == L * SW and h.rnn_layers == L
    flat = h.flatten(c["sd"], dev)
    rows, goal, prev, h0, m = _gpu_inputs(c["cfg"], c["batch"], dev)
    ws = torch.empty(h.workspace_bytes(T, N, False), dtype=torch.uint8, device=dev)
    hv, hf = h.forward(flat, rows, goal, h0, m, T, N, ws, for_backward=False, prev_actions=prev)
    torch.cuda.synchronize()
    assert tuple(hf.shape) == (N, L * SW)
    hv = hv.view(T, N, -1)
    st = c["h"][0]
    errs = [_rel(hv[..., :A], c["logits"]), _rel(hv[..., A:], c["values"])] + [
        _rel(hf[:, l * SW:(l + 1) * SW], st[:, l * SW:(l + 1) * SW]) for l in range(L)]
    print("forward rel-L2 (logits, values, each layer's state):", errs)
    assert max(errs) < ref.FWD_TOL, errs
    # in place (h_final is h0): within the bound too (T = 1: the general route, the stacked kernel needs a row of its own)
    h0b = h0.clone()
    hv2, hf2 = h.forward(flat, rows, goal, h0b, m, T, N, ws, for_backward=False, prev_actions=prev, h_final=h0b)
    torch.cuda.synchronize()
    assert _rel(hv2.view(T, N, -1)[..., :A], c["logits"]) < ref.FWD_TOL and _rel(hf2, st) < ref.FWD_TOL
    if T > 1:
        assert torch.equal(hv2.view(T, N, -1), hv) and torch.equal(hf2, hf)


@pytest.mark.parametrize("case", CASES)
def test_optimiser_step_matches_reference_and_is_deterministic(dev, case):
    """forward, PPO loss, backward, clip, Adam: every gradient tensor, each ``_l{k}`` one included, and the parameter update; two
    backward passes and two learn passes give equal bits (no float atomics on any route of a handle with L > 1)."""
    from embodied_clip_amd import ppo
    T, N, A, L = case[0], case[1], case[7], case[9]
    c = _case(*case)
    info, ref_grads, sd, sd_ref = c["info"], c["ref_grads"], c["sd"], c["sd_ref"]
    h, flat, hv, hf, sums, grads, again = _learn_step(case, c["cfg"], sd, c["batch"], dev)
    hv3 = hv.view(T, N, -1)
    assert _rel(hv3[..., :A], c["logits"]) < ref.FWD_TOL and _rel(hv3[..., A:], c["values"]) < ref.FWD_TOL   # the learn plan's forward
    assert _rel(hf, c["h"][0]) < ref.FWD_TOL
    total = ((sums[0] + 0.5 * sums[1] + 0.01 * sums[2]) / (T * N)).item()
    assert abs(total - info["ppo_total"]) < 1e-5 * max(1.0, abs(info["ppo_total"]))
    gv = h.views(grads)
    assert set(gv) == set(ref_grads)
    for l in range(1, L):
        assert all(k in gv for k in ref.names(l))
    errs = {name: _rel(gv[name], gref) for name, gref in ref_grads.items()}
    print("gradient rel-L2:", errs)
    for name, e in errs.items():
        assert e < ref.GRAD_TOL, (name, e)
    assert torch.equal(grads, again)
    _, _, hv_b, hf_b, _, grads_b, _ = _learn_step(case, c["cfg"], sd, c["batch"], dev)
    assert torch.equal(hv_b, hv) and torch.equal(hf_b, hf) and torch.equal(grads_b, grads)
    opt = ppo.FlatAdam(flat, lr=3e-4, max_grad_norm=0.5)
    opt.step(grads)
    torch.cuda.synchronize()
    assert abs(opt.grad_norm() - info["grad_norm"]) < 1e-4 * info["grad_norm"]
    pv = h.views(flat)
    for name, pref in sd_ref.items():
        upd, upd_ref = pv[name].cpu() - sd[name], pref - sd[name]       # (the update, not the parameter)
        well = ref_grads[name].abs() > 1e-6
        assert ((upd - upd_ref).abs() * well).max() < 0.05 * 3e-4 + 1e-7, name
        assert upd.abs().max() <= 3e-4 * 1.001 + 1e-7, name


@pytest.mark.parametrize("case", [CASES[0], CASES[1], CASES[3]])
def test_dh_final_reaches_the_gradients_from_every_layer(dev, case):
    """backward(dhv = 0, dh_final) == the float64 gradients of sum(dstate * final state); zeroing any ONE layer's slice of
    dh_final changes the gradients, so every slice is read."""
    H, L = case[4], case[9]
    c = _case(*case)
    b = c["batch"]
    want = ref.state_grad_reference(case[10], c["sd"], {**b, "noise": None}, case[6])
    dstate = b["dstate"].float().contiguous().to(dev)
    h, _, _, _, _, grads, again = _learn_step(case, c["cfg"], c["sd"], b, dev, dhv_zero=True, dh_final=dstate)
    gv = h.views(grads)
    live = 0
    for name, gref in want.items():
        if float(gref.abs().max()) == 0:
            assert not gv[name].any(), name            # (the heads receive nothing)
            continue
        live += 1
        assert _rel(gv[name], gref) < ref.GRAD_TOL, (name, _rel(gv[name], gref))
    assert live >= 8 + 4 * (L - 1) and torch.equal(grads, again)
    SW = h.state_width // L
    for l in range(L):
        part = dstate.clone()
        part[:, l * SW:(l + 1) * SW] = 0
        _, _, _, _, _, g_part, _ = _learn_step(case, c["cfg"], c["sd"], b, dev, dhv_zero=True, dh_final=part)
        assert not torch.equal(g_part, grads), l


@pytest.mark.parametrize("cell", [ref.GRU, ref.LSTM])
def test_forward_does_not_depend_on_actor_slicing(dev, cell):
    """The act step of 37 actors == the act steps of actors [0, 19) and [19, 37), bit for bit, state rows included."""
    case = (1, 37, 7, 64, 32, 6, 1, 6, 0, 2, cell)
    cfg, sd, b = ref.policy_inputs(*case)
    h = _handle(case, cfg)
    flat = h.flatten(sd, dev)
    rows, goal, prev, h0, m = _gpu_inputs(cfg, b, dev)

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


def _chained(case, dev):
    """-> (rel-L2 of T chained act steps' hv from the T-step forward's, ... of the final state)"""
    T, N = case[0], case[1]
    c = _case(*case)
    h = _handle(case, c["cfg"])
    flat = h.flatten(c["sd"], dev)
    rows, goal, prev, h0, m = _gpu_inputs(c["cfg"], c["batch"], dev)
    ws = torch.empty(h.workspace_bytes(T, N, False), dtype=torch.uint8, device=dev)
    hv, hf = h.forward(flat, rows, goal, h0, m, T, N, ws, for_backward=False, prev_actions=prev)
    hv, hf = hv.clone(), hf.clone()
    ws1 = torch.empty(h.workspace_bytes(1, N, False), dtype=torch.uint8, device=dev)
    state, steps = h0, []
    for t in range(T):
        sl = slice(t * N, (t + 1) * N)
        hv_t, state = h.forward(flat, rows[sl].contiguous(), goal[sl].contiguous(), state, m[sl].contiguous(), 1, N, ws1, for_backward=False,
                                reuse_tables=t > 0, prev_actions=None if prev is None else prev[sl].contiguous())
        steps.append(hv_t.clone())
        state = state.clone()
    torch.cuda.synchronize()
    A = case[7]
    lg = c["logits"].reshape(T * N, A)
    return _rel(torch.cat(steps), hv), _rel(state, hf), _rel(torch.cat(steps)[:, :A], lg), _rel(state, c["h"][0])


@pytest.mark.parametrize("case", [CASES[0], CASES[1], CASES[2], CASES[3], CASES[9]])
def test_chained_act_steps_equal_the_sequence_forward(dev, case):
    """a T-step inference forward and T chained act steps (the stacked kernel, one launch per layer) agree within the forward
    bound, and the chained steps meet the reference within it"""
    errs = _chained(case, dev)
    print("chained act steps vs sequence forward (hv, state), vs reference (logits, state):", errs)
    assert max(errs) < ref.FWD_TOL, errs


_CHILD = """
import sys, torch
sys.path.insert(0, {tests!r})
import test_gpu_rnn_layers as t
dev = torch.device("cuda:0")
for case in (t.CASES[0], t.CASES[1], t.CASES[3]):
    errs = t._chained(case, dev)
    print("EC_RNN_STACK=0", case, errs)
    assert max(errs) < t.ref.FWD_TOL, errs
print("CHILD-OK")
"""


def test_chained_act_steps_on_the_general_route(dev, repo_root):
    """the same under EC_RNN_STACK=0 (the switch is read once per process: a child process)"""
    env = {"EC_RNN_STACK": "0", "PYTHONPATH": repo_root + os.pathsep + os.environ.get("PYTHONPATH", "")}
    out = GPU.run([sys.executable, "-c", _CHILD.format(tests=os.path.dirname(os.path.abspath(__file__)))], env=env, cwd=repo_root, limit=240)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0 and "CHILD-OK" in out.stdout


@pytest.mark.parametrize("cell", [ref.GRU, ref.LSTM])
def test_one_layer_through_the_new_constructor_is_the_old_handle(dev, cell):
    """``PolicyHandle(rnn_layers=1)`` (ec_policy_create_rnn_layers) and ec_policy_create_rnn's handle: layout, workspace sizes, bits
    of a forward, an act step and a learn pass"""
    import ctypes as C
    from embodied_clip_amd import _lib, synthetic as syn
    from embodied_clip_amd.policy import PolicyHandle
    lib = _lib.load()
    kw = dict(in_channels=64, hidden=64)
    a = PolicyHandle(rnn_type=cell, rnn_layers=1, **kw)
    b = PolicyHandle(rnn_type=cell, **kw)
    old = C.c_void_p()                                  # b's handle replaced by one from the old constructor
    _lib.check(lib.ec_policy_create_rnn(C.byref(old), C.byref(_lib.PolicyCfg(**b.cfg)), _lib.RNN_TYPES[cell]))
    lib.ec_policy_destroy(b.h)
    b.h = old
    assert a.offsets == b.offsets and a.state_width == b.state_width and lib.ec_policy_rnn_layers(old) == 1
    T, N = 3, 5
    assert all(a.workspace_bytes(t, n, l) == b.workspace_bytes(t, n, l) for (t, n, l) in ((1, 32, False), (T, N, True), (T, N, False)))
    sd = syn.policy_state_dict(3, rnn_type=cell, **kw)
    g = torch.Generator().manual_seed(4)
    feat = torch.randn(T * N, 49, 64, generator=g).abs().to(dev)
    goal = syn.synthetic_goals(6, (T * N,)).to(dev)
    h0 = (torch.randn(N, a.state_width, generator=g) * 0.3).to(dev)
    m = (torch.rand(T * N, generator=g) > 0.3).float().to(dev)
    dhv = torch.randn(T * N, 7, generator=g).to(dev)
    outs = []
    for hd in (a, b):
        flat = hd.flatten(sd, dev)
        ws = torch.empty(hd.workspace_bytes(T, N, True), dtype=torch.uint8, device=dev)
        hv, hf = hd.forward(flat, feat, goal, h0, m, T, N, ws)
        grads = hd.backward(flat, feat, m, T, N, ws, dhv, None, torch.zeros_like(flat))
        ws1 = torch.empty(hd.workspace_bytes(1, N, False), dtype=torch.uint8, device=dev)
        hv1, hf1 = hd.forward(flat, feat[:N].contiguous(), goal[:N].contiguous(), h0, m[:N].contiguous(), 1, N, ws1, for_backward=False)
        outs.append([t.clone() for t in (hv, hf, grads, hv1, hf1)])
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(*outs))

"""GPU: the pooled-embedding net through the policy's C-ABI (``PolicyHandle.pooled``) against the float64 reference of
tests/_pooled_net_ref.py, at every case of its table (T, N, D, H, ids, sensors, E, null, A, L, cell).

Bounds (the policy path's own, tests/_rnn_stack_ref.py FWD_TOL / GRAD_TOL): rel-L2 2e-5 forward, 2e-4 per gradient tensor;
tests/test_pooled_net_ref.py checks on the CPU that the fp32 evaluation of the reference stays within a tenth of both at every
case.  Also: two backward calls give equal bits; chained act steps (the new route, and EC_POOLED_ACT=0 in a child process) agree
with the sequence forward within the forward bound; sliced actors equal unsliced actors bit for bit; ``act`` equals ``forward``
followed by the stand-alone selection bit for bit (sampled, greedy, forced).

Measured on an MI355X, worst over the eight cases: forward 6.7e-7 (the values of the H = 512 LSTM x 2 case), gradients 6.2e-6
(visual_fc's weight at N = 33, H = 256) and 4.4e-6 among the recurrent tensors; chained act steps against the sequence forward
and the reference within 3.3e-7 on the new route and 2.8e-7 under EC_POOLED_ACT=0.
"""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _pooled_net_ref as ref  # noqa: E402
from _child import GPU  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = ref.POLICY_CASES


def _rel(a, b):
    return ref.rel_l2(a, b)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _case(*case):
    """Inputs and the float64 reference (forward, PPO loss, gradients), computed once per case and shared (never modified)."""
    kw, sd, batch = ref.policy_inputs(*case)
    r = ref.policy_reference(case, sd, batch)
    return dict(kw=kw, sd=sd, raw=batch, **r)


def _handle(kw):
    from embodied_clip_amd.policy import PolicyHandle
    return PolicyHandle.pooled(**kw)


def _gpu_inputs(case, b, dev):
    T, N, D = case[0], case[1], case[2]
    f = lambda t, *shape: None if t is None else t.reshape(*shape).contiguous().to(dev)
    K = sum(case[5])
    return dict(embed=f(b["embed"].float(), T * N, D), goal=f(b["goal"], T * N), sensors=f(None if b["sensors"] is None else b["sensors"].float(), T * N, K),
                prev=f(b["prev_actions"], T * N), h0=b["state0"].float().contiguous().to(dev), m=b["masks"].reshape(-1).float().to(dev))


def _forward(h, flat, x, T, N, ws, sl=None, h0=None, **kw):
    s = (lambda t: None if t is None else t[sl].contiguous()) if sl is not None else (lambda t: t)
    return h.forward(flat, s(x["embed"]), s(x["goal"]), x["h0"] if h0 is None else h0, s(x["m"]), T, N, ws, prev_actions=s(x["prev"]),
                     sensors=s(x["sensors"]), **kw)


@pytest.mark.parametrize("case", CASES)
def test_forward_matches_reference(dev, case):
    T, N, H, A, L = case[0], case[1], case[3], case[8], case[9]
    c = _case(*case)
    h = _handle(c["kw"])
    SW = (2 if case[10] == ref.LSTM else 1) * H
    assert h.state_width == L * SW
    flat = h.flatten(c["sd"], dev)
    x = _gpu_inputs(case, c["raw"], dev)
    ws = torch.empty(h.workspace_bytes(T, N, False), dtype=torch.uint8, device=dev)
    hv, hf = _forward(h, flat, x, T, N, ws, for_backward=False)
    torch.cuda.synchronize()
    hv = hv.view(T, N, -1)
    errs = [_rel(hv[..., :A], c["logits"]), _rel(hv[..., A:], c["values"])] + [
        _rel(hf[:, l * SW:(l + 1) * SW], c["state"][:, l * SW:(l + 1) * SW]) for l in range(L)]
    print("forward rel-L2 (logits, values, each layer's state):", errs)
    assert max(errs) <= ref.FWD_TOL, errs
    # in place (h_final is h0): within the bound too (T = 1: the general route, the fused step needs a row of its own)
    h0b = x["h0"].clone()
    hv2, hf2 = _forward(h, flat, x, T, N, ws, h0=h0b, for_backward=False, h_final=h0b)
    torch.cuda.synchronize()
    assert _rel(hv2.view(T, N, -1)[..., :A], c["logits"]) <= ref.FWD_TOL and _rel(hf2, c["state"]) <= ref.FWD_TOL
    if T > 1:
        assert torch.equal(hv2.view(T, N, -1), hv) and torch.equal(hf2, hf)


def _learn_step(case, c, dev):
    """forward (learn plan), PPO loss, backward twice on the GPU -> (handle, hv, h_final, sums, grads, again)"""
    from embodied_clip_amd import ppo
    T, N, A = case[0], case[1], case[8]
    h = _handle(c["kw"])
    flat = h.flatten(c["sd"], dev)
    x = _gpu_inputs(case, c["raw"], dev)
    ws = torch.empty(h.workspace_bytes(T, N, True), dtype=torch.uint8, device=dev)
    hv, hf = _forward(h, flat, x, T, N, ws)
    b = c["batch"]
    f = lambda t: t.reshape(-1).float().contiguous().to(dev)
    dhv, sums = ppo.ppo_loss_raw(hv, b["actions"].reshape(-1).to(dev), f(b["old_log_probs"]), f(b["old_values"]), f(b["returns"]),
                                 f(b["norm_adv"]), A)
    grads = torch.zeros_like(flat)
    h.backward(flat, x["embed"], x["m"], T, N, ws, dhv, None, grads)
    again = torch.zeros_like(flat)                       # the same backward once more (reads the same workspace)
    h.backward(flat, x["embed"], x["m"], T, N, ws, dhv, None, again)
    torch.cuda.synchronize()
    return h, hv, hf, sums, grads, again


@pytest.mark.parametrize("case", CASES)
def test_gradients_match_reference_and_are_deterministic(dev, case):
    """forward (learn plan), PPO loss, backward: every gradient tensor against float64; two backward calls and two learn passes
    give equal bits (no float atomics on any route of a pooled handle)."""
    T, N, A = case[0], case[1], case[8]
    c = _case(*case)
    h, hv, hf, sums, grads, again = _learn_step(case, c, dev)
    hv3 = hv.view(T, N, -1)
    assert _rel(hv3[..., :A], c["logits"]) <= ref.FWD_TOL and _rel(hv3[..., A:], c["values"]) <= ref.FWD_TOL   # the learn plan's forward
    assert _rel(hf, c["state"]) <= ref.FWD_TOL
    total = ((sums[0] + 0.5 * sums[1] + 0.01 * sums[2]) / (T * N)).item()
    assert abs(total - c["info"]["ppo_total"]) < 1e-5 * max(1.0, abs(c["info"]["ppo_total"]))
    gv = h.views(grads)
    assert set(gv) == set(c["grads"])
    errs = {name: _rel(gv[name], gref) for name, gref in c["grads"].items()}
    print("gradient rel-L2:", errs)
    for name, gref in c["grads"].items():
        assert float(gref.abs().max()) > 0, name          # every tensor receives a gradient: none is compared against zero
    for name, e in errs.items():
        assert e <= ref.GRAD_TOL, (name, e)
    assert torch.equal(grads, again)
    _, hv_b, hf_b, _, grads_b, _ = _learn_step(case, c, dev)
    assert torch.equal(hv_b, hv) and torch.equal(hf_b, hf) and torch.equal(grads_b, grads)


def _chained(case, dev):
    """-> rel-L2 of T chained act steps from the T-step forward (hv, state) and from the reference (logits, state)"""
    T, N, A = case[0], case[1], case[8]
    c = _case(*case)
    h = _handle(c["kw"])
    flat = h.flatten(c["sd"], dev)
    x = _gpu_inputs(case, c["raw"], dev)
    ws = torch.empty(h.workspace_bytes(T, N, False), dtype=torch.uint8, device=dev)
    hv, hf = _forward(h, flat, x, T, N, ws, for_backward=False)
    hv, hf = hv.clone(), hf.clone()
    ws1 = torch.empty(h.workspace_bytes(1, N, False), dtype=torch.uint8, device=dev)
    state, steps = x["h0"], []
    for t in range(T):
        hv_t, state = _forward(h, flat, x, 1, N, ws1, sl=slice(t * N, (t + 1) * N), h0=state, for_backward=False, reuse_tables=t > 0)
        steps.append(hv_t.clone())
        state = state.clone()
    torch.cuda.synchronize()
    steps = torch.cat(steps)
    return _rel(steps, hv), _rel(state, hf), _rel(steps[:, :A], c["logits"].reshape(T * N, A)), _rel(state, c["state"])


@pytest.mark.parametrize("case", CASES)
def test_chained_act_steps_equal_the_sequence_forward(dev, case):
    errs = _chained(case, dev)
    print("chained act steps vs sequence forward (hv, state), vs reference (logits, state):", errs)
    assert max(errs) <= ref.FWD_TOL, errs


_CHILD = """
import sys, torch
sys.path.insert(0, {tests!r})
import test_gpu_pooled_net as t
dev = torch.device("cuda:0")
for case in t.CASES:
    errs = t._chained(case, dev)
    print("EC_POOLED_ACT=0", case, errs)
    assert max(errs) <= t.ref.FWD_TOL, errs
print("CHILD-OK")
"""


def test_chained_act_steps_on_the_general_route(dev, repo_root):
    """the same under EC_POOLED_ACT=0 (the switch is read once per process: a child process)"""
    env = {"EC_POOLED_ACT": "0", "PYTHONPATH": repo_root + os.pathsep + os.environ.get("PYTHONPATH", "")}
    out = GPU.run([sys.executable, "-c", _CHILD.format(tests=os.path.dirname(os.path.abspath(__file__)))], env=env, cwd=repo_root, limit=240)
    print(out.stdout[-3000:], out.stderr[-2000:])
    assert out.returncode == 0 and "CHILD-OK" in out.stdout


@pytest.mark.parametrize("case", CASES)
def test_sliced_actors_equal_unsliced_actors(dev, case):
    """the act step of N actors == the act steps of actors [0, 2) and [2, N), bit for bit, state rows included"""
    N = case[1]
    c = _case(*case)
    h = _handle(c["kw"])
    flat = h.flatten(c["sd"], dev)
    x = _gpu_inputs(case, c["raw"], dev)          # (the first N rows: step 0 of the batch)

    def run(a, z):
        n = z - a
        ws = torch.empty(h.workspace_bytes(1, n, False), dtype=torch.uint8, device=dev)
        hv, hf = _forward(h, flat, x, 1, n, ws, sl=slice(a, z), h0=x["h0"][a:z].contiguous(), for_backward=False)
        return hv.clone(), hf.clone()
    cut = 2 if N <= 5 else 19
    hv, hf = run(0, N)
    hv_a, hf_a = run(0, cut)
    hv_b, hf_b = run(cut, N)
    torch.cuda.synchronize()
    assert torch.equal(hv, torch.cat([hv_a, hv_b])) and torch.equal(hf, torch.cat([hf_a, hf_b]))


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("mode", ["sample", "greedy", "forced"])
def test_act_equals_forward_plus_selection(dev, case, mode):
    """``ec_policy_act_pooled`` == ``ec_policy_forward_pooled`` at T = 1 followed by the stand-alone selection, bit for bit"""
    from embodied_clip_amd import _lib, imitation
    lib = _lib.load()
    N, A = case[1], case[8]
    c = _case(*case)
    h = _handle(c["kw"])
    flat = h.flatten(c["sd"], dev)
    x = _gpu_inputs(case, c["raw"], dev)
    sl = slice(0, N)
    ws = torch.empty(h.workspace_bytes(1, N, False), dtype=torch.uint8, device=dev)
    hv, hf = _forward(h, flat, x, 1, N, ws, sl=sl, for_backward=False)
    hv, hf = hv.clone(), hf.clone()
    seed, step, first = 12345, 7, 3
    g = torch.Generator().manual_seed(N + A)
    expert = torch.randint(0, A, (N,), generator=g).to(dev)
    emask = (torch.rand(N, generator=g) > 0.3).float().to(dev)
    a_ref = torch.empty(N, dtype=torch.int64, device=dev)
    lp_ref, v_ref = torch.empty(N, device=dev), torch.empty(N, device=dev)
    if mode == "greedy":
        _lib.check(lib.ec_mode_actions(hv.data_ptr(), a_ref.data_ptr(), lp_ref.data_ptr(), v_ref.data_ptr(), N, A, _lib.stream_ptr()))
    else:
        _lib.check(lib.ec_sample_actions(hv.data_ptr(), a_ref.data_ptr(), lp_ref.data_ptr(), v_ref.data_ptr(), N, A, seed, step, first,
                                         _lib.stream_ptr()))
        if mode == "forced":
            imitation.teacher_force(hv, expert, emask, 0.6, a_ref, lp_ref, A, seed, step, first)
    hv2 = torch.empty_like(hv)
    hf2 = torch.empty_like(hf)
    actions = torch.empty(N, dtype=torch.int64, device=dev)
    logp = torch.empty(N, device=dev)
    values = torch.empty(N, device=dev)
    s = lambda t: None if t is None else t[sl].contiguous()
    h.act(flat, s(x["embed"]), s(x["goal"]), x["h0"], s(x["m"]), N, ws, hv2, hf2, actions, logp, values, seed=seed, step=step, first_actor=first,
          deterministic=mode == "greedy", prev_actions=s(x["prev"]), sensors=s(x["sensors"]),
          expert_actions=expert if mode == "forced" else None, expert_mask=emask if mode == "forced" else None,
          force_p=0.6 if mode == "forced" else 0.0)
    torch.cuda.synchronize()
    assert torch.equal(hv2, hv) and torch.equal(hf2, hf)
    assert torch.equal(actions, a_ref) and torch.equal(logp, lp_ref) and torch.equal(values, v_ref) and torch.equal(values, hv[:, A])
    if mode == "forced":
        assert bool((actions[emask > 0] == expert[emask > 0]).float().mean() > 0.2)

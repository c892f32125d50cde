"""GPU: the two-view rearrangement net through the policy's C-ABI (``PolicyHandle.two_view``) against the float64 reference of
tests/_two_view_ref.py, at every case of its table (T, N, S2, C, H, E, A, L, cell) -- T x N of 1 x 5, 4 x 3 and 3 x 33 with
episode resets in the masks; GRU and LSTM; one and two layers; E = 0, 6 and 96 (above 64: the table and its chain on
ec_gemm_f32); 6 and 84 actions -- under the PPO loss and under the imitation loss.

Bounds (the policy path's own, tests/_rnn_stack_ref.py FWD_TOL / GRAD_TOL): rel-L2 2e-5 forward, 2e-4 per gradient tensor.  The
gradient of visual_attention.2.bias is analytically ZERO (softmax is shift-invariant), so it is held to
|g| <= GRAD_TOL * ||grad visual_attention.2.weight|| instead; under the imitation loss the critic receives no gradient at all and
must come out exactly zero.  Also: two backward calls and two learn passes give equal bits; sliced actors equal unsliced actors
bit for bit; ``act`` equals ``forward`` followed by the stand-alone selection bit for bit (sampled, greedy, forced); chained act
steps equal the sequence forward within FWD_TOL.

Measured on an MI355X, worst over the six cases: forward 2.6e-7 (the values of the 4 x 3 LSTM x 2 case), gradients 5.7e-6 under the
PPO loss (visual_attention.0.bias at 3 x 33) and 4.8e-6 under the imitation loss, 4.6e-6 for prev_action_embedder.weight at
E = 96 (the ec_gemm_f32 chain); |grad visual_attention.2.bias| at most 3.7e-7 of its neighbour's norm; chained act steps within
1.6e-7 of the sequence forward and of the reference.
"""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _two_view_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = ref.POLICY_CASES


def _rel(a, b):
    return ref.rel_l2(a, b)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _inputs(*case):
    return ref.policy_inputs(*case)


@functools.lru_cache(maxsize=None)
def _case(loss, *case):
    """Inputs and the float64 reference (forward, loss, gradients), computed once per (case, loss) and shared (never modified)."""
    kw, sd, batch = _inputs(*case)
    r = ref.policy_reference(case, sd, batch, loss)
    return dict(kw=kw, sd=sd, raw=batch, **r)


def _handle(kw):
    from embodied_clip_amd.policy import PolicyHandle
    return PolicyHandle.two_view(**kw)


def _gpu_inputs(case, b, dev):
    T, N, S2, C = case[:4]
    f = lambda t, *shape: None if t is None else t.reshape(*shape).contiguous().to(dev)
    return dict(u=f(b["u"].to(torch.bfloat16), T * N, S2, C), w=f(b["w"].to(torch.bfloat16), T * N, S2, C), prev=f(b["prev_actions"], T * N),
                h0=b["state0"].float().contiguous().to(dev), m=b["masks"].reshape(-1).float().to(dev))


def _forward(h, flat, x, T, N, ws, sl=None, h0=None, **kw):
    s = (lambda t: None if t is None else t[sl].contiguous()) if sl is not None else (lambda t: t)
    return h.forward(flat, s(x["u"]), None, x["h0"] if h0 is None else h0, s(x["m"]), T, N, ws, feat2=s(x["w"]), prev_actions=s(x["prev"]),
                     **kw)


@pytest.mark.parametrize("case", CASES)
def test_forward_matches_reference(dev, case):
    T, N, H, A, L = case[0], case[1], case[4], case[6], case[7]
    c = _case("ppo", *case)
    h = _handle(c["kw"])
    SW = (2 if case[8] == ref.LSTM else 1) * H
    assert h.state_width == L * SW
    flat = h.flatten(c["sd"], dev)
    x = _gpu_inputs(case, c["raw"], dev)
    ws = torch.empty(h.workspace_bytes(T, N, False), dtype=torch.uint8, device=dev)
    hv, hf = _forward(h, flat, x, T, N, ws, for_backward=False)
    torch.cuda.synchronize()
    hv = hv.view(T, N, -1)
    errs = [_rel(hv[..., :A], c["logits"]), _rel(hv[..., A:], c["values"])] + [
        _rel(hf[:, l * SW:(l + 1) * SW], c["state"][:, l * SW:(l + 1) * SW]) for l in range(L)]
    print(case, "forward rel-L2 (logits, values, each layer's state):", errs)
    assert max(errs) <= ref.FWD_TOL, errs
    # in place (h_final is h0): within the bound too (T = 1: the general route, the fused step needs a row of its own)
    h0b = x["h0"].clone()
    hv2, hf2 = _forward(h, flat, x, T, N, ws, h0=h0b, for_backward=False, h_final=h0b)
    torch.cuda.synchronize()
    assert _rel(hv2.view(T, N, -1)[..., :A], c["logits"]) <= ref.FWD_TOL and _rel(hf2, c["state"]) <= ref.FWD_TOL


def _learn_step(case, c, loss, dev):
    """forward (learn plan), the loss, backward twice on the GPU -> (handle, hv, h_final, total, grads, again)"""
    from embodied_clip_amd import imitation, ppo
    T, N, A = case[0], case[1], case[6]
    h = _handle(c["kw"])
    flat = h.flatten(c["sd"], dev)
    x = _gpu_inputs(case, c["raw"], dev)
    ws = torch.empty(h.workspace_bytes(T, N, True), dtype=torch.uint8, device=dev)
    hv, hf = _forward(h, flat, x, T, N, ws)
    b = c["batch"]
    f = lambda t: t.reshape(-1).float().contiguous().to(dev)
    if loss == "ppo":
        dhv, sums = ppo.ppo_loss_raw(hv, b["actions"].reshape(-1).to(dev), f(b["old_log_probs"]), f(b["old_values"]), f(b["returns"]),
                                     f(b["norm_adv"]), A)
        total = lambda: ((sums[0] + 0.5 * sums[1] + 0.01 * sums[2]) / (T * N)).item()
    else:
        dhv, sums = imitation.imitation_loss_raw(hv, b["expert"].reshape(-1).to(dev), f(b["emask"]), A)
        total = lambda: (sums[0] / sums[1]).item()
    grads = torch.zeros_like(flat)
    h.backward(flat, x["u"], x["m"], T, N, ws, dhv, None, grads, feat2=x["w"])
    again = torch.zeros_like(flat)                       # the same backward once more (reads the same workspace)
    h.backward(flat, x["u"], x["m"], T, N, ws, dhv, None, again, feat2=x["w"])
    torch.cuda.synchronize()
    return h, hv, hf, total(), grads, again


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("loss", ref.LOSSES)
def test_gradients_match_reference_and_are_deterministic(dev, case, loss):
    """forward (learn plan), loss, backward: every gradient tensor against float64; two backward calls and two learn passes give
    equal bits (no float atomics on any route of the handle)."""
    T, N, A = case[0], case[1], case[6]
    c = _case(loss, *case)
    h, hv, hf, total, grads, again = _learn_step(case, c, loss, dev)
    hv3 = hv.view(T, N, -1)
    assert _rel(hv3[..., :A], c["logits"]) <= ref.FWD_TOL and _rel(hv3[..., A:], c["values"]) <= ref.FWD_TOL   # the learn plan's forward
    assert _rel(hf, c["state"]) <= ref.FWD_TOL
    assert abs(total - c["total"]) < 1e-5 * max(1.0, abs(c["total"])), (total, c["total"])
    gv = h.views(grads)
    assert set(gv) == set(c["grads"])
    errs = {}
    for name, gref in c["grads"].items():
        if name == ref.B2:      # analytically zero: against the scale of the neighbouring tensor
            errs[name] = float(gv[name].double().abs().max().cpu() / c["grads"][ref.W2].norm())
        elif float(gref.abs().max()) == 0.0:
            assert loss == "imitation" and name.startswith("critic."), name     # (no value term: nothing else is compared against zero)
            assert float(gv[name].abs().max()) == 0.0, name
        else:
            errs[name] = _rel(gv[name], gref)
    print(case, loss, "gradient rel-L2:", {k: "%.3e" % e for k, e in errs.items()})
    for name, e in errs.items():
        assert e <= ref.GRAD_TOL, (name, e)
    assert torch.equal(grads, again)
    _, hv_b, hf_b, _, grads_b, _ = _learn_step(case, c, loss, dev)
    assert torch.equal(hv_b, hv) and torch.equal(hf_b, hf) and torch.equal(grads_b, grads)


@pytest.mark.parametrize("case", CASES)
def test_chained_act_steps_equal_the_sequence_forward(dev, case):
    T, N, A = case[0], case[1], case[6]
    c = _case("ppo", *case)
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
    errs = (_rel(steps, hv), _rel(state, hf), _rel(steps[:, :A], c["logits"].reshape(T * N, A)), _rel(state, c["state"]))
    print(case, "chained act steps vs sequence forward (hv, state), vs reference (logits, state):", errs)
    assert max(errs) <= ref.FWD_TOL, errs


@pytest.mark.parametrize("case", CASES)
def test_sliced_actors_equal_unsliced_actors(dev, case):
    """the act step of N actors == the act steps of actors [0, cut) and [cut, N), bit for bit, state rows included"""
    N = case[1]
    c = _case("ppo", *case)
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
    """``ec_policy_act_two_view`` == ``ec_policy_forward_two_view`` at T = 1 followed by the stand-alone selection, bit for bit"""
    from embodied_clip_amd import _lib, imitation
    lib = _lib.load()
    N, A = case[1], case[6]
    c = _case("ppo", *case)
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
    h.act(flat, s(x["u"]), None, x["h0"], s(x["m"]), N, ws, hv2, hf2, actions, logp, values, seed=seed, step=step, first_actor=first,
          deterministic=mode == "greedy", feat2=s(x["w"]), prev_actions=s(x["prev"]),
          expert_actions=expert if mode == "forced" else None, expert_mask=emask if mode == "forced" else None,
          force_p=0.6 if mode == "forced" else 0.0)
    torch.cuda.synchronize()
    assert torch.equal(hv2, hv) and torch.equal(hf2, hf)
    assert torch.equal(actions, a_ref) and torch.equal(logp, lp_ref) and torch.equal(values, v_ref) and torch.equal(values, hv[:, A])

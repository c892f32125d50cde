"""GPU: ``ResNetRearrangeActorCriticRNN`` -- the AllenAct drop-in over ``PolicyHandle.two_view`` -- fed as AllenAct feeds it: two
fp32 NCHW feature tensors ``[T, N, C, s, s]``, upstream's recurrent memory, the plugin losses on its output.  Cases of
tests/_two_view_ref.py (T, N, S2, C, H, E, A, L, cell): 4 x 3 with E = 96 = H and 84 actions on a two-layer LSTM; 3 x 33 with 3 x 3
maps of 192 channels; 3 x 33 on a two-layer GRU; 1 x 5 without previous actions.

Bounds (the policy path's own, tests/_rnn_stack_ref.py): rel-L2 FWD_TOL = 2e-5 forward, GRAD_TOL = 2e-4 per gradient tensor by
``_two_view_ref.grad_errors`` (``visual_attention.2.bias``, analytically zero, against ``GRAD_TOL * ||grad visual_attention.2.weight||``).
The class adds NO arithmetic to the handle: its output equals the handle's on the bf16 rows bit for bit.

Measured on an MI355X, worst over the four cases: forward 2.6e-7 (the values of the 4 x 3 LSTM x 2 case); gradients 5.6e-6 through
PPO().loss (visual_attention.0.bias at 3 x 33, 3 x 3 maps) and 4.9e-6 through Imitation().loss (visual_encoder.0.weight at 3 x 33,
GRU x 2; the critic's exactly zero); |grad visual_attention.2.bias| at most 2.8e-7 of its neighbour's norm; chained no_grad act
steps within 2.0e-7 of the sequence forward and of the reference."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _two_view_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = [(4, 3, 49, 64, 96, 96, 84, 2, ref.LSTM), (3, 33, 9, 192, 96, 6, 6, 1, ref.LSTM), (3, 33, 49, 64, 32, 6, 84, 2, ref.GRU),
         (1, 5, 49, 64, 64, 0, 6, 1, ref.GRU)]
assert all(c in ref.POLICY_CASES for c in CASES)
LEARN = [c for c in CASES if c[0] > 1]
RGB, UNSHUFFLED = "rgb_clip", "unshuffled_rgb_clip"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _case(loss, *case):
    """Inputs and the float64 reference (forward, loss, gradients), computed once per (case, loss) and shared (never modified)."""
    kw, sd, batch = ref.policy_inputs(*case)
    return dict(kw=kw, sd=sd, raw=batch, **ref.policy_reference(case, sd, batch, loss))


def _nchw(rows, case):
    """[T, N, S2, C] -> fp32 [T, N, C, s, s]"""
    T, N, S2, C = case[:4]
    s = int(round(S2 ** 0.5))
    return rows.float().view(T, N, s, s, C).permute(0, 1, 4, 2, 3).contiguous()


def _model(case, sd, dev, **kw):
    from embodied_clip_amd import spaces
    from embodied_clip_amd.policy import ResNetRearrangeActorCriticRNN
    T, N, S2, C, H, E, A, L, cell = case
    s = int(round(S2 ** 0.5))
    obs = spaces.Dict({RGB: spaces.Box(-1e9, 1e9, (C, s, s)), UNSHUFFLED: spaces.Box(-1e9, 1e9, (C, s, s))})
    return ResNetRearrangeActorCriticRNN(spaces.Discrete(A), obs, RGB, UNSHUFFLED, hidden_size=H, num_rnn_layers=L, rnn_type=cell,
                                         prev_action_embedding_dim=E, state_dict=sd, device=dev, **kw)


def _feed(case, raw, dev):
    """what AllenAct hands the model: (observations, memory factory, prev_actions, masks)"""
    from embodied_clip_amd.policy import Memory, state_to_memory
    L, cell = case[7], case[8]
    obs = {RGB: _nchw(raw["u"], case).to(dev), UNSHUFFLED: _nchw(raw["w"], case).to(dev)}
    mem0 = state_to_memory(raw["state0"].float(), cell, L).to(dev)
    prev = None if raw["prev_actions"] is None else raw["prev_actions"].to(dev)
    return obs, (lambda: Memory().check_append("rnn", mem0.clone(), 1)), prev, raw["masks"].to(dev)     # (set_tensor updates its object)


def _handle_rows(case, raw, dev):
    T, N, S2, C = case[:4]
    f = lambda t: t.to(torch.bfloat16).reshape(T * N, S2, C).contiguous().to(dev)
    prev = None if raw["prev_actions"] is None else raw["prev_actions"].reshape(-1).to(dev)
    return f(raw["u"]), f(raw["w"]), prev, raw["state0"].float().contiguous().to(dev), raw["masks"].reshape(-1).float().to(dev)


@pytest.mark.parametrize("case", CASES)
def test_forward_matches_reference(dev, case):
    from embodied_clip_amd.policy import state_to_memory
    T, N, S2, C, H, E, A, L, cell = case
    c = _case("ppo", *case)
    model = _model(case, c["sd"], dev)
    assert model.num_recurrent_layers == L * (2 if cell == ref.LSTM else 1) and model.recurrent_hidden_state_size == H
    assert model.recurrent_memory_specification["rnn"][0] == (("layer", model.num_recurrent_layers), ("sampler", None), ("hidden", H))
    obs, mem, prev, masks = _feed(case, c["raw"], dev)
    for grad in (True, False):
        with torch.set_grad_enabled(grad):
            out, mem2 = model(obs, mem(), prev, masks)
        errs = (ref.rel_l2(out.distributions.logits, torch.log_softmax(c["logits"], -1)), ref.rel_l2(out.values, c["values"]),
                ref.rel_l2(mem2.tensor("rnn"), state_to_memory(c["state"], cell, L)))
        print(case, "grad" if grad else "no_grad", "forward rel-L2 (log-probabilities, values, memory):", errs)
        assert out.values.shape == (T, N, 1) and out.distributions.logits.shape == (T, N, A)
        assert max(errs) <= ref.FWD_TOL, errs


def _plugin_loss(loss, c, out, dev):
    from embodied_clip_amd.imitation import Imitation
    from embodied_clip_amd.ppo import PPO
    b = c["batch"]
    f = lambda t: t.float().to(dev)
    if loss == "imitation":
        batch = dict(observations=dict(expert_action=torch.stack([b["expert"].float(), b["emask"].float()], -1).to(dev)))
        return Imitation().loss(0, batch, out)[0]
    batch = dict(actions=b["actions"].to(dev), old_action_log_probs=f(b["old_log_probs"]), values=f(b["old_values"]),
                 returns=f(b["returns"]), norm_adv_targ=f(b["norm_adv"]), adv_targ=f(b["norm_adv"]))
    return PPO().loss(0, batch, out)[0]


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("loss", ref.LOSSES)
def test_gradients_through_the_plugin_losses_match_reference(dev, case, loss):
    c = _case(loss, *case)
    model = _model(case, c["sd"], dev)
    obs, mem, prev, masks = _feed(case, c["raw"], dev)
    out, _ = model(obs, mem(), prev, masks)
    total = _plugin_loss(loss, c, out, dev)
    total.backward()
    assert abs(float(total.detach()) - c["total"]) < 1e-5 * max(1.0, abs(c["total"])), (float(total.detach()), c["total"])
    got = {n: p.grad for n, p in model.named_parameters()}
    assert set(got) == set(c["grads"]) and all(g is not None for g in got.values())
    errs = ref.grad_errors(got, c["grads"])
    print(case, loss, "gradient rel-L2:", {k: "%.3e" % e for k, e in errs.items()})
    for name, e in errs.items():
        assert e <= ref.GRAD_TOL, (name, e)
    flat = model.flat_grads                                  # every .grad is a view of the one flat bucket
    assert all(p.grad.data_ptr() == flat.data_ptr() + 4 * off for (_, p), (off, _) in zip(model._named(), model.handle.offsets.values()))


@pytest.mark.parametrize("case", CASES)
def test_the_bridge_adds_no_arithmetic(dev, case):
    """hv and the final state == the handle's on the bf16 rows with the same flat parameters, bit for bit, with grad and without"""
    from embodied_clip_amd.policy import CategoricalDistr
    T, N, A = case[0], case[1], case[6]
    c = _case("ppo", *case)
    model = _model(case, c["sd"], dev)
    obs, mem, prev, masks = _feed(case, c["raw"], dev)
    u, w, prev_rows, h0, m = _handle_rows(case, c["raw"], dev)
    h = model.handle
    for grad in (True, False):
        ws = torch.empty(h.workspace_bytes(T, N, grad), dtype=torch.uint8, device=dev)
        hv, hf = h.forward(model.flat_params, u, None, h0, m, T, N, ws, for_backward=grad, feat2=w, prev_actions=prev_rows)
        hv = hv.view(T, N, A + 1)
        with torch.set_grad_enabled(grad):
            out, mem2 = model(obs, mem(), prev, masks)
        assert torch.equal(out.values, hv[..., A:])
        assert torch.equal(out.distributions.logits, CategoricalDistr(logits=hv[..., :A]).logits)
        assert torch.equal(mem2.tensor("rnn"), h.state_to_memory(hf))


@pytest.mark.parametrize("case", LEARN)
def test_chained_no_grad_act_steps_equal_the_sequence_forward(dev, case):
    from embodied_clip_amd.policy import state_to_memory
    T, N, A, L, cell = case[0], case[1], case[6], case[7], case[8]
    c = _case("ppo", *case)
    model = _model(case, c["sd"], dev)
    obs, mem, prev, masks = _feed(case, c["raw"], dev)
    memory, logp, values = mem(), [], []
    with torch.no_grad():
        seq, seq_mem = model(obs, mem(), prev, masks)
        for t in range(T):
            out, memory = model({k: v[t:t + 1] for k, v in obs.items()}, memory, None if prev is None else prev[t:t + 1], masks[t:t + 1])
            out.distributions.sample()
            logp.append(out.distributions.logits)
            values.append(out.values)
    model.check_features()                                   # bf16-valued features: nothing to report after the act steps
    logp, values = torch.cat(logp), torch.cat(values)
    errs = (ref.rel_l2(logp, seq.distributions.logits), ref.rel_l2(values, seq.values), ref.rel_l2(memory.tensor("rnn"), seq_mem.tensor("rnn")),
            ref.rel_l2(logp, torch.log_softmax(c["logits"], -1)), ref.rel_l2(memory.tensor("rnn"), state_to_memory(c["state"], cell, L)))
    print(case, "chained act steps vs sequence forward (log-probabilities, values, memory), vs reference:", errs)
    assert max(errs) <= ref.FWD_TOL, errs


@pytest.mark.parametrize("case", CASES[:2])
def test_checkpoint_exchange(dev, case):
    from embodied_clip_amd import synthetic as syn
    from embodied_clip_amd.policy import two_view_param_shapes
    c = _case("ppo", *case)
    model = _model(case, c["sd"], dev)
    shapes = two_view_param_shapes(**c["kw"])
    sd = model.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(s) for k, s in shapes.items()}
    assert [n for n, _ in model._named()] == list(shapes)    # (the flat order; state_dict() walks the module tree)
    net = ref.TwoViewNet(**c["kw"])
    net.load_state_dict({k: v.cpu() for k, v in sd.items()}, strict=True)
    assert all(torch.equal(v, c["sd"][k]) for k, v in net.state_dict().items())

    def is_flat():
        flat = model.flat_params
        return all(p.data_ptr() == flat.data_ptr() + 4 * off and p.device == flat.device
                   for (_, p), (off, _) in zip(model._named(), model.handle.offsets.values()))

    assert is_flat()
    # other values, as a checkpoint of upstream's model or of Worker(net="two_view") would bring them
    other = syn.policy_state_dict(99, two_view=c["kw"])
    model.load_state_dict(other, strict=True)
    assert is_flat()
    model.to(dev)
    assert is_flat()
    obs, mem, prev, masks = _feed(case, c["raw"], dev)
    with torch.no_grad():
        out, _ = model(obs, mem(), prev, masks)
    r = ref.policy_reference(case, other, c["raw"], "ppo")
    assert ref.rel_l2(out.distributions.logits, torch.log_softmax(r["logits"], -1)) <= ref.FWD_TOL
    assert ref.rel_l2(out.values, r["values"]) <= ref.FWD_TOL
    assert ref.rel_l2(out.values, c["values"]) > 1e-3        # (and not the old ones)


def test_rows_cache(dev):
    """learn-pass forwards on one storage version convert once; an in-place write converts anew; act steps leave the cache alone"""
    case = CASES[0]
    T, N = case[:2]
    c = _case("ppo", *case)
    model = _model(case, c["sd"], dev)
    obs, mem, prev, masks = _feed(case, c["raw"], dev)
    storage = {k: torch.zeros(T + 1, *v.shape[1:], device=dev) for k, v in obs.items()}      # a rollout storage: views of it come in
    for k, v in obs.items():
        storage[k][:T] = v
    view = lambda: {k: v[:T] for k, v in storage.items()}
    out1, _ = model(view(), mem(), prev, masks)
    rows = model._rows_cache[3], model._rows_cache[4]
    assert rows[0].dtype == torch.bfloat16 and rows[0].shape == (T * N, case[2], case[3])
    out2, _ = model(view(), mem(), prev, masks)
    assert model._rows_cache[3] is rows[0] and model._rows_cache[4] is rows[1]
    assert torch.equal(out1.values, out2.values)
    with torch.no_grad():
        model({k: v[:1] for k, v in storage.items()}, mem(), None if prev is None else prev[:1], masks[:1])
    assert model._rows_cache[3] is rows[0] and model._rows_cache[4] is rows[1]
    storage[UNSHUFFLED][0, 0, 0, 0, 0] = 2.0                  # a bf16 value, and a new storage version
    out3, _ = model(view(), mem(), prev, masks)
    assert model._rows_cache[4] is not rows[1] and model._rows_cache[4][0, 0, 0] == 2.0
    out3.values.sum().backward()                              # (the cached rows feed the backward)
    assert all(p.grad is not None for p in model.parameters())


def test_rounding_rule(dev):
    case = CASES[0]
    c = _case("ppo", *case)
    obs, mem, prev, masks = _feed(case, c["raw"], dev)
    off = {k: v.clone() for k, v in obs.items()}
    off[UNSHUFFLED][1, 2, 3, 4, 5] += 1e-3                    # one value of the unshuffled view off the bf16 grid
    assert not torch.equal(off[UNSHUFFLED].to(torch.bfloat16).float(), off[UNSHUFFLED])
    model = _model(case, c["sd"], dev)
    with pytest.raises(ValueError) as e:
        model(off, mem(), prev, masks)
    assert RGB in str(e.value) and UNSHUFFLED in str(e.value) and "nearest" in str(e.value)
    model.check_features()                                    # (reported once: the check cleared the flag)
    with torch.no_grad():                                     # an act step on such values runs ...
        model({k: v[1:2] for k, v in off.items()}, mem(), None if prev is None else prev[1:2], masks[1:2])
    with pytest.raises(ValueError) as e:                      # ... and the next check reports it
        model.check_features()
    assert RGB in str(e.value) and UNSHUFFLED in str(e.value)
    out, _ = model(obs, mem(), prev, masks)                   # clean features afterwards: served
    nearest = _model(case, c["sd"], dev, feature_rounding="nearest")
    got, _ = nearest(off, mem(), prev, masks)
    rounded = {k: v.to(torch.bfloat16).float() for k, v in off.items()}
    want, _ = nearest(rounded, mem(), prev, masks)
    assert torch.equal(got.values, want.values) and torch.equal(got.distributions.logits, want.distributions.logits)
    assert not torch.equal(rounded[UNSHUFFLED], obs[UNSHUFFLED])
    nearest.check_features()                                  # never reads the flag, never raises


@pytest.mark.parametrize("case", CASES[:2])
def test_channels_last_input(dev, case):
    T, N, S2, C = case[:4]
    s = int(round(S2 ** 0.5))
    c = _case("ppo", *case)
    model = _model(case, c["sd"], dev)
    obs, mem, prev, masks = _feed(case, c["raw"], dev)
    with torch.no_grad():
        want, wmem = model(obs, mem(), prev, masks)
        for dtype in (torch.bfloat16, torch.float32):
            last = {RGB: c["raw"]["u"].view(T, N, s, s, C).to(dtype).to(dev), UNSHUFFLED: c["raw"]["w"].view(T, N, s, s, C).to(dtype).to(dev)}
            got, gmem = model(last, mem(), prev, masks)
            assert torch.equal(got.values, want.values) and torch.equal(got.distributions.logits, want.distributions.logits)
            assert torch.equal(gmem.tensor("rnn"), wmem.tensor("rnn"))

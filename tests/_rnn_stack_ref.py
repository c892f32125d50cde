"""Float64 reference, case tables and seeded inputs of the multi-layer recurrent cores (test infrastructure only; used by
tests/test_rnn_stack_ref.py on the CPU and the tests/test_gpu_rnn_*.py modules).

Plain torch, dtype-generic.  The cells are imported, not copied: the GRU cell is oracle.policy.gru_cell, the LSTM cell
tests/_lstm_ref.py's, the goal encoders and the previous-action embedding what _lstm_ref.py imports.  The stack restates
torch.nn.GRU / torch.nn.LSTM with num_layers = L and dropout = 0 under [U] allenact RNNStateEncoder's mask (not under the
reference tree: parity unpinned; tests/test_rnn_stack_ref.py holds the stack to torch.nn.GRU / nn.LSTM itself):

  * layer 0 takes the encoder's x, layer l >= 1 takes x = h^{l-1}_t;
  * the episode mask multiplies the previous state (h, and c on the LSTM) of EVERY layer, never a layer's input;
  * the heads read the top layer's h.

State convention (include/ec_amd.h): an actor's state is ONE row of width L * SW, layer-major -- [h^0 | h^1 | ...] (GRU) or
[h^0 | c^0 | h^1 | c^1 | ...] (LSTM).  Upstream's memory is [L, N, H] (GRU) or [2L, N, H] = torch.cat([h, c], 0) (LSTM).

Run as a program (CPU only), this file prints what the bounds of the GPU tests are held against:

    python tests/_rnn_stack_ref.py
"""
import contextlib
import os
import sys
from unittest import mock

import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import _lstm_ref as lstm_ref  # noqa: E402
import _prev_action_ref as pa_ref  # noqa: E402

rel_l2 = pa_ref.rel_l2
EMB_KEY = pa_ref.EMB_KEY
FWD_TOL, GRAD_TOL = lstm_ref.FWD_TOL, lstm_ref.GRAD_TOL      # the policy path's own: 2e-5 forward, 2e-4 per gradient tensor
GRU, LSTM = "GRU", "LSTM"


def names(l):
    """(weight_ih, weight_hh, bias_ih, bias_hh) of layer l"""
    return tuple(f"state_encoder.rnn.{k}_l{l}" for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))


def num_layers(sd):
    L = 1
    while names(L)[0] in sd:
        L += 1
    return L


# ---- state layouts ------------------------------------------------------------------------------------------------------------
def memory_to_state(mem, cell, L):
    """[L, N, H] | [2L, N, H] (all h layers, then all c layers) -> [N, L * SW] layer-major rows"""
    k = 2 if cell == LSTM else 1
    _, N, H = mem.shape
    cols = []
    for l in range(L):
        cols.append(mem[l])
        if k == 2:
            cols.append(mem[L + l])
    return torch.cat(cols, dim=-1).contiguous()


def state_to_memory(state, cell, L):
    k = 2 if cell == LSTM else 1
    H = state.shape[1] // (k * L)
    parts = state.split(H, dim=-1)
    hs = [parts[k * l] for l in range(L)]
    cs = [parts[k * l + 1] for l in range(L)] if k == 2 else []
    return torch.stack(hs + cs, 0).contiguous()


# ---- one layer's step, both cells ------------------------------------------------------------------------------------------------
def layer_step(cell, x, state_prev, m, wih, whh, bih, bhh):
    """One step of one layer.  x [N, I]; state_prev [N, SW] ([h] or [h | c]); m [N] masks the previous state only.
    -> the layer's new state [N, SW] (its h is [:, :H])"""
    from oracle import policy as opol
    H = whh.shape[1]
    mm = m.reshape(-1, 1).to(x.dtype)
    if cell == GRU:
        return opol.gru_cell(x, mm * state_prev, wih, whh, bih, bhh)
    h, c, _, _ = lstm_ref.cell(F.linear(x, wih, bih), state_prev[:, :H], state_prev[:, H:], m, whh, bhh)
    return torch.cat([h, c], dim=-1)


def stack_step(cell, x, state, m, sd, L=None, wrong=None):
    """One time step of the whole stack.  state [N, L * SW] -> (top h [N, H], new state).  `wrong`: a deliberately wrong variant
    (tests/test_rnn_stack_ref.py): "mask_x" | "skip_layer" | "xn_inside" | "swap_hc" | "drop_bih"."""
    L = L or num_layers(sd)
    H = sd[names(0)[1]].shape[1]
    SW = (2 if cell == LSTM else 1) * H
    outs, hs = [], []
    inp = x
    for l in range(L):
        wih, whh, bih, bhh = (sd[k] for k in names(l))
        prev = state[:, l * SW:(l + 1) * SW]
        if l and wrong == "mask_x":
            inp = m.reshape(-1, 1).to(x.dtype) * inp
        if l == 2 and wrong == "skip_layer":
            inp = hs[0]
        if l and wrong == "drop_bih":
            bih = torch.zeros_like(bih)
        if l and wrong == "swap_hc" and cell == LSTM:
            prev = torch.cat([prev[:, H:], prev[:, :H]], dim=-1)
        if l and wrong == "xn_inside" and cell == GRU:
            new = _gru_xn_inside(inp, m.reshape(-1, 1).to(x.dtype) * prev, wih, whh, bih, bhh)
        else:
            new = layer_step(cell, inp, prev, m, wih, whh, bih, bhh)
        outs.append(new)
        inp = new[:, :H]
        hs.append(inp)
    return inp, torch.cat(outs, dim=-1)


def _gru_xn_inside(x, h, w_ih, w_hh, b_ih, b_hh):
    """WRONG on purpose: n = tanh(r * (x_n + h_n)) -- the input's n part inside the reset gate's product"""
    gi, gh = F.linear(x, w_ih, b_ih), F.linear(h, w_hh, b_hh)
    i_r, i_z, i_n = gi.chunk(3, -1)
    h_r, h_z, h_n = gh.chunk(3, -1)
    r, z = torch.sigmoid(i_r + h_r), torch.sigmoid(i_z + h_z)
    n = torch.tanh(r * (i_n + h_n))
    return (1 - z) * n + z * h


def sequence(cell, x, state0, masks, sd, wrong=None):
    """RNNStateEncoder over x [T, N, I] from state rows [N, L * SW]; masks [T, N, 1].  -> (top h [T, N, H], state [N, L * SW])"""
    state, outs = state0, []
    for t in range(x.shape[0]):
        top, state = stack_step(cell, x[t], state, masks[t].reshape(-1), sd, wrong=wrong)
        outs.append(top)
    return torch.stack(outs, 0), state


# ---- the model ----------------------------------------------------------------------------------------------------------------
def actor_critic_forward(cell, feat, goal, prev_actions, state0, masks, sd, null, wrong=None):
    """goal encoder -> [+ previous-action embedding] -> L-layer core -> heads: (logits, values, state [1, N, L * SW])"""
    from oracle import policy as opol
    T, N = feat.shape[:2]
    A = sd["actor.linear.weight"].shape[0]
    if goal.is_floating_point():
        import _pointnav_ref
        x = _pointnav_ref.goal_encoder(feat.reshape(T * N, *feat.shape[2:]), goal.reshape(T * N, -1), sd)
    else:
        x = opol.goal_encoder(feat.reshape(T * N, *feat.shape[2:]), goal.reshape(T * N), sd)
    x = x.view(T, N, -1)
    if EMB_KEY in sd:
        x = pa_ref.recurrent_input(x, prev_actions, masks, sd[EMB_KEY], null, A)
    out, state = sequence(cell, x, state0[0], masks, sd, wrong=wrong)
    logits = F.linear(out, sd["actor.linear.weight"], sd["actor.linear.bias"])
    values = F.linear(out, sd["critic.fc.weight"], sd["critic.fc.bias"])
    return logits, values, state.unsqueeze(0)


@contextlib.contextmanager
def as_oracle_policy(cell, prev_actions, null):
    """Puts the forward above in oracle.policy.actor_critic_forward's place, so that oracle.ppo.ppo_update_step serves unchanged"""
    from oracle import policy as opol

    def forward(feat, goal, h0, masks, sd):
        return actor_critic_forward(cell, feat, goal, prev_actions, h0, masks, sd, null)
    with mock.patch.object(opol, "actor_critic_forward", forward):
        yield


# ---- the kernel tests' cases (ec_rnn_stack_step_fwd alone) ------------------------------------------------------------------------
# (N, H): one lane row, whole-K staging | a second actor block holding one row | twelve unit blocks, whole-K | one LDS-DMA chunk
# per half | two chunks per half, the reference width
KERNEL_CASES = [(1, 32), (33, 64), (3, 96), (5, 256), (37, 512)]
KERNEL_MASKS = ("ones", "zeros", "mixed")


def kernel_mask(N, kind):
    if kind == "ones":
        return torch.ones(N)
    if kind == "zeros":
        return torch.zeros(N)
    return (torch.arange(N) % 3 != 1).float() if N > 1 else torch.zeros(1)


def kernel_inputs(cell, N, H):
    """fp32 inputs of one case (the mask is chosen by the test): x, both weights, both biases, the previous state row"""
    G = (4 if cell == LSTM else 3) * H
    SW = (2 if cell == LSTM else 1) * H
    g = torch.Generator().manual_seed(7000 + 1000 * N + H + (1 if cell == LSTM else 0))
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(x=0.7 * r(N, H), wih=r(G, H) / H ** 0.5, whh=r(G, H) / H ** 0.5, bih=0.1 * r(G), bhh=0.1 * r(G), state=0.5 * r(N, SW))


def kernel_reference(cell, d, mask, dtype=torch.float64):
    """the layer's new state [N, SW] in `dtype`"""
    t = {k: v.to(dtype) for k, v in d.items()}
    return layer_step(cell, t["x"], t["state"], mask, t["wih"], t["whh"], t["bih"], t["bhh"])


def kernel_fp32_distance():
    """worst rel-L2 of the fp32 closed form from float64 over every case and mask: {(cell, "h" | "c"): (figure, case)}"""
    worst = {}
    for cell in (GRU, LSTM):
        for (N, H) in KERNEL_CASES:
            d = kernel_inputs(cell, N, H)
            for kind in KERNEL_MASKS:
                m = kernel_mask(N, kind)
                r64, r32 = kernel_reference(cell, d, m), kernel_reference(cell, d, m, torch.float32)
                for name, sl in (("h", slice(0, H)), ("c", slice(H, 2 * H))):
                    if name == "c" and cell == GRU:
                        continue
                    v = rel_l2(r32[:, sl], r64[:, sl])
                    if v > worst.get((cell, name), (-1.0, None))[0]:
                        worst[(cell, name)] = (v, (N, H, kind))
    return worst


_BOUNDS = {}


def kernel_bounds():
    """The GPU bound of every kernel output: 10 x the worst fp32-vs-float64 rel-L2 of its closed form over the case table"""
    if not _BOUNDS:
        _BOUNDS.update({k: 10.0 * v for k, (v, _) in kernel_fp32_distance().items()})
    return _BOUNDS


# ---- the policy tests' cases (tests/test_gpu_rnn_layers.py) -----------------------------------------------------------------------
# (T, N, S, C, H, E, null, A, goal_in, L, cell)
POLICY_CASES = [
    (3, 5, 7, 64, 64, 0, 0, 6, 0, 2, GRU),        # basic learn pass, two GRU layers
    (4, 33, 7, 64, 32, 0, 0, 6, 0, 3, LSTM),      # three LSTM layers, a second actor block
    (2, 2, 7, 64, 256, 0, 0, 6, 0, 2, GRU),       # the fused reverse route
    (2, 2, 7, 64, 256, 0, 0, 6, 0, 2, LSTM),
    (1, 3, 7, 64, 64, 0, 0, 6, 0, 2, GRU),        # T = 1
    (1, 3, 7, 64, 64, 0, 0, 6, 0, 2, LSTM),
    (3, 4, 7, 64, 32, 0, 0, 4, 2, 2, LSTM),       # coordinate goals
    (3, 4, 7, 64, 32, 6, 1, 6, 0, 2, GRU),        # previous actions (null token)
    (2, 3, 7, 64, 32, 0, 0, 84, 0, 2, LSTM),      # 84 actions: the wide heads
    (3, 5, 7, 64, 40, 0, 0, 6, 0, 2, GRU),        # H % 32 != 0: GEMM + gate kernels both ways, the act step on the general route too
]
REDRAW_MARGIN = 1e-4       # re-draw the features while a compressor pre-activation lies this close to its ReLU kink


def policy_cfg(T, N, S, C, H, E, null, A, goal_in, L, cell):
    return dict(in_channels=C, spatial=S, hidden=H, goal_in=goal_in, num_actions=A, prev_action_dims=E, prev_action_null=null)


def _near_kink(sd, feat, goal, goal_in):
    """smallest |pre-activation| of the compressor's two ReLUs (float64): a kink nearer than fp32 resolves flips a unit"""
    T, N = feat.shape[:2]
    s = {k: v.double() for k, v in sd.items()}
    x = feat.double().reshape(T * N, *feat.shape[2:])
    a1 = F.conv2d(x, s["goal_visual_encoder.resnet_compressor.0.weight"], s["goal_visual_encoder.resnet_compressor.0.bias"])
    a2 = F.conv2d(F.relu(a1), s["goal_visual_encoder.resnet_compressor.2.weight"], s["goal_visual_encoder.resnet_compressor.2.bias"])
    return min(float(a1.abs().min()), float(a2.abs().min()))


def policy_inputs(T, N, S, C, H, E, null, A, goal_in, L, cell):
    """-> (cfg, sd, batch): seeded fp32 parameters (every recurrent bias given values, so that a bias bug shows) and one rollout
    batch whose h0 is the state rows [1, N, L * SW]; masks have zeros at t = 0 and in the middle."""
    from embodied_clip_amd import synthetic as syn
    cfg = policy_cfg(T, N, S, C, H, E, null, A, goal_in, L, cell)
    sd = syn.policy_state_dict(7, **cfg, rnn_type=cell, rnn_layers=L)
    G = (4 if cell == LSTM else 3) * H
    SW = (2 if cell == LSTM else 1) * H
    g = torch.Generator().manual_seed(8 + L)
    for l in range(L):
        sd[names(l)[2]] = 0.05 * torch.randn(G, generator=g)
        sd[names(l)[3]] = 0.05 * torch.randn(G, generator=g)
    goal = syn.synthetic_goal_vectors(9, (T, N), goal_in, rho_max=30.0) if goal_in else syn.synthetic_goals(9, (T, N))
    for _ in range(16):
        feat = torch.randn(T, N, C, S, S, generator=g).abs()       # post-ReLU features are non-negative
        if _near_kink(sd, feat, goal, goal_in) > REDRAW_MARGIN:
            break
    h0 = torch.randn(1, N, L * SW, generator=g) * 0.5
    masks = torch.ones(T, N, 1)
    masks[0, ::2] = 0.0                                             # episodes that start at t = 0 ...
    if T > 2:
        masks[T // 2, 1::3] = 0.0                                   # ... and in the middle
    actions = torch.randint(0, A, (T, N), generator=g)
    prev = torch.randint(0, A, (T, N), generator=g)
    noise = [torch.randn(T, N, 1, generator=g) for _ in range(4)]
    dstate = torch.randn(N, L * SW, generator=g) / (L * SW) ** 0.5  # dL/d(final state): a non-zero slice for every layer
    batch = dict(feat=feat, goal=goal, h0=h0, masks=masks, actions=actions, prev_actions=prev, noise=noise, dstate=dstate)
    return cfg, sd, batch


def policy_reference(cell, sd, batch, null, dtype=torch.float32):
    """The reference's forward and one optimiser step in `dtype` -> dict(logits, values, h, info, ref_grads, sd_ref, batch)"""
    from oracle import policy as opol
    from oracle import ppo as oppo
    c = lambda t: t.to(dtype) if t.is_floating_point() else t
    sd = {k: c(v) for k, v in sd.items()}
    b = {k: c(v) for k, v in batch.items() if k != "noise"}
    n = [c(v) for v in batch["noise"]]
    with torch.no_grad():
        lg, vv, hf = actor_critic_forward(cell, b["feat"], b["goal"], b["prev_actions"], b["h0"], b["masks"], sd, null)
    b["old_log_probs"] = opol.categorical_log_prob(lg, b["actions"]).unsqueeze(-1) + 0.2 * n[0]
    b["old_values"] = vv + 0.2 * n[1]
    b["returns"], b["norm_adv"] = n[2], n[3]
    sd_ref = {k: v.clone() for k, v in sd.items()}
    with as_oracle_policy(cell, b["prev_actions"], null):
        info, ref_grads = oppo.ppo_update_step(sd_ref, b, {}, lr=3e-4, max_grad_norm=0.5)
    return dict(logits=lg, values=vv, h=hf, info=info, ref_grads=ref_grads, sd_ref=sd_ref, batch=b)


def state_grad_reference(cell, sd, batch, null, dtype=torch.float64):
    """Gradients of L = sum(dstate * final state) alone: what a backward with dhv = 0 and dh_final = dstate must produce"""
    c = lambda t: t.to(dtype) if t.is_floating_point() else t
    leaves = {k: c(v).clone().requires_grad_(True) for k, v in sd.items()}
    b = {k: c(v) for k, v in batch.items() if k != "noise"}
    _, _, state = actor_critic_forward(cell, b["feat"], b["goal"], b["prev_actions"], b["h0"], b["masks"], leaves, null)
    loss = (state[0] * b["dstate"]).sum()
    ns = list(leaves)
    grads = torch.autograd.grad(loss, [leaves[k] for k in ns], allow_unused=True)
    return {k: (torch.zeros_like(leaves[k]) if g is None else g).detach() for k, g in zip(ns, grads)}


def policy_fp32_distance(case):
    """rel-L2 of the fp32 reference from its float64 self at one policy case: (forward, worst gradient tensor).  The float64 run
    replays the fp32 run's PPO batch, so both differentiate the same loss."""
    from oracle import ppo as oppo
    cell, null = case[10], case[6]
    cfg, sd, batch = policy_inputs(*case)
    r32 = policy_reference(cell, sd, batch, null)
    b64 = {k: (v.double() if v.is_floating_point() else v) for k, v in r32["batch"].items()}
    sd64 = {k: v.double() for k, v in sd.items()}
    with torch.no_grad():
        lg, vv, hf = actor_critic_forward(cell, b64["feat"], b64["goal"], b64["prev_actions"], b64["h0"], b64["masks"], sd64, null)
    with as_oracle_policy(cell, b64["prev_actions"], null):
        _, g64 = oppo.ppo_update_step({k: v.clone() for k, v in sd64.items()}, b64, {}, lr=3e-4, max_grad_norm=0.5)
    fwd = max(rel_l2(r32["logits"], lg), rel_l2(r32["values"], vv), rel_l2(r32["h"], hf))
    grad = max(rel_l2(r32["ref_grads"][k], g64[k]) for k in g64)
    return fwd, grad


if __name__ == "__main__":
    for k, (v, case) in kernel_fp32_distance().items():
        print(f"{k[0]:5s}{k[1]:2s} worst fp32-vs-fp64 rel-L2 {v:.3e} at (N, H, mask) = {case}")
    for case in POLICY_CASES:
        print("policy case", case, "fp32-vs-fp64 rel-L2 (forward, worst gradient tensor): %.3e %.3e" % policy_fp32_distance(case))

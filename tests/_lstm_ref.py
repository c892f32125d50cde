"""Float64 reference, case tables and seeded inputs of the LSTM recurrent core (test infrastructure only; used by
tests/test_lstm_ref.py on the CPU and the tests/test_gpu_lstm*.py modules).

Plain torch, dtype-generic; nothing here imports the product except its seeded parameter generator.  The cell is restated from
torch.nn.LSTM and [U] allenact RNNStateEncoder(rnn_type="LSTM"), neither of which is under the reference tree: parity is
unpinned.  The goal encoders and the previous-action embedding are imported (oracle.policy.goal_encoder, tests/_pointnav_ref.py,
tests/_prev_action_ref.py), not copied.

State convention (include/ec_amd.h): an actor's recurrent state is ONE row [h | c] of width 2H; upstream's memory tensor is
[2, N, H] (h then c) and is converted at the plugin boundary only (memory_to_state / state_to_memory below).

Run as a program (CPU only, about a minute), this file prints what the bounds of the GPU tests are held against: the worst rel-L2
of the SAME closed forms evaluated in fp32 torch against float64 over the kernel case table, and the fp32 model's distance from
its float64 self at every policy case,

    python tests/_lstm_ref.py
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

import _prev_action_ref as pa_ref  # noqa: E402

rel_l2 = pa_ref.rel_l2
EMB_KEY = pa_ref.EMB_KEY
WIH, WHH, BIH, BHH = ("state_encoder.rnn.weight_ih_l0", "state_encoder.rnn.weight_hh_l0", "state_encoder.rnn.bias_ih_l0",
                      "state_encoder.rnn.bias_hh_l0")
FWD_TOL, GRAD_TOL = 2e-5, 2e-4           # the policy path's own: forward rel-L2, per-tensor gradient rel-L2


# ---- state layouts ------------------------------------------------------------------------------------------------------------
def memory_to_state(mem):
    """[2, N, H] (h, c) -> [N, 2H] rows [h | c]"""
    L, N, H = mem.shape
    return mem.permute(1, 0, 2).reshape(N, L * H).contiguous()


def state_to_memory(state, L=2):
    """[N, 2H] rows [h | c] -> [2, N, H]"""
    return state.view(state.shape[0], L, -1).permute(1, 0, 2).contiguous()


# ---- the masked cell and its closed-form reverse step ---------------------------------------------------------------------------
def cell(a_in, h_prev, c_prev, m, whh, bhh):
    """One step.  a_in [N, 4H] = W_ih x + b_ih; m [N] in {0, 1} resets BOTH states.  -> (h, c, gates [N, 4H] = i|f|g|o, cp)"""
    mm = m.reshape(-1, 1).to(a_in.dtype)
    hp, cp = mm * h_prev, mm * c_prev
    a = a_in + hp @ whh.t() + bhh
    i, f, g, o = a.chunk(4, dim=-1)
    i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
    c = f * cp + i * g
    h = o * torch.tanh(c)
    return h, c, torch.cat([i, f, g, o], dim=-1), cp


def reverse_gates(dh, dc_in, gates, c, cp, m):
    """Closed form of one reverse step's gate math.  dh = dL/dh_t (everything), dc_in = dL/dc_t from step t+1.
    -> (da [N, 4H], dc_out = m * dc * f: dL/dc_{t-1} through the cell state)"""
    i, f, g, o = gates.chunk(4, dim=-1)
    tc = torch.tanh(c)
    d_o = dh * tc * o * (1 - o)
    dc = dc_in + dh * o * (1 - tc * tc)
    di = dc * g * i * (1 - i)
    df = dc * cp * f * (1 - f)
    dg = dc * i * (1 - g * g)
    return torch.cat([di, df, dg, d_o], dim=-1), m.reshape(-1, 1).to(dh.dtype) * dc * f


def reverse_step(dhs, carry_h, carry_c, gates, c, cp, m, whh):
    """The gate-plus-GEMM route: dh = dhs + carry_h.  -> (da, carry_h' = m * (da W_hh), carry_c')"""
    da, cc = reverse_gates(dhs + carry_h, carry_c, gates, c, cp, m)
    return da, m.reshape(-1, 1).to(da.dtype) * (da @ whh), cc


def reverse_step_fused(dhs, carry_c, gates, c, cp, m, whh, da_next, m_next):
    """The fused route: dh = dhs + m_{t+1} * (da_{t+1} W_hh).  -> (da, carry_c')"""
    dh = dhs + m_next.reshape(-1, 1).to(dhs.dtype) * (da_next @ whh)
    return reverse_gates(dh, carry_c, gates, c, cp, m)


def sequence(x, state0, masks, sd):
    """RNNStateEncoder(rnn_type="LSTM") over x [T, N, I] from state rows [N, 2H]; masks [T, N, 1].  -> (out [T, N, H], state [N, 2H])"""
    H = sd[WHH].shape[1]
    h, c = state0[:, :H], state0[:, H:]
    outs = []
    for t in range(x.shape[0]):
        a_in = F.linear(x[t], sd[WIH], sd[BIH])
        h, c, _, _ = cell(a_in, h, c, masks[t].reshape(-1), sd[WHH], sd[BHH])
        outs.append(h)
    return torch.stack(outs, 0), torch.cat([h, c], dim=-1)


# ---- the model ----------------------------------------------------------------------------------------------------------------
def actor_critic_forward(feat, goal, prev_actions, state0, masks, sd, null):
    """goal encoder -> [+ previous-action embedding] -> LSTM -> heads: (logits, values, state [1, N, 2H]).  state0: [1, N, 2H]."""
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
    out, state = sequence(x, state0[0], masks, sd)
    logits = F.linear(out, sd["actor.linear.weight"], sd["actor.linear.bias"])
    values = F.linear(out, sd["critic.fc.weight"], sd["critic.fc.bias"])
    return logits, values, state.unsqueeze(0)


@contextlib.contextmanager
def as_oracle_policy(prev_actions, null):
    """Puts the forward above in oracle.policy.actor_critic_forward's place for the duration of a `with` block, so that
    oracle.ppo.ppo_update_step serves unchanged (batch["h0"] is then the state rows [1, N, 2H])."""
    from oracle import policy as opol

    def forward(feat, goal, h0, masks, sd):
        return actor_critic_forward(feat, goal, prev_actions, h0, masks, sd, null)
    with mock.patch.object(opol, "actor_critic_forward", forward):
        yield


# ---- the kernel tests' cases ----------------------------------------------------------------------------------------------------
# (N, H): one lane row, whole-K staging, grid.x = 4 | a second actor block holding one row | one LDS-DMA chunk | two chunks
KERNEL_CASES = [(1, 32), (33, 64), (5, 256), (37, 512)]
KERNEL_OUTPUTS = ("h", "c", "gates", "da", "carry_h", "carry_c", "da_fused", "carry_c_fused")


def kernel_masks(N):
    """masks holding both values: one tensor with zeros and ones, or at one actor the two single-value masks"""
    if N == 1:
        return [torch.zeros(1), torch.ones(1)]
    return [(torch.arange(N) % 3 != 1).float()]


def kernel_inputs(N, H, mask):
    """fp32 inputs of one case.  The backward's gates / c / c_prev are the float64 forward's results rounded to fp32: inputs
    of the reverse step, the same for the kernel and for the closed form."""
    g = torch.Generator().manual_seed(1000 * N + H + int(mask.sum().item()))
    r = lambda *s: torch.randn(*s, generator=g)
    d = dict(a_in=r(N, 4 * H), whh=r(4 * H, H) / H ** 0.5, bhh=0.1 * r(4 * H), state=0.5 * r(N, 2 * H), mask=mask.clone(),
             dhs=r(N, H), carry_h=0.5 * r(N, H), carry_c=0.5 * r(N, H), da_next=0.2 * r(N, 4 * H),
             mask_next=(torch.arange(N) % 2 == 0).float() if N > 1 else torch.ones(1))
    h, c, gates, cp = cell(d["a_in"].double(), d["state"][:, :H].double(), d["state"][:, H:].double(), mask, d["whh"].double(),
                           d["bhh"].double())
    d.update(gates=gates.float(), c=c.float(), cp=cp.float())
    return d


def kernel_reference(d, dtype=torch.float64):
    """-> dict over KERNEL_OUTPUTS of the closed forms in `dtype`"""
    t = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in d.items()}
    H = t["whh"].shape[1]
    h, c, gates, _ = cell(t["a_in"], t["state"][:, :H], t["state"][:, H:], t["mask"], t["whh"], t["bhh"])
    da, ch, cc = reverse_step(t["dhs"], t["carry_h"], t["carry_c"], t["gates"], t["c"], t["cp"], t["mask"], t["whh"])
    daf, ccf = reverse_step_fused(t["dhs"], t["carry_c"], t["gates"], t["c"], t["cp"], t["mask"], t["whh"], t["da_next"], t["mask_next"])
    return dict(h=h, c=c, gates=gates, da=da, carry_h=ch, carry_c=cc, da_fused=daf, carry_c_fused=ccf)


def fp32_distance():
    """worst rel-L2 of the fp32 closed forms from float64 over every case and mask: {name: (figure, case)}"""
    worst = {}
    for (N, H) in KERNEL_CASES:
        for mask in kernel_masks(N):
            d = kernel_inputs(N, H, mask)
            r64, r32 = kernel_reference(d), kernel_reference(d, torch.float32)
            for k in KERNEL_OUTPUTS:
                if not r64[k].any():                        # (one actor, mask 0: carries that are exactly zero in every precision)
                    assert not r32[k].any(), k
                    continue
                v = rel_l2(r32[k], r64[k])
                if v > worst.get(k, (-1.0, None))[0]:
                    worst[k] = (v, (N, H, mask.tolist()[:3]))
    return worst


_BOUNDS = {}


def kernel_bounds():
    """The GPU bound of every kernel output: 10 x the worst fp32-vs-float64 rel-L2 of its closed form over the case table
    (measured here, once per process; the figures of one run are quoted in tests/test_gpu_lstm_kernels.py's docstring)"""
    if not _BOUNDS:
        _BOUNDS.update({k: 10.0 * v for k, (v, _) in fp32_distance().items()})
    return _BOUNDS


# ---- the policy tests' cases (tests/test_gpu_lstm.py) ---------------------------------------------------------------------------
# (T, N, S, C, H, E, null, A, goal_in, bf16 features)
POLICY_CASES = [
    (1, 1, 7, 64, 32, 0, 0, 6, 0, False),        # the act step at one actor
    (3, 5, 7, 64, 64, 0, 0, 6, 0, False),        # basic learn pass
    (6, 4, 3, 64, 32, 0, 0, 6, 0, False),        # S*S = 9, flat = 288: the routes that keep weight_ih's column order
    (4, 33, 7, 64, 32, 32, 1, 4, 3, True),       # coordinate goals with previous actions
    (2, 16, 7, 64, 512, 0, 0, 6, 0, True),       # the fused backward, two K chunks
    (3, 5, 7, 64, 256, 6, 0, 84, 0, False),      # the wide learn plan, fused backward
]


def policy_cfg(T, N, S, C, H, E, null, A, goal_in, bf16):
    return dict(in_channels=C, spatial=S, hidden=H, goal_in=goal_in, num_actions=A, prev_action_dims=E, prev_action_null=null)


def policy_inputs(T, N, S, C, H, E, null, A, goal_in, bf16):
    """-> (cfg, sd, batch): seeded fp32 parameters (LSTM shapes; the recurrent biases, zero in the generator, are given values
    here so that a bias bug shows) and one rollout batch whose h0 is the state rows [1, N, 2H]"""
    from embodied_clip_amd import synthetic as syn
    cfg = policy_cfg(T, N, S, C, H, E, null, A, goal_in, bf16)
    sd = syn.policy_state_dict(7, **cfg, rnn_type="LSTM")
    g = torch.Generator().manual_seed(8)
    sd[BIH] = 0.05 * torch.randn(4 * H, generator=g)
    sd[BHH] = 0.05 * torch.randn(4 * H, generator=g)
    feat = torch.randn(T, N, C, S, S, generator=g).abs()       # post-ReLU features are non-negative
    if bf16:
        feat = feat.to(torch.bfloat16).float()
    goal = syn.synthetic_goal_vectors(9, (T, N), goal_in, rho_max=30.0) if goal_in else syn.synthetic_goals(9, (T, N))
    h0 = torch.randn(1, N, 2 * H, generator=g) * 0.5
    masks = syn.synthetic_masks(10, T, N, p_reset=0.2)
    actions = torch.randint(0, A, (T, N), generator=g)
    prev = torch.randint(0, A, (T, N), generator=g)
    noise = [torch.randn(T, N, 1, generator=g) for _ in range(4)]
    dstate = torch.randn(N, 2 * H, generator=g) / (2 * H) ** 0.5      # dL/d(final state), for the dh_final test
    batch = dict(feat=feat, goal=goal, h0=h0, masks=masks, actions=actions, prev_actions=prev, noise=noise, dstate=dstate)
    return cfg, sd, batch


def policy_reference(sd, batch, null, dtype=torch.float32):
    """The reference's forward and one optimiser step in `dtype` -> dict(logits, values, h, info, ref_grads, sd_ref, batch)"""
    from oracle import policy as opol
    from oracle import ppo as oppo
    c = lambda t: t.to(dtype) if t.is_floating_point() else t
    sd = {k: c(v) for k, v in sd.items()}
    b = {k: c(v) for k, v in batch.items() if k != "noise"}
    n = [c(v) for v in batch["noise"]]
    with torch.no_grad():
        lg, vv, hf = actor_critic_forward(b["feat"], b["goal"], b["prev_actions"], b["h0"], b["masks"], sd, null)
    b["old_log_probs"] = opol.categorical_log_prob(lg, b["actions"]).unsqueeze(-1) + 0.2 * n[0]
    b["old_values"] = vv + 0.2 * n[1]
    b["returns"], b["norm_adv"] = n[2], n[3]
    sd_ref = {k: v.clone() for k, v in sd.items()}
    with as_oracle_policy(b["prev_actions"], null):
        info, ref_grads = oppo.ppo_update_step(sd_ref, b, {}, lr=3e-4, max_grad_norm=0.5)
    return dict(logits=lg, values=vv, h=hf, info=info, ref_grads=ref_grads, sd_ref=sd_ref, batch=b)


def state_grad_reference(sd, batch, null, dtype=torch.float64):
    """Gradients of L = sum(dstate * final state) alone (no head term): what a backward with dhv = 0 and dh_final = dstate
    must produce; the c half of dstate reaches the parameters only through the cell state."""
    c = lambda t: t.to(dtype) if t.is_floating_point() else t
    leaves = {k: c(v).clone().requires_grad_(True) for k, v in sd.items()}
    b = {k: c(v) for k, v in batch.items() if k != "noise"}
    _, _, state = actor_critic_forward(b["feat"], b["goal"], b["prev_actions"], b["h0"], b["masks"], leaves, null)
    loss = (state[0] * b["dstate"]).sum()
    names = list(leaves)
    grads = torch.autograd.grad(loss, [leaves[k] for k in names], allow_unused=True)
    return {k: (torch.zeros_like(leaves[k]) if g is None else g).detach() for k, g in zip(names, grads)}


def policy_fp32_distance(case):
    """rel-L2 of the fp32 reference from its float64 self at one policy case: (worst of logits / values / state, worst gradient tensor).
    The float64 run replays the fp32 run's PPO batch (old log-probs and values), so both differentiate the same loss."""
    from oracle import ppo as oppo
    cfg, sd, batch = policy_inputs(*case)
    r32 = policy_reference(sd, batch, case[6])
    b64 = {k: (v.double() if v.is_floating_point() else v) for k, v in r32["batch"].items()}
    sd64 = {k: v.double() for k, v in sd.items()}
    with torch.no_grad():
        lg, vv, hf = actor_critic_forward(b64["feat"], b64["goal"], b64["prev_actions"], b64["h0"], b64["masks"], sd64, case[6])
    with as_oracle_policy(b64["prev_actions"], case[6]):
        _, g64 = oppo.ppo_update_step({k: v.clone() for k, v in sd64.items()}, b64, {}, lr=3e-4, max_grad_norm=0.5)
    fwd = max(rel_l2(r32["logits"], lg), rel_l2(r32["values"], vv), rel_l2(r32["h"], hf))
    grad = max(rel_l2(r32["ref_grads"][k], g64[k]) for k in g64)
    return fwd, grad


if __name__ == "__main__":
    for k, (v, case) in fp32_distance().items():
        print(f"{k:14s} worst fp32-vs-fp64 rel-L2 {v:.3e} at (N, H, mask[:3]) = {case}")
    for case in POLICY_CASES:
        print("policy case", case, "fp32-vs-fp64 rel-L2 (forward, worst gradient tensor): %.3e %.3e" % policy_fp32_distance(case))

"""Float64 reference, case tables and seeded inputs of the two-view rearrangement net (test infrastructure only; used by
tests/test_two_view_ref.py on the CPU and the tests/test_gpu_two_view*.py modules).

The net restates [U] ai2thor-rearrangement's ResNetRearrangeActorCriticRNN (published sources, not under the reference tree:
parity unpinned).  The reference is COMPOSED of torch's own modules in upstream's NCHW form -- nn.Conv2d(.., 1), torch.softmax,
nn.Embedding, nn.LSTM / nn.GRU, nn.Linear -- under the module names of the flat parameter table (embodied_clip_amd/policy.py),
so a handle's state dict loads into it unchanged:

    concat = cat([u, w, u * w], channel)                    u, w: the two frozen CLIP maps [B, C, s, s]
    enc    = visual_encoder(concat)                         Sequential(Conv2d(3C, H, 1), ReLU)
    att    = visual_attention(concat)                       Sequential(Conv2d(3C, A1, 1), ReLU, Conv2d(A1, 1, 1))
    probs  = softmax(att.view(B, -1), -1).view(B, 1, s, s)
    v      = (enc * probs).mean(-1).mean(-1)                a MEAN over the pixels, not a sum
    x      = [ v | prev_action_embedder[(prev + 1) * mask] ]
    h      = RNN(x, m * h_prev); logits, value = actor.linear(h), critic.fc(h)

The features are non-negative, as a post-ReLU trunk output is, and rounded to bf16: the reference and the kernels read the same
values.

Run as a program (CPU only), this file prints what the bounds of the GPU tests are held against:

    python tests/_two_view_ref.py
"""
import os
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import _rnn_stack_ref as _rs  # noqa: E402

GRU, LSTM = "GRU", "LSTM"
FWD_TOL, GRAD_TOL = _rs.FWD_TOL, _rs.GRAD_TOL          # the policy path's own bounds: 2e-5 forward, 2e-4 per gradient tensor
B2 = "visual_attention.2.bias"                          # its gradient is analytically zero (softmax is shift-invariant)
W2 = "visual_attention.2.weight"
FRONT = ("visual_encoder.0.weight", "visual_encoder.0.bias", "visual_attention.0.weight", "visual_attention.0.bias", W2, B2)


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a.reshape(-1) - b.reshape(-1)).norm() / b.norm().clamp_min(1e-30)).item()


# ---- the front alone: (B, S2, C, H, A1) ------------------------------------------------------------------------------------------
#   B: 1, 5, 33 -- frames straddling 32-row tiles and a last partial group; 770 -- the five-tile kernel (three frames of 49
#      pixels per workgroup, taken from 256 workgroups on) with a last group of two frames
#   S2: 49, 9 (seven frames per 64 rows), 64 (a frame fills the group)
#   C: 64 = one staged chunk per plane, 192 = three (no power of two)
#   H: 32, 96 with A1 = 32; A1 = 64 once; one full-width row (C = 2048, H = 512: three column chunks per frame group)
KERNEL_CASES = [
    (1, 49, 64, 32, 32),
    (5, 49, 64, 96, 32),
    (33, 49, 192, 96, 32),
    (5, 9, 64, 32, 32),
    (33, 9, 192, 32, 32),
    (5, 64, 192, 96, 32),
    (33, 64, 64, 32, 32),
    (5, 49, 64, 32, 64),
    (770, 49, 64, 32, 32),
    (3, 49, 2048, 512, 32),
]
# what the issue's CPU check covered (the fp32 evaluation of the reference against float64)
FP32_CASES = [(5, 49, 64, 64, 32), (33, 49, 128, 96, 32), (3, 49, 2048, 512, 32), (4, 9, 64, 32, 32)]
EDGES = ("zero_u", "logits80", "dead_column")


class TwoViewFront(nn.Module):
    """visual_encoder / visual_attention in upstream's NCHW form"""

    def __init__(self, in_channels, hidden, attn_hidden=32):
        super().__init__()
        self.visual_encoder = nn.Sequential(nn.Conv2d(3 * in_channels, hidden, 1), nn.ReLU(inplace=True))
        self.visual_attention = nn.Sequential(nn.Conv2d(3 * in_channels, attn_hidden, 1), nn.ReLU(inplace=True),
                                              nn.Conv2d(attn_hidden, 1, 1))

    def forward(self, u, w):
        """u, w [B, C, s, s] -> v [B, H]"""
        concat = torch.cat([u, w, u * w], dim=1)
        enc = self.visual_encoder(concat)
        att = self.visual_attention(concat)
        B = u.shape[0]
        probs = torch.softmax(att.view(B, -1), dim=-1).view(B, 1, *att.shape[-2:])
        return (enc * probs).mean(-1).mean(-1)


def to_nchw(rows):
    """pixel-major rows [B, S2, C] -> [B, C, s, s]"""
    B, S2, C = rows.shape
    s = int(round(S2 ** 0.5))
    assert s * s == S2
    return rows.view(B, s, s, C).permute(0, 3, 1, 2).contiguous()


def closed_form(u, w, sd, dv=None):
    """The pixel-major closed form of the issue (u, w [B, S2, C]; the six front tensors in `sd`) -> v, and with dv the six gradients
    of sum(v * dv) by the closed-form backward."""
    B, S2, C = u.shape
    We, be = sd[FRONT[0]].reshape(-1, 3 * C), sd[FRONT[1]]
    Wa, ba = sd[FRONT[2]].reshape(-1, 3 * C), sd[FRONT[3]]
    w2, b2 = sd[W2].reshape(-1), sd[B2]
    c = torch.cat([u, w, u * w], -1)                          # [B, S2, 3C]
    e = torch.relu(c @ We.t() + be)
    m = torch.relu(c @ Wa.t() + ba)
    l = m @ w2 + b2
    a = torch.softmax(l, -1)                                  # over the S2 pixels of the frame
    v = (a.unsqueeze(-1) * e).sum(1) / S2
    if dv is None:
        return v
    s = (e * dv.unsqueeze(1)).sum(-1) / S2
    dl = a * (s - (a * s).sum(-1, keepdim=True))
    de = (a / S2).unsqueeze(-1) * dv.unsqueeze(1) * (e > 0)
    dm = dl.unsqueeze(-1) * w2 * (m > 0)
    c2 = c.reshape(B * S2, 3 * C)
    grads = {FRONT[0]: (de.reshape(B * S2, -1).t() @ c2).reshape(sd[FRONT[0]].shape), FRONT[1]: de.sum((0, 1)),
             FRONT[2]: (dm.reshape(B * S2, -1).t() @ c2).reshape(sd[FRONT[2]].shape), FRONT[3]: dm.sum((0, 1)),
             W2: (dl.unsqueeze(-1) * m).sum((0, 1)).reshape(sd[W2].shape), B2: dl.sum().reshape(1)}
    return v, grads


def features(gen, B, S2, C):
    """non-negative (a post-ReLU trunk output), about half the entries zero, rounded to bf16"""
    return torch.relu(torch.randn(B, S2, C, generator=gen)).to(torch.bfloat16).float()


def kernel_inputs(B, S2, C, H, A1, edge=None):
    """-> (sd of the six front tensors fp32, u, w [B, S2, C] bf16-valued fp32, dv [B, H])"""
    from embodied_clip_amd import synthetic as syn
    full = syn.policy_state_dict(7, two_view=dict(in_channels=C, hidden=H, num_actions=6, attn_hidden=A1, rnn_type=GRU))
    sd = {k: full[k].clone() for k in FRONT}
    g = torch.Generator().manual_seed(1000 + B + 3 * S2 + 5 * C + 7 * H + A1)
    sd[FRONT[1]] = 0.1 * torch.randn(H, generator=g)
    sd[FRONT[3]] = 0.1 * torch.randn(A1, generator=g)
    sd[W2] = torch.randn(1, A1, 1, 1, generator=g)
    sd[B2] = torch.tensor([0.3])
    u, w = features(g, B, S2, C), features(g, B, S2, C)
    dv = torch.randn(B, H, generator=g)
    if edge == "zero_u":
        u[0] = 0.0                                            # frame 0: c = [0 | w | 0]
    elif edge == "logits80":
        # scale w_2 so that the largest |l - b_2| is 80 (both signs occur: w_2 has both): finite and within the bounds only with the
        # frame's maximum subtracted inside the softmax, and nearly one-hot probabilities
        c = torch.cat([u, w, u * w], -1).double()
        m = torch.relu(c @ sd[FRONT[2]].double().reshape(A1, -1).t() + sd[FRONT[3]].double())
        raw = m @ sd[W2].double().reshape(-1)
        sd[W2] = (sd[W2].double() * (80.0 / raw.abs().max())).float()
    elif edge == "dead_column":
        sd[FRONT[1]][1] = -1.0e4                              # encoder column 1 never fires: e = 0, its gradients are zero
    return sd, u, w, dv


def front_reference(sd, u, w, dv, dtype=torch.float64):
    """The NCHW module form in `dtype` -> (v, grads of sum(v * dv) by autograd)"""
    B, S2, C = u.shape
    H, A1 = sd[FRONT[1]].numel(), sd[FRONT[3]].numel()
    net = TwoViewFront(C, H, A1).to(dtype)
    net.load_state_dict({k: t.to(dtype) for k, t in sd.items()}, strict=True)
    v = net(to_nchw(u.to(dtype)), to_nchw(w.to(dtype)))
    names = [k for k, _ in net.named_parameters()]
    gr = torch.autograd.grad((v * dv.to(dtype)).sum(), [p for _, p in net.named_parameters()])
    return v.detach(), dict(zip(names, [t.detach() for t in gr]))


def grad_errors(got, want):
    """per tensor: rel-L2; visual_attention.2.bias -- analytically zero -- as |g| / ||grad visual_attention.2.weight||"""
    out = {}
    for k, gref in want.items():
        if k == B2:
            out[k] = float(got[k].double().abs().max().cpu() / want[W2].double().norm().cpu())
        else:
            out[k] = rel_l2(got[k], gref)
    return out


# ---- the whole net: (T, N, S2, C, H, E, A, L, cell) ------------------------------------------------------------------------------
#   T x N: 1 x 5, 4 x 3, 3 x 33 (a row tail past one 32-row block), episode resets in the masks
#   E: 0, 6 (prev_action.hip's kernels), 96 = H (above 64: the table and its chain on ec_gemm_f32); A: 6 and 84 (wide heads)
POLICY_CASES = [
    (1, 5, 49, 64, 64, 0, 6, 1, GRU),
    (4, 3, 49, 64, 96, 96, 84, 2, LSTM),
    (3, 33, 9, 192, 96, 6, 6, 1, LSTM),
    (3, 33, 49, 64, 32, 6, 84, 2, GRU),
    (4, 3, 9, 64, 96, 96, 6, 1, GRU),
    (1, 5, 49, 64, 64, 6, 84, 1, LSTM),
]
LOSSES = ("ppo", "imitation")


def handle_kwargs(T, N, S2, C, H, E, A, L, cell):
    """the keywords of ``PolicyHandle.two_view`` / ``policy.two_view_param_shapes``"""
    return dict(in_channels=C, hidden=H, num_actions=A, attn_hidden=32, prev_action_dims=E, prev_action_null=1 if E else 0,
                rnn_type=cell, rnn_layers=L, spatial=int(round(S2 ** 0.5)))


class TwoViewNet(TwoViewFront):
    """The reference model.  Parameter names == the flat table's, so ``load_state_dict(sd)`` takes a handle's state dict."""

    def __init__(self, in_channels, hidden, num_actions, attn_hidden, prev_action_dims, prev_action_null, rnn_type, rnn_layers, spatial):
        super().__init__(in_channels, hidden, attn_hidden)
        self.H, self.L, self.cell, self.E, self.null = hidden, rnn_layers, rnn_type, prev_action_dims, prev_action_null
        if prev_action_dims:
            self.prev_action_embedder = nn.Embedding(num_actions + prev_action_null, prev_action_dims)
        self.state_encoder = nn.Module()
        self.state_encoder.rnn = (nn.LSTM if rnn_type == LSTM else nn.GRU)(hidden + prev_action_dims, hidden, num_layers=rnn_layers)
        self.actor = nn.Module()
        self.actor.linear = nn.Linear(hidden, num_actions)
        self.critic = nn.Module()
        self.critic.fc = nn.Linear(hidden, 1)

    def forward(self, u, w, prev, state0, masks):
        """u, w [T, N, S2, C]; prev [T, N] | None; state0 [N, L * SW]; masks [T, N, 1] -> (logits, values [T, N, 1], state)"""
        from _pooled_net_ref import memory_to_state, state_to_memory
        T, N = masks.shape[:2]
        v = TwoViewFront.forward(self, to_nchw(u.reshape(T * N, *u.shape[2:])), to_nchw(w.reshape(T * N, *w.shape[2:])))
        parts = [v]
        if self.E:
            idx = prev_row(prev.reshape(T * N), masks.reshape(T * N), self.null)
            parts.append(self.prev_action_embedder(idx))
        x = torch.cat(parts, 1).view(T, N, -1)
        mem = state_to_memory(state0, self.cell, self.L)
        outs = []
        for t in range(T):
            m = masks[t].reshape(1, N, 1).to(x.dtype)
            if self.cell == LSTM:
                h, c = mem[:self.L] * m, mem[self.L:] * m
                out, (h, c) = self.state_encoder.rnn(x[t:t + 1], (h.contiguous(), c.contiguous()))
                mem = torch.cat([h, c], 0)
            else:
                out, mem = self.state_encoder.rnn(x[t:t + 1], (mem * m).contiguous())
            outs.append(out[0])
        top = torch.stack(outs, 0)
        return self.actor.linear(top), self.critic.fc(top), memory_to_state(mem, self.cell, self.L)


def prev_row(prev, masks, null=1):
    """upstream's row of the previous-action table: ((prev + 1) * mask).long() with the null token, else the action itself"""
    return ((prev.to(masks.dtype) + 1) * masks).long() if null else prev


def policy_inputs(T, N, S2, C, H, E, A, L, cell):
    """-> (kwargs, sd, batch): seeded fp32 parameters (every recurrent bias given values) and one rollout batch; masks have zeros
    at t = 0 and in the middle; the expert acts on about 70 % of the steps"""
    from embodied_clip_amd import synthetic as syn
    case = (T, N, S2, C, H, E, A, L, cell)
    kw = handle_kwargs(*case)
    sd = syn.policy_state_dict(13, two_view=kw)
    G = (4 if cell == LSTM else 3) * H
    SW = (2 if cell == LSTM else 1) * H
    g = torch.Generator().manual_seed(300 + 7 * L + C + H + E + T * N)
    for l in range(L):
        sd[f"state_encoder.rnn.bias_ih_l{l}"] = 0.05 * torch.randn(G, generator=g)
        sd[f"state_encoder.rnn.bias_hh_l{l}"] = 0.05 * torch.randn(G, generator=g)
    sd[FRONT[1]] = 0.1 * torch.randn(H, generator=g)
    sd[FRONT[3]] = 0.1 * torch.randn(32, generator=g)
    sd[W2] = torch.randn(1, 32, 1, 1, generator=g)
    sd[B2] = torch.tensor([0.3])
    u, w = features(g, T * N, S2, C).view(T, N, S2, C), features(g, T * N, S2, C).view(T, N, S2, C)
    state0 = torch.randn(N, L * SW, generator=g) * 0.5
    masks = torch.ones(T, N, 1)
    masks[0, ::2] = 0.0
    if T > 2:
        masks[T // 2, 1::3] = 0.0
    actions = torch.randint(0, A, (T, N), generator=g)
    prev = torch.randint(0, A, (T, N), generator=g) if E else None
    expert = torch.randint(0, A, (T, N), generator=g)
    emask = (torch.rand(T, N, generator=g) < 0.7).float()
    emask[0, 0] = 1.0
    noise = [torch.randn(T, N, 1, generator=g) for _ in range(4)]
    batch = dict(u=u, w=w, prev_actions=prev, state0=state0, masks=masks, actions=actions, expert=expert, emask=emask, noise=noise)
    return kw, sd, batch


def build(case, sd, dtype=torch.float64):
    net = TwoViewNet(**handle_kwargs(*case)).to(dtype)
    net.load_state_dict({k: v.to(dtype) for k, v in sd.items()}, strict=True)
    return net


def policy_reference(case, sd, batch, loss="ppo", dtype=torch.float64, replay=None):
    """Forward, the loss and every parameter's gradient in `dtype` -> dict(logits, values, state, total, grads, batch).
    ppo: the PPO batch derives from the forward and the seeded noise (`replay`: another run's, differentiated instead);
    imitation: the masked mean of the expert's cross entropy (AllenAct's Imitation loss over expert actions)."""
    from oracle import policy as opol
    from oracle import ppo as oppo
    c = lambda t: t.to(dtype) if (t is not None and t.is_floating_point()) else t
    b = {k: c(v) for k, v in batch.items() if k != "noise"}
    net = build(case, sd, dtype)
    with torch.no_grad():
        lg, vv, st = net(b["u"], b["w"], b["prev_actions"], b["state0"], b["masks"])
    if replay is None:
        n = [c(v) for v in batch["noise"]]
        b["old_log_probs"] = opol.categorical_log_prob(lg, b["actions"]).unsqueeze(-1) + 0.2 * n[0]
        b["old_values"] = vv + 0.2 * n[1]
        b["returns"], b["norm_adv"] = n[2], n[3]
    else:
        for k in ("old_log_probs", "old_values", "returns", "norm_adv"):
            b[k] = c(replay[k])
    logits, values, _ = net(b["u"], b["w"], b["prev_actions"], b["state0"], b["masks"])
    if loss == "ppo":
        total, _ = oppo.ppo_loss(logits, values, b["actions"], b["old_log_probs"], b["old_values"], b["returns"], b["norm_adv"])
    else:
        A = logits.shape[-1]
        ce = F.cross_entropy(logits.reshape(-1, A), b["expert"].reshape(-1), reduction="none")
        total = (ce * b["emask"].reshape(-1)).sum() / b["emask"].sum()
    names = [k for k, _ in net.named_parameters()]
    gr = torch.autograd.grad(total, [p for _, p in net.named_parameters()], allow_unused=True)
    grads = {k: (torch.zeros_like(p) if g is None else g).detach() for k, g, (_, p) in zip(names, gr, net.named_parameters())}
    assert set(grads) == set(sd), sorted(set(grads) ^ set(sd))
    return dict(logits=lg, values=vv, state=st, total=float(total.detach()), grads=grads, batch=b)


def front_fp32_distance(case):
    """rel-L2 of the fp32 evaluation of the front from its float64 self: (forward, worst gradient tensor by grad_errors)"""
    sd, u, w, dv = kernel_inputs(*case)
    v32, g32 = front_reference(sd, u, w, dv, torch.float32)
    v64, g64 = front_reference(sd, u, w, dv, torch.float64)
    return rel_l2(v32, v64), max(grad_errors(g32, g64).values())


if __name__ == "__main__":
    for case in FP32_CASES:
        print("front", case, "fp32-vs-fp64 rel-L2 (forward, worst gradient tensor): %.3e %.3e" % front_fp32_distance(case))

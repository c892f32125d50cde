"""Float64 reference, case table and seeded inputs of the pooled-embedding net (test infrastructure only; used by
tests/test_pooled_net_ref.py on the CPU and the tests/test_gpu_pooled_net*.py modules).

The net restates [U] habitat-lab's PointNavResNetNet over one pooled CLIP vector per frame (published sources, not under the
reference tree: parity unpinned).  The reference is COMPOSED of torch's own modules -- nn.Linear, nn.Embedding, nn.GRU, nn.LSTM --
under the module names of the flat parameter table (embodied_clip_amd/policy.py), so a state dict loads into it unchanged:

    v   = ReLU(visual_fc(e))
    x   = [ v | obj_categories_embedding[goal] | sensor embeddings ... | prev_action_embedding[(prev + 1) * mask] ]
    h   = RNN(x, m * h_prev)          the mask multiplies the previous state (h, and c on the LSTM) of every layer
    logits, value = action_distribution.linear(h), critic.fc(h)

State convention (include/ec_amd.h): an actor's state is ONE row of width L * SW, layer-major -- [h^0 | h^1 | ...] (GRU) or
[h^0 | c^0 | h^1 | c^1 | ...] (LSTM).

Run as a program (CPU only), this file prints what the bounds of the GPU tests are held against:

    python tests/_pooled_net_ref.py
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

GRU, LSTM = "GRU", "LSTM"
FWD_TOL, GRAD_TOL = 2e-5, 2e-4          # the policy path's own bounds (tests/_rnn_stack_ref.py FWD_TOL / GRAD_TOL)
EMBED_DIMS = 32


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


# (T, N, D, H, ids, sensors, E, null, A, L, cell): the smallest shapes that still exercise each route
#   D: 64 -> visual_fc on 8 waves, 112 -> 7 waves, 72 -> the general route
#   H: 64 plain staging, 256 one LDS-DMA chunk, 512 two chunks, 40 the fused step off (GRU only)
#   N: 5, and 33 = a row tail past one 32-row block;  T: 1 and 3 (mask zeros at t = 0 and mid-sequence: the null row is read)
POLICY_CASES = [
    (3, 5, 64, 64, 12, (), 0, 0, 6, 1, GRU),              # ids only, no previous action
    (3, 33, 112, 256, 12, (2, 2), 32, 1, 6, 2, LSTM),     # ids with GPS + compass, previous action, two LSTM layers, a row tail
    (3, 5, 64, 512, 0, (3,), 32, 1, 84, 2, LSTM),         # PointNav's 3-float goal only, 84 actions, the published core
    (3, 5, 72, 64, 12, (2, 2), 0, 0, 6, 1, LSTM),         # D = 72: the general route at T = 1 too
    (3, 5, 64, 40, 0, (3,), 32, 1, 6, 2, GRU),            # H = 40: GEMM + gate kernels
    (1, 5, 112, 64, 12, (), 32, 0, 6, 3, GRU),            # T = 1, three layers, previous action without a null row
    (1, 33, 64, 256, 12, (2, 2), 32, 1, 84, 1, GRU),      # T = 1, a row tail, wide heads
    (3, 5, 64, 512, 12, (2, 2), 32, 1, 6, 1, GRU),        # the GRU at the reference width
]
REDRAW_MARGIN = 1e-4       # re-draw the embeddings while a visual_fc pre-activation lies this close to the ReLU kink


def handle_kwargs(T, N, D, H, ids, sensors, E, null, A, L, cell):
    """the keywords of ``PolicyHandle.pooled`` / ``policy.pooled_param_shapes``"""
    return dict(embed_in=D, hidden=H, num_goals=ids, sensors=tuple(sensors), num_actions=A, prev_action_dims=E,
                prev_action_null=null if E else 0, rnn_type=cell, rnn_layers=L)


def sensor_names(sensors):
    from embodied_clip_amd.policy import pooled_sensor_names
    return pooled_sensor_names(sensors)


class PooledNet(nn.Module):
    """The reference model.  Parameter names == the flat table's, so ``load_state_dict(sd)`` takes a handle's state dict."""

    def __init__(self, embed_in, hidden, num_goals, sensors, num_actions, prev_action_dims, prev_action_null, rnn_type, rnn_layers):
        super().__init__()
        self.H, self.L, self.cell, self.A = hidden, rnn_layers, rnn_type, num_actions
        self.sensors, self.null, self.E = tuple(sensors), prev_action_null, prev_action_dims
        self.visual_fc = nn.Sequential(nn.Flatten(), nn.Linear(embed_in, hidden), nn.ReLU(True))
        width = hidden
        if num_goals:
            self.obj_categories_embedding = nn.Embedding(num_goals, EMBED_DIMS)
            width += EMBED_DIMS
        self.sensor_mods = []
        for name, k in zip(sensor_names(sensors), sensors):
            setattr(self, name, nn.Linear(k, EMBED_DIMS))
            self.sensor_mods.append(name)
            width += EMBED_DIMS
        if prev_action_dims:
            self.prev_action_embedding = nn.Embedding(num_actions + prev_action_null, prev_action_dims)
            width += prev_action_dims
        self.state_encoder = nn.Module()
        self.state_encoder.rnn = (nn.LSTM if rnn_type == LSTM else nn.GRU)(width, hidden, num_layers=rnn_layers)
        self.action_distribution = nn.Module()
        self.action_distribution.linear = nn.Linear(hidden, num_actions)
        self.critic = nn.Module()
        self.critic.fc = nn.Linear(hidden, 1)

    def recurrent_input(self, embed, goal, sensors, prev, masks):
        T, N = masks.shape[:2]
        parts = [self.visual_fc(embed.reshape(T * N, -1))]
        if hasattr(self, "obj_categories_embedding"):
            parts.append(self.obj_categories_embedding(goal.reshape(T * N)))
        c0 = 0
        for name, k in zip(self.sensor_mods, self.sensors):
            parts.append(getattr(self, name)(sensors.reshape(T * N, -1)[:, c0:c0 + k]))
            c0 += k
        if self.E:
            p = prev.reshape(T * N)
            idx = ((p.to(masks.dtype) + 1) * masks.reshape(T * N)).long() if self.null else p
            parts.append(self.prev_action_embedding(idx))
        return torch.cat(parts, dim=1).view(T, N, -1)

    def forward(self, embed, goal, sensors, prev, state0, masks):
        """embed [T, N, D]; goal [T, N] | None; sensors [T, N, K] | None; prev [T, N] | None; state0 [N, L * SW]; masks [T, N, 1]
        -> (logits [T, N, A], values [T, N, 1], state [N, L * SW])"""
        T, N = masks.shape[:2]
        x = self.recurrent_input(embed, goal, sensors, prev, masks)
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
        return self.action_distribution.linear(top), self.critic.fc(top), memory_to_state(mem, self.cell, self.L)


def memory_to_state(mem, cell, L):
    """[L, N, H] | [2L, N, H] (all h layers, then all c layers) -> [N, L * SW] layer-major rows"""
    cols = []
    for l in range(L):
        cols.append(mem[l])
        if cell == LSTM:
            cols.append(mem[L + l])
    return torch.cat(cols, dim=-1).contiguous()


def state_to_memory(state, cell, L):
    k = 2 if cell == LSTM else 1
    H = state.shape[1] // (k * L)
    parts = state.split(H, dim=-1)
    hs = [parts[k * l] for l in range(L)]
    cs = [parts[k * l + 1] for l in range(L)] if k == 2 else []
    return torch.stack(hs + cs, 0).contiguous()


def build(case, sd, dtype=torch.float64):
    net = PooledNet(**handle_kwargs(*case)).to(dtype)
    net.load_state_dict({k: v.to(dtype) for k, v in sd.items()}, strict=True)
    return net


# ---- a direct per-step loop, written out (tests/test_pooled_net_ref.py holds the module composition above to it) --------------------
def direct_forward(case, sd, batch, dtype=torch.float64):
    """The same net as explicit arithmetic: F.linear / row gathers / the two cells' gate formulas, one step and one layer at a time."""
    T, N, D, H, ids, sensors, E, null, A, L, cell = case
    c = lambda t: t.to(dtype) if t.is_floating_point() else t
    s = {k: c(v) for k, v in sd.items()}
    b = {k: c(v) for k, v in batch.items() if isinstance(v, torch.Tensor)}
    masks = b["masks"]
    v = torch.relu(F.linear(b["embed"].reshape(T * N, D), s["visual_fc.1.weight"], s["visual_fc.1.bias"]))
    parts = [v]
    if ids:
        parts.append(s["obj_categories_embedding.weight"][b["goal"].reshape(-1)])
    c0 = 0
    for name, k in zip(sensor_names(sensors), sensors):
        parts.append(F.linear(b["sensors"].reshape(T * N, -1)[:, c0:c0 + k], s[name + ".weight"], s[name + ".bias"]))
        c0 += k
    if E:
        p = b["prev_actions"].reshape(-1)
        idx = torch.where(masks.reshape(-1) == 0, torch.zeros_like(p), p + 1) if null else p
        parts.append(s["prev_action_embedding.weight"][idx])
    x = torch.cat(parts, 1).view(T, N, -1)
    SW = (2 if cell == LSTM else 1) * H
    state = b["state0"]
    tops = []
    for t in range(T):
        m = masks[t].reshape(N, 1)
        inp, new = x[t], []
        for l in range(L):
            wih, whh, bih, bhh = (s[f"state_encoder.rnn.{k}_l{l}"] for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
            prev = state[:, l * SW:(l + 1) * SW]
            hp = m * prev[:, :H]
            gi, gh = F.linear(inp, wih, bih), F.linear(hp, whh, bhh)
            if cell == LSTM:
                cp = m * prev[:, H:]
                i, f, g, o = (gi + gh).chunk(4, -1)
                cn = torch.sigmoid(f) * cp + torch.sigmoid(i) * torch.tanh(g)
                hn = torch.sigmoid(o) * torch.tanh(cn)
                new += [hn, cn]
            else:
                ir, iz, inn = gi.chunk(3, -1)
                hr, hz, hnn = gh.chunk(3, -1)
                r, z = torch.sigmoid(ir + hr), torch.sigmoid(iz + hz)
                n = torch.tanh(inn + r * hnn)
                hn = (1 - z) * n + z * hp
                new.append(hn)
            inp = hn
        state = torch.cat(new, -1)
        tops.append(inp)
    top = torch.stack(tops, 0)
    logits = F.linear(top, s["action_distribution.linear.weight"], s["action_distribution.linear.bias"])
    values = F.linear(top, s["critic.fc.weight"], s["critic.fc.bias"])
    return logits, values, state


# ---- seeded inputs -------------------------------------------------------------------------------------------------------------
def policy_inputs(T, N, D, H, ids, sensors, E, null, A, L, cell):
    """-> (kwargs, sd, batch): seeded fp32 parameters (every recurrent bias given values, so that a bias bug shows) and one rollout
    batch.  state0 is the state rows [N, L * SW]; masks have zeros at t = 0 and in the middle; PointNav-like sensor ranges."""
    from embodied_clip_amd import synthetic as syn
    case = (T, N, D, H, ids, sensors, E, null, A, L, cell)
    kw = handle_kwargs(*case)
    sd = syn.policy_state_dict(11, pooled=kw)
    G = (4 if cell == LSTM else 3) * H
    SW = (2 if cell == LSTM else 1) * H
    g = torch.Generator().manual_seed(100 + 7 * L + D + H)
    for l in range(L):
        sd[f"state_encoder.rnn.bias_ih_l{l}"] = 0.05 * torch.randn(G, generator=g)
        sd[f"state_encoder.rnn.bias_hh_l{l}"] = 0.05 * torch.randn(G, generator=g)
    for _ in range(16):
        embed = torch.randn(T, N, D, generator=g)
        pre = F.linear(embed.double().reshape(T * N, D), sd["visual_fc.1.weight"].double(), sd["visual_fc.1.bias"].double())
        if float(pre.abs().min()) > REDRAW_MARGIN:
            break
    K = sum(sensors)
    goal = torch.randint(0, ids, (T, N), generator=g) if ids else None
    sens = None
    if K:
        sens = torch.randn(T, N, K, generator=g)
        if tuple(sensors) == (3,):       # (rho, cos -phi, sin -phi)
            phi = 3.0 * torch.randn(T, N, generator=g)
            sens = torch.stack([10.0 * torch.rand(T, N, generator=g), torch.cos(-phi), torch.sin(-phi)], -1)
    state0 = torch.randn(N, L * SW, generator=g) * 0.5
    masks = torch.ones(T, N, 1)
    masks[0, ::2] = 0.0                                             # episodes that start at t = 0 ...
    if T > 2:
        masks[T // 2, 1::3] = 0.0                                   # ... and in the middle
    actions = torch.randint(0, A, (T, N), generator=g)
    prev = torch.randint(0, A, (T, N), generator=g) if E else None
    noise = [torch.randn(T, N, 1, generator=g) for _ in range(4)]
    batch = dict(embed=embed, goal=goal, sensors=sens, prev_actions=prev, state0=state0, masks=masks, actions=actions, noise=noise)
    return kw, sd, batch


def policy_reference(case, sd, batch, dtype=torch.float64, replay=None):
    """Forward, PPO loss and every parameter's gradient in `dtype` -> dict(logits, values, state, info, grads, batch).
    The PPO batch (old log-probs / values, returns, advantages) derives from the forward and the seeded noise; `replay`: the
    `batch` entry of another run, whose PPO batch is differentiated instead (the fp32 run replayed in float64)."""
    from oracle import policy as opol
    from oracle import ppo as oppo
    c = lambda t: t.to(dtype) if (t is not None and t.is_floating_point()) else t
    b = {k: c(v) for k, v in batch.items() if k != "noise"}
    net = build(case, sd, dtype)
    with torch.no_grad():
        lg, vv, st = net(b["embed"], b["goal"], b["sensors"], b["prev_actions"], b["state0"], b["masks"])
    if replay is None:
        n = [c(v) for v in batch["noise"]]
        b["old_log_probs"] = opol.categorical_log_prob(lg, b["actions"]).unsqueeze(-1) + 0.2 * n[0]
        b["old_values"] = vv + 0.2 * n[1]
        b["returns"], b["norm_adv"] = n[2], n[3]
    else:
        for k in ("old_log_probs", "old_values", "returns", "norm_adv"):
            b[k] = c(replay[k])
    logits, values, _ = net(b["embed"], b["goal"], b["sensors"], b["prev_actions"], b["state0"], b["masks"])
    total, info = oppo.ppo_loss(logits, values, b["actions"], b["old_log_probs"], b["old_values"], b["returns"], b["norm_adv"])
    names = [k for k, _ in net.named_parameters()]
    gr = torch.autograd.grad(total, [p for _, p in net.named_parameters()], allow_unused=True)
    grads = {k: (torch.zeros_like(p) if g is None else g).detach() for k, g, (_, p) in zip(names, gr, net.named_parameters())}
    assert set(grads) == set(sd), (sorted(set(grads) ^ set(sd)))
    return dict(logits=lg, values=vv, state=st, info=info, grads=grads, batch=b)


def policy_fp32_distance(case):
    """rel-L2 of the fp32 evaluation of the reference from its float64 self: (forward, worst gradient tensor); the float64 run
    replays the fp32 run's PPO batch, so both differentiate the same loss."""
    kw, sd, batch = policy_inputs(*case)
    r32 = policy_reference(case, sd, batch, torch.float32)
    r64 = policy_reference(case, sd, batch, torch.float64, replay=r32["batch"])
    fwd = max(rel_l2(r32["logits"], r64["logits"]), rel_l2(r32["values"], r64["values"]), rel_l2(r32["state"], r64["state"]))
    grad = max(rel_l2(r32["grads"][k], r64["grads"][k]) for k in r64["grads"])
    return fwd, grad


if __name__ == "__main__":
    for case in POLICY_CASES:
        print("case", case, "fp32-vs-fp64 rel-L2 (forward, worst gradient tensor): %.3e %.3e" % policy_fp32_distance(case))

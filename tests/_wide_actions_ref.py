"""Float64 reference, case tables and seeded inputs for the wide action space (8 to 256 actions): the heads, the action selection
and the PPO loss (test infrastructure only; used by tests/test_wide_actions_ref.py on the CPU and tests/test_gpu_wide_actions.py).

Plain torch, dtype-generic.  Nothing here imports the product: the counter-based uniforms (ec_mix64), CategoricalDistr.sample /
mode (ec_sample_row / ec_mode_row, csrc/common.h) and the teacher-forcing rule (il_teacher_force_kernel) are restated.

Run as a program (CPU only, well under a minute), this file prints what the bounds of the GPU test are derived from: the worst
whole-tensor rel-L2 and the worst per-row figure (row error norm over the RMS row norm, tests/_act_route_ref.py::per_row) of
the SAME formulas evaluated in fp32 torch against float64, over the case tables below,

    python tests/_wide_actions_ref.py
"""
import torch

M64 = (1 << 64) - 1
TF_STREAM = 0x7465616368466F72          # "teachFor": the forcing draw's stream constant
STEP_MUL = 0x100000001B3


# ---- counter-based uniforms ---------------------------------------------------------------------------------------------------
def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def sample_uniform(seed, step, actor):
    """ec_sample_row's uniform of the key (seed, step, global actor id): 24 bits in [0, 1)"""
    h = mix64(mix64(seed) ^ ((step * STEP_MUL + actor) & M64))
    return (h >> 40) / 16777216.0


def force_uniform(seed, step, actor):
    """the teacher-forcing uniform of the same key: another stream"""
    h = mix64(mix64(mix64(seed) ^ TF_STREAM) ^ ((step * STEP_MUL + actor) & M64))
    return (h >> 40) / 16777216.0


# ---- CategoricalDistr ---------------------------------------------------------------------------------------------------------
def lse_rows(logits):
    mx = logits.max(dim=-1, keepdim=True).values
    return (mx + (logits - mx).exp().sum(dim=-1, keepdim=True).log()).squeeze(-1)


def mode_rows(logits):
    """-> (actions, logp): the FIRST index of the maximal logit"""
    A = logits.shape[-1]
    mx = logits.max(dim=-1, keepdim=True).values
    idx = torch.arange(A).expand_as(logits)
    a = torch.where(logits == mx, idx, torch.full_like(idx, A)).min(dim=-1).values
    return a, logits.gather(-1, a[:, None]).squeeze(-1) - lse_rows(logits)


def sample_rows(logits, seed, step, first_actor=0):
    """-> (actions, logp): inverse CDF, the first k with u < cdf_k (A - 1 when the rounded CDF stays below u)"""
    B, A = logits.shape
    lse = lse_rows(logits)
    cdf = (logits - lse[:, None]).exp().cumsum(dim=-1)
    u = torch.tensor([sample_uniform(seed, step, first_actor + n) for n in range(B)], dtype=logits.dtype)
    below = u[:, None] < cdf
    idx = torch.arange(A).expand_as(logits)
    a = torch.where(below, idx, torch.full_like(idx, A - 1)).min(dim=-1).values
    return a, logits.gather(-1, a[:, None]).squeeze(-1) - lse


def force_rows(logits, actions, logp, expert, mask, p, seed, step, first_actor=0):
    """TeacherForcingDistr behind a selection -> (actions, logp): where mask != 0 and u < p the expert's action and its
    log-prob (NaN for an id outside [0, A)); rows with mask 0 never look at their expert id"""
    B, A = logits.shape
    lse = lse_rows(logits)
    actions, logp = actions.clone(), logp.clone()
    for n in range(B):
        if mask[n] == 0 or not (force_uniform(seed, step, first_actor + n) < p):
            continue
        e = int(expert[n])
        actions[n] = e
        logp[n] = logits[n, e] - lse[n] if 0 <= e < A else float("nan")
    return actions, logp


# ---- heads --------------------------------------------------------------------------------------------------------------------
def heads_forward(hs, Wa, ba, wc, bc):
    """hv [B, A + 1] = [hs Wa^T + ba | hs wc + bc]"""
    return torch.cat([hs @ Wa.t() + ba, (hs @ wc.reshape(-1, 1)) + bc], dim=1)


def heads_backward(hs, Wa, wc, dhv):
    """-> (dhs, dWa, dba, dwc, dbc) of heads_forward for the output gradient dhv"""
    A = Wa.shape[0]
    dl, dv = dhv[:, :A], dhv[:, A:]
    return dl @ Wa + dv @ wc.reshape(1, -1), dl.t() @ hs, dl.sum(0), (dv.t() @ hs).reshape(wc.shape), dv.sum(0)


# ---- PPO ----------------------------------------------------------------------------------------------------------------------
def ppo_terms(hv, actions, old_logp, old_v, ret, nadv, clip, vclip):
    """per-row (action loss, value loss, -entropy, ratio, v) of [U] PPO.loss_per_step; vclip < 0: use_clipped_value_loss=False"""
    A = hv.shape[1] - 1
    lp = torch.log_softmax(hv[:, :A], dim=-1)
    v = hv[:, A]
    ratio = (lp.gather(-1, actions[:, None]).squeeze(-1) - old_logp).exp()
    la = -torch.min(ratio * nadv, ratio.clamp(1.0 - clip, 1.0 + clip) * nadv)
    if vclip >= 0:
        vcl = old_v + (v - old_v).clamp(-vclip, vclip)
        lv = 0.5 * torch.max((v - ret) ** 2, (vcl - ret) ** 2)
    else:
        lv = 0.5 * (ret - v) ** 2
    return la, lv, (lp.exp() * lp).sum(-1), ratio, v


def ppo_loss(inp, dtype=torch.float64):
    """-> (dhv [B, A + 1], sums4, terms [B, 4]) in `dtype`: dhv = grad_scale * d(mean la + vcoef mean lv + ecoef mean -H)/d(hv)
    by autograd; sums4 = the four per-row terms summed in float64"""
    f = lambda k: inp[k].to(dtype)
    hv = f("hv").clone().requires_grad_(True)
    la, lv, neg_ent, ratio, _ = ppo_terms(hv, inp["actions"], f("old_logp"), f("old_v"), f("ret"), f("nadv"), inp["clip"], inp["vclip"])
    total = (la.mean() + inp["vcoef"] * lv.mean() + inp["ecoef"] * neg_ent.mean()) * inp["grad_scale"]
    (dhv,) = torch.autograd.grad(total, hv)
    terms = torch.stack([la, lv, neg_ent, ratio], dim=1).detach()
    return dhv, terms.double().sum(0), terms


def ppo_branch_rows(inp, tol=1e-4):
    """rows of the float64 reference within `tol` (relative) of a branch point -- ratio = 1 +- clip, |v - v_old| = vclip,
    l1 = l2 with the value clip active: there an fp32 evaluation may take the other side, and the gradient jumps"""
    f = lambda k: inp[k].double()
    clip, vclip = inp["clip"], inp["vclip"]
    _, _, _, ratio, v = ppo_terms(f("hv"), inp["actions"], f("old_logp"), f("old_v"), f("ret"), f("nadv"), clip, vclip)
    near = ((ratio - (1 - clip)).abs() <= tol * (1 - clip)) | ((ratio - (1 + clip)).abs() <= tol * (1 + clip))
    if vclip >= 0:
        dv = v - f("old_v")
        near |= (dv.abs() - vclip).abs() <= tol * vclip
        vcl = f("old_v") + dv.clamp(-vclip, vclip)
        l1, l2 = (v - f("ret")) ** 2, (vcl - f("ret")) ** 2
        near |= (dv.abs() > vclip) & ((l1 - l2).abs() <= tol * torch.max(l1, l2))
    return near


# ---- figures ------------------------------------------------------------------------------------------------------------------
def rel_l2(got, ref):
    return ((got.double() - ref.double()).norm() / ref.double().norm().clamp_min(1e-30)).item()


def per_row(got, ref):
    e = (got.double() - ref.double()).norm(dim=-1)
    return (e.max() / ref.double().norm(dim=-1).pow(2).mean().sqrt().clamp_min(1e-30)).item()


def sums_err(got4, terms64):
    """error of the four sums relative to the sum of the terms' magnitudes (the action loss sums signed terms: relative to
    the sum itself the figure would measure the cancellation, not the arithmetic)"""
    return ((got4.double() - terms64.double().sum(0)).abs() / terms64.double().abs().sum(0).clamp_min(1e-30)).max().item()


# ---- case tables and seeded inputs ----------------------------------------------------------------------------------------------
# (A, H, B): every A, H and B of the issue's lists at least once; A around the 16-output passes and the 64-lane strides, H = 32
# (half of the 16 K-lanes idle) and 96 (a ragged second step), B = 1 / 5 (a ragged workgroup of 4 rows) / 37 / 130
HEADS_CASES = [(8, 32, 1), (8, 512, 37), (9, 96, 5), (9, 512, 130), (16, 32, 37), (16, 768, 5), (17, 96, 130), (17, 512, 1),
               (63, 32, 5), (63, 768, 37), (64, 96, 1), (64, 512, 5), (65, 32, 130), (65, 768, 1), (84, 96, 37), (84, 512, 130),
               (84, 768, 5), (255, 32, 37), (255, 512, 5), (255, 768, 130), (256, 96, 5), (256, 512, 37), (256, 768, 130),
               (256, 32, 1)]


def heads_inputs(A, H, B):
    g = torch.Generator().manual_seed(1000003 * A + 1009 * H + B)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(hs=torch.tanh(r(B, H)), Wa=r(A, H) / H ** 0.5, ba=0.1 * r(A), wc=r(H) / H ** 0.5, bc=0.1 * r(1))


# name -> dict(A, B, vclip (>= 0: clipped value loss), scale (of the logits), grad_scale)
PPO_CASES = {}
for _i, (_A, _B) in enumerate([(17, 1), (63, 15), (64, 16), (65, 17), (84, 257), (255, 2051), (256, 257), (17, 2051), (84, 2051),
                               (256, 17), (64, 2051), (255, 15)]):
    PPO_CASES["a%d_b%d" % (_A, _B)] = dict(A=_A, B=_B, vclip=0.1 if _i % 2 == 0 else -1.0, scale=1.0, grad_scale=1.0 if _i % 3 else 0.375)
PPO_CASES["a17_b16401"] = dict(A=17, B=16401, vclip=0.1, scale=1.0, grad_scale=1.0)      # past the block cap: 17-row chunks
PPO_CASES["a84_b257_scale30"] = dict(A=84, B=257, vclip=0.1, scale=30.0, grad_scale=1.0)  # near-one-hot rows
PPO_CASES["a84_b257_noclipv"] = dict(A=84, B=257, vclip=-1.0, scale=1.0, grad_scale=2.5)
PPO_CASES["a6_b257"] = dict(A=6, B=257, vclip=0.1, scale=1.0, grad_scale=1.0)            # beside ec_ppo_loss_ex
PPO_CASES["a16_b257"] = dict(A=16, B=257, vclip=0.1, scale=1.0, grad_scale=1.0)


def ppo_inputs(name):
    """seeded rollout-like rows: actions drawn from the policy, old log-probs 0.12 sigma around the new ones (ratios on both
    sides of 1 +- 0.1), old values 0.15 sigma around the values (both sides of the value clip)"""
    c = PPO_CASES[name]
    A, B = c["A"], c["B"]
    g = torch.Generator().manual_seed(7919 * A + B + int(c["scale"]) + (1 if c["vclip"] < 0 else 0))
    r = lambda *s: torch.randn(*s, generator=g)
    hv = torch.cat([c["scale"] * r(B, A), r(B, 1)], dim=1)
    lp = torch.log_softmax(hv[:, :A].double(), dim=-1)
    actions = torch.multinomial(lp.exp().float().clamp_min(1e-30), 1, generator=g).squeeze(-1)
    old_logp = (lp.gather(-1, actions[:, None]).squeeze(-1) + 0.12 * r(B).double()).float()
    return dict(hv=hv, actions=actions, old_logp=old_logp, old_v=hv[:, A] + 0.15 * r(B), ret=hv[:, A] + r(B), nadv=r(B), clip=0.1,
                vclip=c["vclip"], vcoef=0.5, ecoef=0.01, grad_scale=c["grad_scale"])


def heads_fp32_figures():
    """worst (logits rel, logits row, values rel, values row) of fp32 torch against float64 over HEADS_CASES"""
    w = [0.0] * 4
    for (A, H, B) in HEADS_CASES:
        inp = heads_inputs(A, H, B)
        ref = heads_forward(*(inp[k].double() for k in ("hs", "Wa", "ba", "wc", "bc")))
        got = heads_forward(*(inp[k] for k in ("hs", "Wa", "ba", "wc", "bc")))
        f = (rel_l2(got[:, :A], ref[:, :A]), per_row(got[:, :A], ref[:, :A]), rel_l2(got[:, A:], ref[:, A:]), per_row(got[:, A:], ref[:, A:]))
        print("heads A %3d H %3d B %3d  logits %.2e / %.2e  values %.2e / %.2e" % ((A, H, B) + f), flush=True)
        w = [max(a, b) for a, b in zip(w, f)]
    return w


def ppo_fp32_figures():
    """worst (dhv rel, dhv row, sums) of fp32 torch against float64 over PPO_CASES, branch-point rows left out of the
    element figures; also the worst excluded fraction"""
    w, frac = [0.0] * 3, 0.0
    for name in PPO_CASES:
        inp = ppo_inputs(name)
        keep = ~ppo_branch_rows(inp)
        d64, _, t64 = ppo_loss(inp)
        d32, s32, _ = ppo_loss(inp, torch.float32)
        f = (rel_l2(d32[keep], d64[keep]), per_row(d32[keep], d64[keep]), sums_err(s32, t64))
        frac = max(frac, 1.0 - keep.float().mean().item())
        print("ppo %-18s dhv %.2e / %.2e  sums %.2e  excluded %d of %d" % ((name,) + f + (int((~keep).sum()), keep.numel())), flush=True)
        w = [max(a, b) for a, b in zip(w, f)]
    return w, frac


if __name__ == "__main__":
    h = heads_fp32_figures()
    p, frac = ppo_fp32_figures()
    print("heads, fp32 vs float64, worst: logits rel-L2 %.3e per-row %.3e; values rel-L2 %.3e per-row %.3e" % tuple(h))
    print("ppo,   fp32 vs float64, worst: dhv rel-L2 %.3e per-row %.3e; sums %.3e; worst excluded fraction %.4f" % (tuple(p) + (frac,)))

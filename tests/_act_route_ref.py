"""Inputs, float64 reference and error figures for the cases of tests/_act_route_cases.py (test infrastructure only; used by
tests/test_gpu_act_routes.py in-process and by tests/_act_route_check.py in a child process).

The reference is the ORACLE's forward (oracle/policy.py::actor_critic_forward; tests/_pointnav_ref.py for coordinate goals)
on the state dict and every input cast to float64 -- both are written in dtype-generic torch ops, nothing in them pins fp32.
bf16 features are rounded to bf16 first and then cast, so the reference sees exactly the numbers the kernels read.

Run as a program (CPU only, ~1 min), this file measures what the per-actor bound of the GPU test is derived from: the worst
per-row error of the fp32 oracle against the float64 oracle over the whole case table,

    python tests/_act_route_ref.py
"""
import os
import sys
import zlib

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _act_route_cases as cases  # noqa: E402

OUTPUTS = ("logits", "values", "h_final")


def state_dict(case):
    from embodied_clip_amd import synthetic as syn
    return syn.policy_state_dict(0, **cases.cfg_of(case))


def make_inputs(case, name, draw=0):
    """feat (and feat2) [T*N, S*S, C] bf16 / fp32 rows = abs(randn) * 0.5; a different goal per neighbouring actor; h0 = 0.3 *
    randn; masks with ~20 % zeros, at least one zero and one one.  `draw` 1: the new inputs of a reuse pair's second call."""
    from embodied_clip_amd import synthetic as syn
    cfg, T, N = cases.cfg_of(case), case["T"], case["N"]
    seed = zlib.crc32(name.encode()) + 7919 * draw
    g = torch.Generator().manual_seed(seed)
    S, C, B = cfg["spatial"] ** 2, cfg["in_channels"], T * N
    dt = torch.bfloat16 if case["bf16"] else torch.float32
    feats = [(torch.randn(B, S, C, generator=g).abs() * 0.5).to(dt) for _ in range(1 + cfg["dual"])]
    if cfg["goal_in"]:
        goal = syn.synthetic_goal_vectors(seed % 1000003, (T, N), cfg["goal_in"])
        assert len({tuple(v) for v in goal.reshape(B, -1).tolist()}) == B
    else:
        goal = ((torch.arange(B) * 5 + 1 + draw) % cfg["num_goals"]).reshape(T, N)
        assert B < 2 or (goal.reshape(-1)[1:] != goal.reshape(-1)[:-1]).all()
    h0 = 0.3 * torch.randn(N, cfg["hidden"], generator=g)
    masks = (torch.rand(T, N, generator=g) >= 0.2).float()
    masks.view(-1)[0] = 1.0
    if B > 1:
        masks.view(-1)[-1] = 0.0
        assert (masks == 0).any() and (masks == 1).any()
    return dict(feat=feats[0], feat2=feats[1] if cfg["dual"] else None, goal=goal, h0=h0, masks=masks)


def slice_inputs(inp, n):
    """actors 0..n-1 of a T = 1 call's inputs"""
    return dict(feat=inp["feat"][:n].contiguous(), feat2=None if inp["feat2"] is None else inp["feat2"][:n].contiguous(),
                goal=inp["goal"][:, :n].contiguous(), h0=inp["h0"][:n].contiguous(), masks=inp["masks"][:, :n].contiguous())


def oracle(case, sd, inp, dtype=torch.float64):
    """-> dict(logits [B, A], values [B, 1], h_final [N, H]) in `dtype`"""
    from oracle import policy as opol
    import _pointnav_ref
    cfg, T, N = cases.cfg_of(case), case["T"], case["N"]
    s = cfg["spatial"]
    sdd = {k: v.to(dtype) for k, v in sd.items()}
    nchw = lambda f: f.float().to(dtype).view(T, N, s, s, cfg["in_channels"]).permute(0, 1, 4, 2, 3).contiguous()
    feat = (nchw(inp["feat"]), nchw(inp["feat2"])) if cfg["dual"] else nchw(inp["feat"])
    h0, masks = inp["h0"].to(dtype).unsqueeze(0), inp["masks"].to(dtype).unsqueeze(-1)
    with torch.no_grad():
        if cfg["goal_in"]:
            lg, vv, hf = _pointnav_ref.actor_critic_forward(feat, inp["goal"].to(dtype), h0, masks, sdd)
        else:
            lg, vv, hf = opol.actor_critic_forward(feat, inp["goal"], h0, masks, sdd)
    assert lg.dtype == vv.dtype == hf.dtype == dtype
    return dict(logits=lg.reshape(T * N, -1), values=vv.reshape(T * N, 1), h_final=hf[0])


def rel_l2(got, ref):
    return ((got.double() - ref.double()).norm() / ref.double().norm().clamp_min(1e-30)).item()


def per_row(got, ref):
    """the worst row's error norm relative to the RMS row norm of the reference: one wrong actor among many shows here in
    full, where the whole-tensor figure divides it by sqrt(rows)"""
    e = (got.double() - ref.double()).norm(dim=-1)
    return (e.max() / ref.double().norm(dim=-1).pow(2).mean().sqrt().clamp_min(1e-30)).item()


def figures(got, ref):
    """got / ref: dicts of OUTPUTS -> {output: (rel-L2, per-row)}"""
    return {k: (rel_l2(got[k], ref[k]), per_row(got[k], ref[k])) for k in OUTPUTS}


def split_hv(hv, h_final, A):
    hv = hv.float().cpu()
    return dict(logits=hv[:, :A], values=hv[:, A:], h_final=h_final.float().cpu())


def gpu_forward(handle, flat, inp, case, dev, ws=None, reuse=False, fill=0):
    """one inference call; a workspace of its own (filled with the byte `fill`) unless `ws` is given -> (outputs, workspace)"""
    T, N = case["T"], case["N"]
    if ws is None:
        ws = torch.full((handle.workspace_bytes(T, N, False),), fill, dtype=torch.uint8, device=dev)
    goal = inp["goal"].reshape(T * N, -1).contiguous() if handle.goal_in else inp["goal"].reshape(-1)
    hv, hf = handle.forward(flat, inp["feat"].to(dev), goal.to(dev), inp["h0"].to(dev), inp["masks"].reshape(-1).to(dev), T, N, ws,
                            for_backward=False, reuse_tables=reuse, feat2=None if inp["feat2"] is None else inp["feat2"].to(dev))
    torch.cuda.synchronize()
    return split_hv(hv, hf, handle.A), ws


def run_case(name, dev):
    """The GPU side of one case -> dict(figs=[{output: (rel, row)} per call], equal=bool): every call against the float64
    oracle, and the whole case a second time in fresh workspaces (filled with other bytes) for bit equality."""
    from embodied_clip_amd.policy import PolicyHandle
    case = cases.CASES[name]
    handle = PolicyHandle(**cases.cfg_of(case))
    sd = state_dict(case)
    flat = handle.flatten(sd, dev)
    draws = [make_inputs(case, name, d) for d in range(2 if case["mode"] == "reuse" else 1)]
    runs = []
    for fill in (0xFF, 0x00):                     # (0xFF: every float of the workspace starts as a NaN)
        ws, outs = None, []
        for d, inp in enumerate(draws):
            out, ws = gpu_forward(handle, flat, inp, case, dev, ws=ws, reuse=d > 0, fill=fill)
            outs.append(out)
        runs.append(outs)
    equal = all(torch.equal(a[k], b[k]) for a, b in zip(*runs) for k in OUTPUTS)
    figs = [figures(out, oracle(case, sd, inp)) for out, inp in zip(runs[0], draws)]
    return dict(figs=figs, equal=equal, outs=runs[0], draws=draws)


def worst(figs_list):
    """-> (worst rel-L2, worst per-row) over calls and outputs"""
    return (max(f[k][0] for f in figs_list for k in OUTPUTS), max(f[k][1] for f in figs_list for k in OUTPUTS))


if __name__ == "__main__":
    torch.manual_seed(0)
    top = {k: (0.0, 0.0, "") for k in OUTPUTS}
    for name, case in cases.CASES.items():
        sd = state_dict(case)
        for d in range(2 if case["mode"] == "reuse" else 1):
            inp = make_inputs(case, name, d)
            f = figures(oracle(case, sd, inp, torch.float32), oracle(case, sd, inp))
            print("%-22s draw %d  " % (name, d) + "  ".join("%s %.2e / %.2e" % (k, *f[k]) for k in OUTPUTS), flush=True)
            for k in OUTPUTS:
                assert f[k][0] < 2e-5, (name, k, f[k])
                if f[k][1] > top[k][1]:
                    top[k] = (f[k][0], f[k][1], name)
    print("fp32 oracle vs float64 oracle, worst per-row figure:", {k: (v[1], v[2]) for k, v in top.items()})
    print("worst of all: %.3e" % max(v[1] for v in top.values()))

"""Run as a subprocess by tests/test_gpu_prev_action.py (the library reads EC_WIH_PERM once per process): one policy case with a
previous-action embedding -- the inference forward, the T = 1 act step and one learn pass (forward, PPO loss, backward twice) --
against tests/_prev_action_ref.py; prints the forward / per-tensor gradient errors as JSON."""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

CASE = (3, 5, 7, 64, 32, 6, 1, 6, 0, False)


def main():
    import _prev_action_ref as ref
    from embodied_clip_amd import ppo
    from embodied_clip_amd.policy import PolicyHandle
    T, N, A, null = CASE[0], CASE[1], CASE[7], CASE[6]
    dev = torch.device("cuda:0")
    cfg, sd, batch = ref.policy_inputs(*CASE)
    r = ref.policy_reference(sd, batch, null)
    b = r["batch"]
    h = PolicyHandle(**cfg)
    flat = h.flatten(sd, dev)
    rows = b["feat"].permute(0, 1, 3, 4, 2).reshape(T * N, cfg["spatial"] ** 2, cfg["in_channels"]).contiguous().to(dev)
    f = lambda t: t.reshape(-1).contiguous().to(dev)
    goal, prev, m, h0 = f(b["goal"]), f(b["prev_actions"]), f(b["masks"]), b["h0"][0].contiguous().to(dev)
    rel = lambda a, c: ((a.double().cpu() - c.double()).norm() / c.double().norm().clamp_min(1e-30)).item()
    # inference forward over all T, then the act step (T = 1) against the reference's first step
    ws = torch.empty(h.workspace_bytes(T, N, False), dtype=torch.uint8, device=dev)
    hv, hf = h.forward(flat, rows, goal, h0, m, T, N, ws, for_backward=False, prev_actions=prev)
    hv3 = hv.view(T, N, A + 1)
    fwd = [rel(hv3[..., :A], r["logits"]), rel(hv3[..., A:], r["values"]), rel(hf, r["h"][0])]
    ws1 = torch.empty(h.workspace_bytes(1, N, False), dtype=torch.uint8, device=dev)
    hv1, _ = h.forward(flat, rows[:N].contiguous(), goal[:N].contiguous(), h0, m[:N].contiguous(), 1, N, ws1, for_backward=False,
                       prev_actions=prev[:N].contiguous())
    act = [rel(hv1[:, :A], r["logits"][0]), rel(hv1[:, A:], r["values"][0])]
    # learn pass
    wsl = torch.empty(h.workspace_bytes(T, N, True), dtype=torch.uint8, device=dev)
    hvl, _ = h.forward(flat, rows, goal, h0, m, T, N, wsl, prev_actions=prev)
    dhv, _ = ppo.ppo_loss_raw(hvl, f(b["actions"]), f(b["old_log_probs"]), f(b["old_values"]), f(b["returns"]), f(b["norm_adv"]), A)
    g1, g2 = torch.zeros_like(flat), torch.zeros_like(flat)
    h.backward(flat, rows, m, T, N, wsl, dhv, None, g1)
    h.backward(flat, rows, m, T, N, wsl, dhv, None, g2)
    torch.cuda.synchronize()
    gv, ga = h.views(g1), h.views(g2)
    wih = "state_encoder.rnn.weight_ih_l0"
    out = {"wih_perm": os.environ.get("EC_WIH_PERM", "1"), "forward": fwd, "act": act,
           "grads": {n: rel(gv[n], r["ref_grads"][n]) for n in gv},
           "deterministic": bool(torch.equal(gv[ref.EMB_KEY], ga[ref.EMB_KEY]) and torch.equal(gv[wih], ga[wih]))}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""Run as a subprocess by tests/test_gpu_wide_actions_engine.py (the engine reads EC_ACT_FUSED_SAMPLE when a worker is built, the
library its switches once per process): one iteration of the test's worker under the environment it was started with; the
rollout and the parameters go to the file named on the command line.

    python tests/_wide_actions_engine_check.py <num_actions> <loss> <out.pt>
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def build_worker(num_actions, loss, N=6, T=4, seed=11, **kw):
    """the tiny worker of tests/test_gpu_imitation_engine.py at another action count"""
    from embodied_clip_amd import synthetic as syn
    from embodied_clip_amd.engine import Worker
    import _imitation_ref as iref
    kw.setdefault("update_repeats", 2)
    if loss != "ppo":
        kw.setdefault("teacher_forcing", lambda s: 0.5)
    w = Worker(N, T=T, device="cuda:0", seed=seed, encoder_sd=syn.rn50_visual_state_dict(0),
               policy_sd=syn.policy_state_dict(0, num_actions=num_actions), num_actions=num_actions, loss=loss, **kw)
    if hasattr(w.env, "expert_mask"):       # both mask values at these small shapes; ids of steps without an expert action: -1
        m = iref.engine_test_mask(w.T, w.N).to(w.env.expert_mask.device)
        w.env.expert_mask.copy_(m)
        w.env.expert_actions[m == 0] = -1
    return w


def record_hv(w):
    """wrap the worker's act step: the slice's rows of ``hv_act`` after every call, as ``hv_steps`` [T + 1, N, A + 1] (the
    last row is the bootstrap step's) -- on the slice's stream, behind the call"""
    orig = w._act_slice
    w.hv_steps = torch.zeros((w.T + 1, w.N, w.A + 1), dtype=torch.float32, device=w.hv_act.device)
    torch.cuda.synchronize()                # (the slices run on streams of their own)

    def act_slice(sl, t, *a, **k):
        orig(sl, t, *a, **k)
        w.hv_steps[t, sl.o:sl.o + sl.n].copy_(w.hv_act[sl.o:sl.o + sl.n])
    w._act_slice = act_slice


def snapshot(w):
    torch.cuda.synchronize()
    keys = ("actions", "logp", "values", "hv_act", "params") + (("hv_steps",) if hasattr(w, "hv_steps") else ())
    return {k: getattr(w, k).detach().cpu().clone() for k in keys}


if __name__ == "__main__":
    w = build_worker(int(sys.argv[1]), sys.argv[2])
    record_hv(w)
    w.iteration()
    out = snapshot(w)
    out["act_wide"], out["act_fused"] = bool(w._act_wide), bool(w._act_fused)
    torch.save(out, sys.argv[3])

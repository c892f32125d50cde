"""Float64 reference of the imitation loss, a bit-for-bit restatement of the teacher-forcing draw, and the engine tests'
update-tolerance rule.  Shared by the CPU and GPU imitation tests; test infrastructure only."""
import numpy as np
import torch

TF_SEED, TF_STEPS, TF_N, TF_A = 11, 8, 4096, 6      # the teacher-forcing statistics case (CPU and GPU tests use the same)


def imitation_ref(hv, expert, mask, weight=1.0, grad_scale=1.0, denom=None, dhv0=None):
    """[U] allenact Imitation.loss for a CategoricalDistr in float64.  hv [B, A+1] (logits, value); expert int64 [B]; mask [B].
    ``denom``: the shared normaliser instead of this batch's own ``mask.sum()``; ``dhv0``: the accumulate form (the term is
    added to it; masked-out rows and the value column keep its values).  An expert id is only used as an index where
    ``mask != 0``.  -> (loss, dhv [B, A+1], sums3 = [sum mask * -logp_e, sum mask, sum mask * [argmax == e]])."""
    hv, mask = hv.double(), mask.double()
    B, A = hv.shape[0], hv.shape[1] - 1
    lp = torch.log_softmax(hv[:, :A], dim=-1)
    on = mask != 0
    e = torch.where(on, expert, torch.zeros_like(expert))
    lpe = lp.gather(1, e[:, None])[:, 0]
    D = float(mask.sum()) if denom is None else float(denom)
    Dc = max(D, 1.0)
    nll = -(mask * lpe)[on].sum()
    agree = (mask * (hv[:, :A].argmax(-1) == e).double())[on].sum()
    sums3 = torch.stack([nll, mask.sum(), agree])
    onehot = torch.zeros(B, A, dtype=torch.float64)
    onehot[torch.arange(B), e] = 1.0
    term = torch.zeros(B, A + 1, dtype=torch.float64)
    term[:, :A] = grad_scale * weight * mask[:, None] * (lp.exp() - onehot) / Dc
    dhv = term if dhv0 is None else dhv0.double() + term
    return nll / Dc, dhv, sums3


def make_case(B, A, scale=1.0, mask_kind="mixed", seed=0):
    """Deterministic inputs (hv fp32 [B, A+1], expert int64 [B], mask fp32 [B]); row maxima are unique by construction."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * B + A)
    hv = torch.randn(B, A + 1, generator=g, dtype=torch.float32) * scale
    # a unique maximum per row: lift one logit clearly above the others
    top = torch.randint(0, A, (B,), generator=g)
    hv[torch.arange(B), top] = hv[:, :A].max(dim=1).values + 0.25 * scale
    expert = torch.randint(0, A, (B,), generator=g)
    expert[::3] = top[::3]                                   # the expert agrees with the arg-max on some rows
    if mask_kind == "ones":
        mask = torch.ones(B)
    elif mask_kind == "zeros":
        mask = torch.zeros(B)
    else:
        mask = (torch.rand(B, generator=g) > 0.3).float()
    return hv, expert, mask


# ---- the engine tests' expert mask ---------------------------------------------------------------------------------------
ENGINE_SHAPES = ((3, 2), (3, 5), (2, 64), (8, 4), (4, 64), (8, 6))       # (T, N) of tests/test_gpu_imitation_engine.py


def engine_test_mask(T, N):
    """fp32 [T+1, N]: the expert mask the engine tests install (p_fail 0.3 instead of the env's 0.05, so that the few steps of
    these small rollouts hold both values; tests/test_imitation_synthetic.py checks that they do)."""
    from embodied_clip_amd import synthetic as syn
    return syn.synthetic_expert(77, torch.zeros(T + 1, N, dtype=torch.int64), 6, p_fail=0.3)[1]


# ---- the teacher-forcing draw (csrc/imitation.hip il_teacher_force_kernel; ec_mix64 of csrc/common.h) ------------------------------
_M = np.uint64(0xFFFFFFFFFFFFFFFF)
TF_STREAM = 0x7465616368466f72


def _mix64(z):
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z + np.uint64(0x9E3779B97F4A7C15)) & _M
        z = ((z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)) & _M
        z = ((z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)) & _M
        return z ^ (z >> np.uint64(31))


def teacher_force_uniform(seed, step, actors):
    """float32 uniforms in [0, 1) (24 bits) of global actors ``actors`` at ``step``."""
    with np.errstate(over="ignore"):
        key = _mix64(np.uint64(seed)) ^ np.uint64(TF_STREAM)
        ctr = (np.uint64(step) * np.uint64(0x100000001B3) + np.asarray(actors, dtype=np.uint64)) & _M
        h = _mix64(_mix64(key) ^ ctr)
    return ((h >> np.uint64(40)).astype(np.float64) * (1.0 / 16777216.0)).astype(np.float32)


def sampler_uniform(seed, step, actors):
    """The uniform ec_sample_row draws for the same key (csrc/common.h): another stream."""
    with np.errstate(over="ignore"):
        ctr = (np.uint64(step) * np.uint64(0x100000001B3) + np.asarray(actors, dtype=np.uint64)) & _M
        h = _mix64(_mix64(np.uint64(seed)) ^ ctr)
    return ((h >> np.uint64(40)).astype(np.float64) * (1.0 / 16777216.0)).astype(np.float32)


def teacher_force_decisions(seed, step, first_actor, mask, p):
    """bool [N]: the rows ec_teacher_force forces."""
    mask = np.asarray(mask)
    u = teacher_force_uniform(seed, step, first_actor + np.arange(mask.shape[0]))
    return (mask != 0) & (u < np.float32(p))


# ---- tests/test_gpu_engine.py::_check_updates, restated -----------------------------------------------------------------------------
def check_updates(pv, sd0, sd_ref, step_grads, steps, lr=3e-4):
    """Parameter updates after ``steps`` Adam steps, HIP vs oracle: an element whose gradient stays at the fp32 noise floor of
    its tensor (every step's |g| < 1e-4 of the tensor's largest) only gets the bound a full sign flip can reach (2 lr per
    step); every other element must agree to 0.15 lr per step."""
    for name, pref in sd_ref.items():
        upd, upd_ref = pv[name].cpu() - sd0[name], pref - sd0[name]
        d = (upd - upd_ref).abs()
        gmax = torch.stack([g[name].abs() for g in step_grads]).amax(0)
        well = gmax > 1e-4 * gmax.max()
        assert d.max() <= 2 * steps * lr + 1e-7, (name, d.max())
        if well.any():
            assert d[well].max() < 0.15 * steps * lr + 1e-7, (name, d[well].max())

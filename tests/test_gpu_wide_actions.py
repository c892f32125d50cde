"""GPU: the kernels of the wide action space (8 to 256 actions; csrc/wide_actions.hip) against float64, each alone and through
ec_policy_act_ex.

Bounds.  The heads and the PPO loss differ from an fp32 evaluation of the same formulas only in summation order and in the
device's exp / log (2^-24-class), so each bound is 8 x the worst figure of FP32 TORCH against float64 over the same case tables
(`python tests/_wide_actions_ref.py`, CPU; the margin of tests/test_gpu_act_routes.py, for its reason) -- never a figure of
the kernels under test:

    heads (24 cases):   logits rel-L2 3.615e-07, per-row 5.674e-07;  values rel-L2 3.319e-07, per-row 6.357e-07
    PPO   (17 cases):   dhv rel-L2 1.724e-07, per-row 1.471e-06;  the four sums 1.245e-07 (relative to the sum of the terms'
                        magnitudes);  rows within 1e-4 of a branch point: at most 13 of 16401 (0.39 % of a case; cap 2 %)

per-row = the worst row's error norm over the RMS row norm (tests/_act_route_ref.py::per_row).  The selection is held to BIT
equality with ec_sample_actions / ec_mode_actions / ec_teacher_force on the hv the fused launch wrote; ec_policy_act_ex to the
float64 policy oracle at the act-route bounds of tests/test_gpu_act_routes.py."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _act_route_ref as aref  # noqa: E402
import _wide_actions_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

FP32_HEADS = dict(logits=(3.615e-07, 5.674e-07), values=(3.319e-07, 6.357e-07))     # measured on the CPU: see the docstring
FP32_PPO_DHV = (1.724e-07, 1.471e-06)
FP32_PPO_SUMS = 1.245e-07
MARGIN = 8
ACT_REL_BOUND, ACT_PER_ROW_BOUND = 2e-5, 8 * 1.99e-6                                # tests/test_gpu_act_routes.py
DEV = "cuda:0"


def _lib():
    from embodied_clip_amd import _lib as L
    return L, L.load()


def _heads(inp, B=None, fill=float("nan"), select=None, seed=0, step=0, first=0, expert=None, mask=None, p=0.0):
    """ec_heads_wide on the first B rows -> (hv, actions, logp, values); select None / "sample" / "greedy\""""
    L, lib = _lib()
    t = {k: v.to(DEV).contiguous() for k, v in inp.items()}
    A, H = t["Wa"].shape
    B = t["hs"].shape[0] if B is None else B
    hv = torch.full((B, A + 1), fill, dtype=torch.float32, device=DEV)
    actions = torch.full((B,), -7, dtype=torch.int64, device=DEV)
    logp = torch.full((B,), fill, dtype=torch.float32, device=DEV)
    values = torch.full((B,), fill, dtype=torch.float32, device=DEV)
    on = select is not None
    L.check(lib.ec_heads_wide(t["hs"].data_ptr(), t["Wa"].data_ptr(), t["ba"].data_ptr(), t["wc"].data_ptr(), t["bc"].data_ptr(),
                              hv.data_ptr(), B, H, A, actions.data_ptr() if on else None, logp.data_ptr() if on else None,
                              values.data_ptr() if on else None, int(select == "greedy"), seed, step, first, L.ptr(expert), L.ptr(mask), p,
                              L.stream_ptr()), "ec_heads_wide")
    torch.cuda.synchronize()
    return hv, actions, logp, values


# ---- 1. the heads alone ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,H,B", ref.HEADS_CASES)
def test_heads_against_float64(A, H, B):
    inp = ref.heads_inputs(A, H, B)
    want = ref.heads_forward(*(inp[k].double() for k in ("hs", "Wa", "ba", "wc", "bc")))
    hv, _, _, _ = _heads(inp)
    hv0, _, _, _ = _heads(inp, fill=0.0)
    got = hv.cpu()
    figs = {}
    for k, sl in (("logits", slice(0, A)), ("values", slice(A, A + 1))):
        figs[k] = (ref.rel_l2(got[:, sl], want[:, sl]), ref.per_row(got[:, sl], want[:, sl]))
        print("heads A %d H %d B %d %s: rel-L2 %.3e per-row %.3e" % (A, H, B, k, *figs[k]))
    for k, (rel, row) in figs.items():
        assert rel < MARGIN * FP32_HEADS[k][0], (k, rel)
        assert row < MARGIN * FP32_HEADS[k][1], (k, row)
    assert torch.equal(hv, hv0), "NaN-filled and zero-filled outputs differ"


@pytest.mark.parametrize("A,H", [(84, 512), (255, 96), (9, 768)])
def test_heads_rows_do_not_depend_on_the_batch(A, H):
    inp = ref.heads_inputs(A, H, 130)
    whole = _heads(inp, select="sample", seed=3, step=4)
    part = _heads(inp, B=41, select="sample", seed=3, step=4)
    for w, q in zip(whole, part):
        assert torch.equal(w[:41], q)


# ---- 2. the selection is the shared function, bit for bit ------------------------------------------------------------------------
def _selection_rows(A, B=37):
    """logits through the heads: hs = I (H = B padded to 4), so Wa^T holds the logits we want; special rows on top"""
    g = torch.Generator().manual_seed(A)
    H = (B + 3) // 4 * 4
    logits = 2.0 * torch.randn(B, A, generator=g)
    logits[1, 5] = logits[1, 2] = logits[1].max() + 1.0                    # tied maxima -> the first index
    logits[2, :] = 0.25                                                     # all tied
    logits[3] = 30.0 * torch.randn(A, generator=g)                          # near one-hot
    logits[4, A - 1] = logits[4].max() + 40.0                               # the last action, all others underflow to tiny terms
    hs = torch.zeros(B, H)
    hs[:, :B] = torch.eye(B)
    Wa = torch.zeros(A, H)
    Wa[:, :B] = logits.t()
    return dict(hs=hs, Wa=Wa, ba=torch.zeros(A), wc=torch.randn(H, generator=g), bc=torch.zeros(1)), logits


def _shared(hv, A, select, seed, step, first, expert=None, mask=None, p=0.0):
    L, lib = _lib()
    B = hv.shape[0]
    actions = torch.full((B,), -7, dtype=torch.int64, device=DEV)
    logp = torch.full((B,), float("nan"), dtype=torch.float32, device=DEV)
    values = torch.full((B,), float("nan"), dtype=torch.float32, device=DEV)
    if select == "greedy":
        L.check(lib.ec_mode_actions(hv.data_ptr(), actions.data_ptr(), logp.data_ptr(), values.data_ptr(), B, A, L.stream_ptr()))
    else:
        L.check(lib.ec_sample_actions(hv.data_ptr(), actions.data_ptr(), logp.data_ptr(), values.data_ptr(), B, A, seed, step, first,
                                      L.stream_ptr()))
    if expert is not None:
        L.check(lib.ec_teacher_force(hv.data_ptr(), expert.data_ptr(), mask.data_ptr(), p, actions.data_ptr(), logp.data_ptr(), B, A,
                                     seed, step, first, L.stream_ptr()))
    torch.cuda.synchronize()
    return actions, logp, values


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))           # (NaN log-probs compare by their bits)


@pytest.mark.parametrize("first", [0, 1000])
@pytest.mark.parametrize("A", [8, 84, 256])
@pytest.mark.parametrize("select", ["sample", "greedy"])
def test_selection_equals_the_shared_functions(select, A, first):
    inp, logits = _selection_rows(A)
    hv, actions, logp, values = _heads(inp, select=select, seed=11, step=5, first=first)
    assert torch.equal(hv[:, :A].cpu(), logits), "identity rows: the logits come through exactly"
    a2, lp2, v2 = _shared(hv, A, select, 11, 5, first)
    assert torch.equal(actions, a2) and _same_bits(logp, lp2) and _same_bits(values, v2)
    assert int(actions.min()) >= 0 and int(actions.max()) < A
    if select == "greedy":
        assert actions[1] == 2 and actions[2] == 0 and actions[4] == A - 1
        assert torch.equal(actions.cpu(), ref.mode_rows(logits.double())[0])
    else:
        assert actions[4] == A - 1 and torch.isfinite(logp).all()


@pytest.mark.parametrize("first", [0, 1000])
@pytest.mark.parametrize("A", [8, 84, 256])
@pytest.mark.parametrize("p", [0.5, 1.0])
def test_forcing_equals_the_shared_function(p, A, first):
    inp, logits = _selection_rows(A)
    B = logits.shape[0]
    g = torch.Generator().manual_seed(A + 1)
    expert = torch.randint(0, A, (B,), generator=g)
    mask = (torch.rand(B, generator=g) < 0.7).float()
    mask[:8] = torch.tensor([1, 1, 1, 1, 1, 0, 1, 1.0])
    expert[mask == 0] = 1 << 40                                             # garbage: never read
    expert[6], expert[7] = A, -1                                            # present and out of range -> NaN log-prob
    expert, mask = expert.to(DEV), mask.to(DEV)
    hv, actions, logp, values = _heads(inp, select="sample", seed=11, step=5, first=first, expert=expert, mask=mask, p=p)
    a2, lp2, v2 = _shared(hv, A, "sample", 11, 5, first, expert, mask, p)
    assert torch.equal(actions, a2) and _same_bits(logp, lp2) and _same_bits(values, v2)
    free = _shared(hv, A, "sample", 11, 5, first)
    off = (mask == 0)
    assert torch.equal(actions[off], free[0][off]) and _same_bits(logp[off], free[1][off])       # mask 0: untouched
    mask_c = mask.cpu()
    forced = torch.tensor([bool(mask_c[n] != 0) and ref.force_uniform(11, 5, first + n) < p for n in range(B)])
    assert torch.equal(actions.cpu()[forced], expert.cpu()[forced])
    assert 0 < int(forced.sum()) and (p == 1.0 or int(forced.sum()) < int((mask != 0).sum()))
    if p == 1.0:
        assert actions[6] == A and actions[7] == -1 and torch.isnan(logp[6]) and torch.isnan(logp[7])
        assert int(torch.isnan(logp).sum()) == 2


# ---- 3. ec_policy_act_ex end to end -----------------------------------------------------------------------------------------------
C128 = dict(in_channels=128)
ACT_CASES = {
    "wide_a9": dict(cfg=dict(num_actions=9, **C128), T=1, N=33, bf16=1, mode="infer"),
    "wide_a84": dict(cfg=dict(num_actions=84, **C128), T=1, N=33, bf16=1, mode="infer"),
    "wide_a84_vec": dict(cfg=dict(num_actions=84, goal_in=2, **C128), T=1, N=33, bf16=1, mode="infer"),
    "wide_a84_dual": dict(cfg=dict(num_actions=84, dual=1, in_channels=256), T=1, N=8, bf16=1, mode="infer"),
    "wide_a84_reuse": dict(cfg=dict(num_actions=84, **C128), T=1, N=33, bf16=1, mode="reuse"),
}


def _act_ex(handle, flat, inp, case, ws, reuse, **kw):
    N = case["N"]
    goal = inp["goal"].reshape(N, -1).contiguous() if handle.goal_in else inp["goal"].reshape(-1)
    hv = torch.full((N, handle.A + 1), float("nan"), dtype=torch.float32, device=DEV)
    hf = torch.full((N, handle.H), float("nan"), dtype=torch.float32, device=DEV)
    actions = torch.full((N,), -7, dtype=torch.int64, device=DEV)
    logp, values = torch.full((N,), float("nan"), device=DEV), torch.full((N,), float("nan"), device=DEV)
    handle.act_ex(flat, inp["feat"].to(DEV), goal.to(DEV), inp["h0"].to(DEV), inp["masks"].reshape(-1).to(DEV), N, ws, hv, hf, actions,
                  logp, values, reuse_tables=reuse, feat2=None if inp["feat2"] is None else inp["feat2"].to(DEV), **kw)
    torch.cuda.synchronize()
    return hv, hf, actions, logp, values


@pytest.mark.parametrize("name", list(ACT_CASES))
def test_act_ex_against_the_float64_oracle(name):
    from embodied_clip_amd.policy import PolicyHandle
    case = ACT_CASES[name]
    cfg = aref.cases.cfg_of(case)
    handle = PolicyHandle(**cfg)
    sd = aref.state_dict(case)
    flat = handle.flatten(sd, DEV)
    A = cfg["num_actions"]
    draws = [aref.make_inputs(case, name, d) for d in range(2 if case["mode"] == "reuse" else 1)]
    runs = []
    for fill in (0xFF, 0x00):
        ws = torch.full((handle.workspace_bytes(1, case["N"], False),), fill, dtype=torch.uint8, device=DEV)
        runs.append([_act_ex(handle, flat, inp, case, ws, d > 0, seed=5, step=7 + d, first_actor=100) for d, inp in enumerate(draws)])
    for d, inp in enumerate(draws):
        hv, hf, actions, logp, values = runs[0][d]
        figs = aref.figures(aref.split_hv(hv, hf, A), aref.oracle(case, sd, inp))
        for k in aref.OUTPUTS:
            print("%s call %d %s: rel-L2 %.3e per-row %.3e" % (name, d, k, *figs[k]))
        for k in aref.OUTPUTS:
            assert figs[k][0] < ACT_REL_BOUND and figs[k][1] < ACT_PER_ROW_BOUND, (name, d, k, figs[k])
        a2, lp2, v2 = _shared(hv, A, "sample", 5, 7 + d, 100)
        assert torch.equal(actions, a2) and _same_bits(logp, lp2) and _same_bits(values, v2)
        for x, y in zip(runs[0][d], runs[1][d]):
            assert torch.equal(x, y), "two runs in fresh workspaces differ"
    # greedy, and forcing, through the same entry point
    ws = torch.zeros(handle.workspace_bytes(1, case["N"], False), dtype=torch.uint8, device=DEV)
    hv, _, actions, logp, values = _act_ex(handle, flat, draws[0], case, ws, False, deterministic=True)
    a2, lp2, v2 = _shared(hv, A, "greedy", 0, 0, 0)
    assert torch.equal(actions, a2) and _same_bits(logp, lp2) and _same_bits(values, v2)
    N = case["N"]
    expert, mask = (torch.arange(N) % A).to(DEV), (torch.arange(N) % 3 != 0).float().to(DEV)
    hv, _, actions, logp, values = _act_ex(handle, flat, draws[0], case, ws, True, seed=5, step=7, first_actor=100, expert_actions=expert,
                                           expert_mask=mask, force_p=0.5)
    a2, lp2, v2 = _shared(hv, A, "sample", 5, 7, 100, expert, mask, 0.5)
    assert torch.equal(actions, a2) and _same_bits(logp, lp2) and _same_bits(values, v2)


def test_act_ex_on_a_narrow_handle_is_act():
    from embodied_clip_amd.imitation import teacher_force
    from embodied_clip_amd.policy import PolicyHandle
    case = dict(cfg=dict(num_actions=6, **C128), T=1, N=33, bf16=1, mode="infer")
    handle = PolicyHandle(**aref.cases.cfg_of(case))
    flat = handle.flatten(aref.state_dict(case), DEV)
    inp = aref.make_inputs(case, "narrow_a6")
    N, A = 33, 6
    ws = lambda: torch.zeros(handle.workspace_bytes(1, N, False), dtype=torch.uint8, device=DEV)
    expert, mask = (torch.arange(N) % A).to(DEV), (torch.arange(N) % 3 != 0).float().to(DEV)
    for kw in (dict(), dict(deterministic=True), dict(expert_actions=expert, expert_mask=mask, force_p=0.5)):
        got = _act_ex(handle, flat, inp, case, ws(), False, seed=5, step=7, first_actor=100, **kw)
        hv, hf = torch.empty((N, A + 1), device=DEV), torch.empty((N, handle.H), device=DEV)
        actions, logp, values = torch.empty(N, dtype=torch.int64, device=DEV), torch.empty(N, device=DEV), torch.empty(N, device=DEV)
        handle.act(flat, inp["feat"].to(DEV), inp["goal"].reshape(-1).to(DEV), inp["h0"].to(DEV), inp["masks"].reshape(-1).to(DEV), N, ws(),
                   hv, hf, actions, logp, values, 5, 7, 100, deterministic=bool(kw.get("deterministic")))
        if "force_p" in kw:
            teacher_force(hv, expert, mask, 0.5, actions, logp, A, 5, 7, 100)
            assert not torch.equal(actions, _shared(hv, A, "sample", 5, 7, 100)[0])
        torch.cuda.synchronize()
        for x, y in zip(got, (hv, hf, actions, logp, values)):
            assert torch.equal(x, y), kw


# ---- 5. the wide PPO loss ---------------------------------------------------------------------------------------------------------
def _wide_loss(inp, rows=None, B_scale=None, scratch=None):
    """ec_ppo_loss_wide on `rows` (a slice; default all) -> (dhv, sums4).  B_scale: grad_scale is set so that grad_scale / B of
    this call equals the whole batch's"""
    from embodied_clip_amd import ppo
    L, lib = _lib()
    rows = slice(None) if rows is None else rows
    t = {k: inp[k][rows].to(DEV).contiguous() for k in ("hv", "actions", "old_logp", "old_v", "ret", "nadv")}
    B, A = t["hv"].shape[0], t["hv"].shape[1] - 1
    gs = inp["grad_scale"] if B_scale is None else inp["grad_scale"] * B / B_scale
    dhv = torch.full_like(t["hv"], float("nan"))
    sums = torch.full((4,), float("nan"), dtype=torch.float64, device=DEV)
    scratch = ppo.ppo_wide_scratch(DEV) if scratch is None else scratch
    L.check(lib.ec_ppo_loss_wide(t["hv"].data_ptr(), t["actions"].data_ptr(), t["old_logp"].data_ptr(), t["old_v"].data_ptr(),
                                 t["ret"].data_ptr(), t["nadv"].data_ptr(), dhv.data_ptr(), sums.data_ptr(), scratch.data_ptr(), B, A,
                                 inp["clip"], inp["vclip"], inp["vcoef"], inp["ecoef"], gs, L.stream_ptr()), "ec_ppo_loss_wide")
    torch.cuda.synchronize()
    return dhv, sums


@functools.lru_cache(maxsize=None)
def _ppo_ref(name):
    inp = ref.ppo_inputs(name)
    dhv, sums, terms = ref.ppo_loss(inp)
    return inp, dhv, terms, ~ref.ppo_branch_rows(inp)


@pytest.mark.parametrize("name", list(ref.PPO_CASES))
def test_wide_ppo_loss_against_float64(name):
    from embodied_clip_amd import ppo
    inp, want, terms, keep = _ppo_ref(name)
    assert 1.0 - keep.float().mean().item() <= 0.02, "more than 2 % of the rows sit at a branch point"
    scratch = ppo.ppo_wide_scratch(DEV)
    dhv, sums = _wide_loss(inp, scratch=scratch)
    dhv2, sums2 = _wide_loss(inp, scratch=scratch)                          # (the ticket counter is left at zero)
    got = dhv.cpu()
    rel, row, se = ref.rel_l2(got[keep], want[keep]), ref.per_row(got[keep], want[keep]), ref.sums_err(sums.cpu(), terms)
    print("ppo %s: dhv rel-L2 %.3e per-row %.3e sums %.3e (excluded %d of %d)" % (name, rel, row, se, int((~keep).sum()), keep.numel()))
    assert torch.isfinite(got).all()
    assert rel < MARGIN * FP32_PPO_DHV[0], rel
    assert row < MARGIN * FP32_PPO_DHV[1], row
    assert se < MARGIN * FP32_PPO_SUMS, se
    assert torch.equal(dhv, dhv2) and torch.equal(sums, sums2), "two runs differ"


@pytest.mark.parametrize("name", ["a6_b257", "a16_b257"])
def test_wide_entry_agrees_with_the_narrow_one(name):
    from embodied_clip_amd import _lib as L
    inp, want, terms, keep = _ppo_ref(name)
    t = {k: inp[k].to(DEV).contiguous() for k in ("hv", "actions", "old_logp", "old_v", "ret", "nadv")}
    B, A = t["hv"].shape[0], t["hv"].shape[1] - 1
    dhv_n, sums_n = torch.empty_like(t["hv"]), torch.empty(4, dtype=torch.float64, device=DEV)
    L.check(L.load().ec_ppo_loss_ex(t["hv"].data_ptr(), t["actions"].data_ptr(), t["old_logp"].data_ptr(), t["old_v"].data_ptr(),
                                    t["ret"].data_ptr(), t["nadv"].data_ptr(), dhv_n.data_ptr(), sums_n.data_ptr(), B, A, inp["clip"],
                                    inp["vclip"], inp["vcoef"], inp["ecoef"], inp["grad_scale"], L.stream_ptr()))
    dhv_w, sums_w = _wide_loss(inp)
    # both sit within the bound of the float64 reference, so within twice the bound of one another
    rel, row = ref.rel_l2(dhv_w.cpu()[keep], dhv_n.cpu()[keep]), ref.per_row(dhv_w.cpu()[keep], dhv_n.cpu()[keep])
    print("wide vs narrow %s: rel-L2 %.3e per-row %.3e" % (name, rel, row))
    assert rel < 2 * MARGIN * FP32_PPO_DHV[0] and row < 2 * MARGIN * FP32_PPO_DHV[1], (rel, row)
    assert ref.sums_err(sums_w.cpu(), terms) < MARGIN * FP32_PPO_SUMS and ref.sums_err(sums_n.cpu(), terms) < MARGIN * FP32_PPO_SUMS


def test_wide_ppo_rows_do_not_depend_on_the_split():
    inp, _, _, _ = _ppo_ref("a84_b2051")
    # B = 2048 and grad_scale = 1 or 3/8: a part of n rows gets grad_scale * n / 2048, an integer (n or 3 n) over a power of
    # two, so exact in fp32, and the kernel's fp32 quotient by n is grad_scale / 2048 exactly, for every n.  The cuts: multiples
    # of the 16-row chunk and of the 4-wave stride, and two that are neither (rows change wave, chunk and workgroup)
    B = 2048
    assert inp["grad_scale"] in (1.0, 0.375)
    whole, _ = _wide_loss(inp, rows=slice(0, B))
    for cut in (1024, 512, 1000, 37):
        a, _ = _wide_loss(inp, rows=slice(0, cut), B_scale=B)
        b, _ = _wide_loss(inp, rows=slice(cut, B), B_scale=B)
        assert torch.equal(a, whole[:cut]), cut
        assert torch.equal(b, whole[cut:]), cut


def test_wide_ppo_bad_action_id_poisons_the_loss():
    inp = dict(ref.ppo_inputs("a84_b257"))
    for bad in (84, -1, 1 << 32):                                           # (1 << 32 truncates to 0: checked as 64 bits)
        inp["actions"] = inp["actions"].clone()
        inp["actions"][100] = bad
        dhv, sums = _wide_loss(inp)
        assert torch.isnan(sums[0]) and torch.isfinite(sums[1:]).all()


def test_ppo_loss_raw_and_the_plugin_loss_take_the_wide_entry():
    from embodied_clip_amd import ppo
    from embodied_clip_amd.allenact_compat import ActorCriticOutput, CategoricalDistr
    inp, want, terms, keep = _ppo_ref("a84_b257")
    t = {k: inp[k].to(DEV).contiguous() for k in ("hv", "actions", "old_logp", "old_v", "ret", "nadv")}
    dhv, sums = ppo.ppo_loss_raw(t["hv"], t["actions"], t["old_logp"], t["old_v"], t["ret"], t["nadv"], 84, inp["clip"], inp["vcoef"],
                                 inp["ecoef"])
    torch.cuda.synchronize()
    d0, s0 = _wide_loss(inp)
    assert torch.equal(dhv, d0) and torch.equal(sums, s0)
    T, N, A = 1, 257, 84
    logits = t["hv"][:, :A].reshape(T, N, A).clone().requires_grad_(True)
    values = t["hv"][:, A:].reshape(T, N, 1).clone().requires_grad_(True)
    batch = dict(actions=t["actions"].reshape(T, N), old_action_log_probs=t["old_logp"].reshape(T, N, 1), values=t["old_v"].reshape(T, N, 1),
                 returns=t["ret"].reshape(T, N, 1), norm_adv_targ=t["nadv"].reshape(T, N, 1))
    total, info = ppo.PPO().loss(0, batch, ActorCriticOutput(CategoricalDistr(logits=logits), values, {}))
    total.backward()
    g = torch.cat([logits.grad.reshape(N, A), values.grad.reshape(N, 1)], dim=1).cpu()
    assert ref.rel_l2(g[keep], want[keep]) < MARGIN * FP32_PPO_DHV[0]
    tot64 = (terms[:, 0].mean() + 0.5 * terms[:, 1].mean() + 0.01 * terms[:, 2].mean()).item()
    assert abs(float(total.detach()) - tot64) < 1e-5 * max(1.0, abs(tot64))

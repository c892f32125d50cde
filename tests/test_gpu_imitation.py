"""GPU: the imitation loss kernel, its normaliser and the teacher-forcing draw (csrc/imitation.hip) against the float64
reference and the restated draw of tests/_imitation_ref.py.

Tolerances are the PPO loss tests' (test_ppo_loss_*): each sum within 1e-5 * max(1, |ref|), rel-L2 of dhv below 1e-5 (torch
fp32 against float64 measures ~6e-8 on these inputs on the CPU); the agreement count is exact (row maxima are unique by
construction).  B = 1025 and 2500 span 5 and 10 blocks of 256 rows with ragged tails of 1 and 196 rows on the thread-per-row path, 65 and 157
blocks of 16 rows with tails of 1 and 4 rows on the wave-per-row path; A = 16 | 17 is the
switch from one thread to one wave per row, 84 and 17 leave tail lanes, 256 fills four logits per lane."""
import math

import numpy as np
import pytest
import torch

import _imitation_ref as ref
from embodied_clip_amd import _lib
from embodied_clip_amd import imitation as il

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _run(hv, e, m, A, **kw):
    dhv, sums = il.imitation_loss_raw(hv.to(DEV), e.to(DEV), m.to(DEV), A, **kw)
    torch.cuda.synchronize()
    return dhv.cpu(), sums.cpu()


def _rel(a, b):
    return ((a.double() - b).norm() / b.norm().clamp_min(1e-300)).item()


@pytest.mark.parametrize("A", [1, 6, 16, 17, 84, 256])
@pytest.mark.parametrize("B", [1, 5, 1025, 2500])
def test_loss_kernel_matches_reference(B, A):
    for kind in ("ones", "zeros", "mixed"):
        for scale in (1.0, 30.0):
            hv, e, m = ref.make_case(B, A, scale=scale, mask_kind=kind)
            if kind != "ones":
                e = torch.where(m != 0, e, torch.full_like(e, -1))      # a row without an expert action never reads its id
            _, rdhv, rs = ref.imitation_ref(hv, e, m, weight=0.7, grad_scale=0.5)
            dhv, s = _run(hv, e, m, A, weight=0.7, grad_scale=0.5)
            r = _rel(dhv, rdhv) if float(rdhv.norm()) > 0 else float(dhv.abs().max())
            print(f"B={B} A={A} mask={kind} scale={scale}: sums {s.tolist()} ref {rs.tolist()} dhv rel-L2 {r:.3e}")
            assert torch.isfinite(dhv).all() and torch.isfinite(s).all()
            for i in (0, 1):
                assert abs(float(s[i] - rs[i])) <= 1e-5 * max(1.0, abs(float(rs[i]))), (kind, scale, i, s, rs)
            assert float(s[2]) == float(rs[2]), (kind, scale, s, rs)
            if float(rdhv.norm()) > 0:
                assert r < 1e-5, (kind, scale, r)
            else:
                assert torch.all(dhv == 0)
            assert torch.all(dhv[:, A] == 0) and torch.all(dhv[m == 0] == 0)


@pytest.mark.parametrize("A", [6, 84])
def test_denominator_given_or_own_split_calls_and_two_runs(A):
    B = 2500
    hv, e, m = ref.make_case(B, A, seed=1)
    d_own, s_own = _run(hv, e, m, A, grad_scale=0.25)
    md = m.reshape(1, B).contiguous().to(DEV)
    D = il.expert_count(md, 0, B)
    assert float(D.cpu()) == float(m.sum())
    # the normaliser given == the call's own: the same bits
    d_giv, s_giv = _run(hv, e, m, A, grad_scale=0.25, denom=D)
    assert torch.equal(d_giv, d_own) and torch.equal(s_giv, s_own)
    # rows split 700 / 1800 over two calls that share the normaliser: every row's gradient is that of the one call
    d_a, s_a = _run(hv[:700], e[:700], m[:700], A, grad_scale=0.25, denom=D)
    d_b, s_b = _run(hv[700:], e[700:], m[700:], A, grad_scale=0.25, denom=D)
    assert torch.equal(torch.cat([d_a, d_b]), d_own)
    assert float(s_a[1] + s_b[1]) == float(s_own[1]) and float(s_a[2] + s_b[2]) == float(s_own[2])
    assert abs(float(s_a[0] + s_b[0] - s_own[0])) <= 1e-12 * abs(float(s_own[0]))
    # two runs in fresh buffers
    d_2, s_2 = _run(hv.clone(), e.clone(), m.clone(), A, grad_scale=0.25)
    assert torch.equal(d_2, d_own) and torch.equal(s_2, s_own)
    # the float64 reference with a shared denominator that is NOT the call's own mask sum
    _, rdhv, _ = ref.imitation_ref(hv[:700], e[:700], m[:700], grad_scale=0.25, denom=float(m.sum()))
    assert _rel(d_a, rdhv) < 1e-5


@pytest.mark.parametrize("A", [6, 84])
def test_accumulate_adds_the_term(A):
    B = 1025
    hv, e, m = ref.make_case(B, A, seed=2)
    term, s0 = _run(hv, e, m, A, weight=2.0)
    dhv0 = torch.randn(B, A + 1, generator=torch.Generator().manual_seed(5)) * 1e-3
    buf = dhv0.clone().to(DEV)
    got, s1 = _run(hv, e, m, A, weight=2.0, dhv=buf, accumulate=True)
    assert torch.equal(s0, s1)
    want = dhv0.double() + term.double()
    bound = 2.0 ** -23 * (dhv0.double().abs() + term.double().abs())
    assert torch.all((got.double() - want).abs() <= bound)
    assert torch.equal(got[:, A], dhv0[:, A])                       # the value column ...
    assert torch.equal(got[m == 0], dhv0[m == 0]) and int((m == 0).sum()) > 0      # ... and masked-out rows: left alone
    assert not torch.equal(got[m != 0][:, :A], dhv0[m != 0][:, :A])


@pytest.mark.parametrize("A", [6, 84])
def test_out_of_range_expert_id(A):
    hv, e, m = ref.make_case(40, A, mask_kind="ones", seed=3)
    base_d, base_s = _run(hv, e, m, A)
    for bad in (-1, A, 10 ** 12):
        e2, m2 = e.clone(), m.clone()
        e2[17], m2[17] = bad, 0.0
        e_ok = e.clone()
        e_ok[17] = 0
        d_ok, s_ok = _run(hv, e_ok, m2, A)
        d, s = _run(hv, e2, m2, A)
        assert torch.equal(d, d_ok) and torch.equal(s, s_ok)      # mask 0: the id has no effect
        d, s = _run(hv, e2, m, A)                                # mask 1: the loss is poisoned
        assert math.isnan(float(s[0])) and float(s[1]) == 40.0
    assert math.isfinite(float(base_s[0]))


def test_expert_count_matches_fsum():
    T, N = 7, 9
    g = torch.Generator().manual_seed(4)
    mask = torch.randint(0, 5, (T + 1, N), generator=g).float() / 4.0      # (a [T+1, N] buffer; T rows are summed)
    md = mask.to(DEV)
    for n0, n1 in ((0, 9), (2, 5), (8, 9)):
        out = torch.full((1,), -1.0, dtype=torch.float64, device=DEV)
        _lib.check(_lib.load().ec_expert_count(md.data_ptr(), T, N, n0, n1, out.data_ptr(), _lib.stream_ptr()), "count")
        torch.cuda.synchronize()
        assert float(out.cpu()) == math.fsum(mask[:T, n0:n1].reshape(-1).tolist()), (n0, n1)


# ---- teacher forcing --------------------------------------------------------------------------------------------------
def _tf_inputs(N, A, seed=6):
    g = torch.Generator().manual_seed(seed)
    hv = torch.randn(N, A + 1, generator=g)
    e = torch.randint(0, A, (N,), generator=g)
    m = (torch.rand(N, generator=g) > 0.3).float()
    e = torch.where(m != 0, e, torch.full_like(e, -1))
    return hv, e, m


def _force(hv, e, m, p, step, first=0, seed=ref.TF_SEED):
    N, A = hv.shape[0], hv.shape[1] - 1
    acts = torch.full((N,), -7, dtype=torch.int64, device=DEV)
    logp = torch.full((N,), 9.0, device=DEV)
    il.teacher_force(hv.contiguous().to(DEV), e.contiguous().to(DEV), m.contiguous().to(DEV), p, acts, logp, A, seed, step, first)
    torch.cuda.synchronize()
    return acts.cpu(), logp.cpu()


def test_teacher_forcing_off_and_always():
    hv, e, m = _tf_inputs(300, 6)
    a, lp = _force(hv, e, m, 0.0, 0)
    assert torch.all(a == -7) and torch.all(lp == 9.0)
    a, lp = _force(hv, e, m, 1.0, 0)
    on = m != 0
    assert torch.equal(a[on], e[on]) and torch.all(a[~on] == -7) and torch.all(lp[~on] == 9.0) and int((~on).sum()) > 0
    want = torch.log_softmax(hv[:, :6].double(), -1)[on].gather(1, e[on][:, None])[:, 0]
    assert torch.allclose(lp[on].double(), want, atol=1e-6, rtol=0)


def test_teacher_forcing_draw_matches_the_restatement_and_is_its_own_stream():
    N, A, S = ref.TF_N, ref.TF_A, ref.TF_STEPS
    hv, e, _ = _tf_inputs(N, A)
    e = e.clamp(min=0)
    ones = torch.ones(N)
    lsm = torch.log_softmax(hv[:, :A].double(), -1)
    forced_all = []
    for step in range(S):
        a, lp = _force(hv, e, ones, 0.5, step)
        want = torch.from_numpy(ref.teacher_force_decisions(ref.TF_SEED, step, 0, ones.numpy(), 0.5))
        got = a != -7
        assert torch.equal(got, want), step                        # every row's decision is the restated draw's
        assert torch.equal(a[got], e[got]) and torch.all(lp[~got] == 9.0)
        assert torch.allclose(lp[got].double(), lsm[got].gather(1, e[got][:, None])[:, 0], atol=1e-6, rtol=0)
        forced_all.append(got)
    frac = torch.stack(forced_all).float().mean().item()
    print(f"forced fraction at p = 0.5 over {S * N} draws: {frac:.5f}")
    assert abs(frac - 0.5) < 0.011                               # 4 sigma; tests/test_imitation_ref.py shows the draw meets it
    # slice invariance: rows [1000, 1300) alone with first_actor = 1000, on a mixed mask
    hv2, e2, m2 = _tf_inputs(N, A, seed=8)
    a, lp = _force(hv2, e2, m2, 0.5, 7)
    sa, slp = _force(hv2[1000:1300], e2[1000:1300], m2[1000:1300], 0.5, 7, first=1000)
    assert torch.equal(sa, a[1000:1300]) and torch.equal(slp, lp[1000:1300])
    assert torch.equal(a != -7, torch.from_numpy(ref.teacher_force_decisions(ref.TF_SEED, 7, 0, m2.numpy(), 0.5)))
    # not the sampler's draw: were the forcing uniform ec_sample_row's, "forced" and "sampled == expert" would be tied together
    lib = _lib.load()
    hvd = hv.contiguous().to(DEV)
    sampled = torch.empty(N, dtype=torch.int64, device=DEV)
    slogp = torch.empty(N, device=DEV)
    _lib.check(lib.ec_sample_actions(hvd.data_ptr(), sampled.data_ptr(), slogp.data_ptr(), None, N, A, ref.TF_SEED, 0, 0,
                                     _lib.stream_ptr()), "sample")
    torch.cuda.synchronize()
    assert int((forced_all[0] != (sampled.cpu() == e)).sum()) >= 1
    u_tf = ref.teacher_force_uniform(ref.TF_SEED, 0, np.arange(N))
    assert not np.array_equal(u_tf, ref.sampler_uniform(ref.TF_SEED, 0, np.arange(N)))

"""The bounds of tests/_vit_stage_ref.py bite, checked without a GPU on the very inputs the GPU tests use: (a) an fp32 / bf16
emulation of each kernel's arithmetic stays under the stage's bound, (b) each named wrong version exceeds it at least 4 x
somewhere.  Where a wrong version can only show on one input family (eps at unit variance is invisible, a leak forward needs a
query that asks for the forbidden key) the family that has to catch it is named in the reference module."""
import pytest
import torch

import _vit_stage_ref as R

MUST_EXCEED = 4.0


def _mha(L, causal, family, B=3, D=128, heads=2):
    qkv = R.attention_inputs(family, B, L, D, heads)
    ref, bound, dom = R.attention_ref(qkv, B, L, D, heads, causal)
    return qkv, ref, bound, dom


@pytest.mark.parametrize("L,causal,family", R.MHA_CASES, ids=lambda v: str(v))
def test_attention_bound_bites(L, causal, family):
    B, D, heads = 3, 128, 2
    qkv, ref, bound, dom = _mha(L, causal, family)
    if family != "next":
        assert float(dom.min()) >= 0.5, float(dom.min())
    assert R.worst_ratio(R.attention_emulate(qkv, B, L, D, heads, causal), ref, bound) <= 1.0
    if L < 2:
        return
    wrong = ["kv_swapped", "scale_rsqrt_D"]
    wrong += {"diag": ["causal_nk_qi"], "next": ["causal_nk_qi_plus_2"], "reverse": []}[family]
    for kind in wrong:
        r = R.worst_ratio(R.attention_wrong(qkv, B, L, D, heads, causal, kind), ref, bound)
        assert r >= MUST_EXCEED, (kind, r)
    if family != "next":      # every key is some query's dominant key: dropping ANY single key shows
        r = R.attention_drop_key_ratios(qkv, B, L, D, heads, causal, ref, bound)
        assert float(r.min()) >= MUST_EXCEED, float(r.min())


def test_attention_wide_case_bound_bites():
    c = R.MHA_WIDE_CASE
    args = (c["B"], c["L"], c["D"], c["heads"])
    qkv = R.attention_inputs(c["family"], *args)
    ref, bound, dom = R.attention_ref(qkv, *args, c["causal"])
    assert float(dom.min()) >= 0.5
    assert R.worst_ratio(R.attention_emulate(qkv, *args, c["causal"]), ref, bound) <= 1.0
    assert float(R.attention_drop_key_ratios(qkv, *args, c["causal"], ref, bound).min()) >= MUST_EXCEED
    for kind in ("kv_swapped", "scale_rsqrt_D"):
        assert R.worst_ratio(R.attention_wrong(qkv, *args, c["causal"], kind), ref, bound) >= MUST_EXCEED, kind


@pytest.mark.parametrize("D", R.LN_DIMS)
@pytest.mark.parametrize("rows", R.LN_ROWS)
def test_layernorm_bound_bites(rows, D):
    for family in R.LN_FAMILIES:
        x, gamma, beta = R.layernorm_inputs(family, rows, D)
        ref, bound = R.layernorm_ref(x.to(R.F64), gamma, beta)
        assert R.worst_ratio(R.layernorm_emulate(x.float(), gamma, beta), ref, bound) <= 1.0, family
        for kind in R.LN_WRONG:
            if R.LN_CAUGHT_BY[kind] != family:
                continue
            r = R.worst_ratio(R.layernorm_wrong(x.to(R.F64), gamma, beta, kind, vector_path=D % 256 == 0), ref, bound)
            assert r >= MUST_EXCEED, (family, kind, r)


@pytest.mark.parametrize("B,L,D", R.ASSEMBLE_SHAPES)
def test_assemble_and_record_bounds_bite(B, L, D):
    pemb, cls, pos, gamma, beta = R.assemble_inputs(B, L, D)
    v64, v32, v_err = R.assemble_rows(pemb, cls, pos, B, L, D)
    ref, bound = R.layernorm_ref(v64, gamma, beta, v_err=v_err)
    y = R.layernorm_emulate(v32, gamma, beta)
    assert R.worst_ratio(y, ref, bound) <= 1.0
    for kind in ("lane_missing", "gamma_beta_shifted"):      # (rows with a common offset: a lost lane moves the mean)
        assert R.worst_ratio(R.layernorm_wrong(v64, gamma, beta, kind), ref, bound) >= MUST_EXCEED, kind
    # the record describes the ROUNDED row; a record of the unrounded row, or M2 about zero instead of the mean, is outside
    (s, m2, n), (bs, bm) = R.record_ref(y.to(R.F64), R.ln_depth(D))
    es, em = R.record_emulate(y)
    assert R.worst_ratio(es, s, bs) <= 1.0 and R.worst_ratio(em, m2, bm) <= 1.0
    us, um = R.record_emulate(ref)
    assert R.worst_ratio(us, s, bs) >= MUST_EXCEED and R.worst_ratio(um, m2, bm) >= MUST_EXCEED
    assert R.worst_ratio((y.double() ** 2).sum(-1), m2, bm) >= MUST_EXCEED


@pytest.mark.parametrize("N,K", R.FOLD_SHAPES)
def test_fold_bounds_bite(N, K):
    W, gamma, beta, b = R.fold_inputs(N, K)
    Wg, (s, bs), (c, bc) = R.fold_ref(W, gamma, beta, b)
    eWg, es, ec = R.fold_emulate(W, gamma, beta, b)
    assert torch.equal(eWg, Wg)
    assert R.worst_ratio(es, s, bs) <= 1.0 and R.worst_ratio(ec, c, bc) <= 1.0
    unrounded = (W.double() * gamma.double()[None, :]).sum(-1)                     # s over the UNROUNDED products
    assert R.worst_ratio(unrounded, s, bs) >= MUST_EXCEED
    assert R.worst_ratio((beta.double()[None, :] * Wg.double()).sum(-1) + b.double(), c, bc) >= MUST_EXCEED   # c from Wg
    assert R.worst_ratio(c - b.double(), c, bc) >= MUST_EXCEED                     # bias left out


@pytest.mark.parametrize("setting", list(R.GEMM_SETTINGS))
def test_gemm_ln_bound_bites(setting):
    width = 256 if setting == "wide" else 128
    for case in R.gemm_cases(setting):
        M, D, N, act, stream = case["M"], case["D"], case["N"], case["act"], case["stream"]
        w = width if D % width == 0 else 128
        x = R.residual_stream(stream, M, D)
        _, (Wg, s, c) = R.consumer_weights(N, D)
        ref, bound = R.gemm_ln_ref(x, Wg, s, c, act)
        assert R.worst_ratio(R.gemm_ln_emulate(x, Wg, s, c, act, w), ref, bound) <= 1.0, case
        if stream != "mean_dominated":
            continue
        assert R.worst_ratio(R.gemm_ln_emulate(x, Wg, s, c, act, w, "no_mean_s"), ref, bound) >= MUST_EXCEED, case
        np_ = D // w
        if np_ > 1:
            for q in range(np_):
                r = R.worst_ratio(R.gemm_ln_emulate(x, Wg, s, c, act, w, ("ignore", q)), ref, bound)
                assert r >= MUST_EXCEED, (case, q, r)
            r = R.worst_ratio(R.gemm_ln_emulate(x, Wg, s, c, act, w, "equal_weight"), ref, bound)
            assert r >= MUST_EXCEED, (case, r)

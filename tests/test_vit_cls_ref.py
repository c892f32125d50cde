"""CPU: the bounds of tests/_vit_cls_ref.py bite.  For every stage of the CLS-only last block the emulation of the kernel's
arithmetic stays under the bound on the GPU test's own inputs, and each named wrong version exceeds it at least 4 x somewhere
(the project's ratio) -- so a kernel that passes tests/test_gpu_vit_cls.py has none of these mistakes."""
import pytest
import torch

import _vit_cls_ref as R

BITE = 4.0


def test_gemm_cases_reach_every_variant_with_every_shape():
    cases = R.gemm_cases()
    assert len(cases) == len(R.GEMM_M) * len(R.GEMM_NK) * len(R.GEMM_PITCH)
    key = lambda c: (c["act"], c["res"], c["store"], c["bias"])      # noqa: E731
    assert {key(c) for c in cases} == {key(v) for v in R.GEMM_VARIANTS}
    for v in R.GEMM_VARIANTS:
        mine = [c for c in cases if key(c) == key(v)]
        assert {c["lda"] // c["K"] for c in mine} == set(R.GEMM_PITCH), v
        assert len({(c["N"], c["K"]) for c in mine}) == len(R.GEMM_NK), v
    assert {c["store"] for c in cases} == {0, 1, 2} and {c["act"] for c in cases} == {0, 2}


@pytest.mark.parametrize("c", R.gemm_cases(), ids=R.gemm_id)
def test_gemm_emulation_stays_under_the_bound(c):
    op = R.gemm_inputs(c)
    ref, bound = R.gemm_ref(c, op)
    assert R.worst_ratio(R.gemm_emulate(c, op), ref, bound) <= 1.0


@pytest.mark.parametrize("kind", R.GEMM_WRONG)
def test_gemm_wrong_versions_exceed_the_bound(kind):
    hit = 0
    for c in R.gemm_cases():
        if not R.gemm_wrong_applies(c, kind):
            continue
        op = R.gemm_inputs(c)
        ref, bound = R.gemm_ref(c, op)
        r = R.worst_ratio(R.gemm_emulate(c, op, wrong=kind), ref, bound)
        assert r >= BITE, (kind, R.gemm_id(c), r)
        hit += 1
    assert hit >= 3, (kind, hit)


def test_gemm_fp32_store_is_held_to_fp32_roundoff():
    """store 2 is bounded with U: the bf16 rounding of the same value exceeds that bound (the two stores are not interchangeable)"""
    c = next(c for c in R.gemm_cases() if c["store"] == R.STORE_F32 and c["act"] == R.ACT_NONE and c["K"] == 64)
    op = R.gemm_inputs(c)
    ref, bound = R.gemm_ref(c, op)
    assert R.worst_ratio(R.bf16(R.gemm_emulate(c, op)), ref, bound) >= BITE


@pytest.mark.parametrize("B,L,heads", R.ATTN_CASES)
def test_attention_bound_bites(B, L, heads):
    qkv, q_rows, kv = R.attn_inputs(B, L, heads)
    ref, bound, dom = R.attn_ref(qkv, B, L, heads)
    assert float(dom.min()) >= 0.5                              # every row has a dominant key: L - 1 - i, so every key dominates once
    assert R.worst_ratio(R.attn_emulate(qkv, B, L, heads), ref[0], bound[0]) <= 1.0
    for kind in R.ATTN_WRONG:
        if R.attn_wrong_applies(B, L, kind):
            r = R.worst_ratio(R.attn_emulate(qkv, B, L, heads, wrong=kind), ref[0], bound[0])
            assert r >= BITE, (kind, r)
    # the inputs the kernel gets are the reference's: q_rows[i] is row i of every frame, kv the k | v columns
    D = heads * 64
    assert torch.equal(q_rows[0], qkv.reshape(B, L, 3 * D)[:, 0, :D]) and torch.equal(kv, qkv[:, D:])


@pytest.mark.parametrize("D", R.LN_DIMS)
def test_layernorm_bound_bites(D):
    for pm in R.LN_PITCH:
        for rows in R.LN_ROWS:
            for family in R.LN_FAMILIES:
                buf, gamma, beta = R.ln_inputs(family, rows, D, pm)
                x = buf[:, :D]
                ref, bound = R.layernorm_ref(x.to(R.F64), gamma, beta)
                assert R.worst_ratio(R.layernorm_emulate(x.to(torch.float32), gamma, beta), ref, bound) <= 1.0, (pm, rows, family)
                if pm > 1 and rows > 1 and family == "plain":
                    assert R.worst_ratio(R.ln_wrong_pitch(buf, rows, D, gamma, beta), ref, bound) >= BITE, (pm, rows)

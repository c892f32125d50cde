"""CPU: the shared comparison rule (tests/_bounds.py) and the guarded output buffer (tests/_guard.py) that every kernel-instance
check relies on -- a helper that let a NaN or a written guard through would pass every kernel."""
import pytest
import torch

import _bounds as B
from _guard import GUARD, SENT16, SENT32, Guarded


def test_worst_ratio_rules():
    ref = torch.tensor([[1.0, 2.0, 0.0], [4.0, 5.0, 6.0]], dtype=torch.float64)
    bound = torch.tensor([[0.5, 0.5, 0.0], [0.5, 0.25, 0.5]], dtype=torch.float64)
    assert B.worst_ratio(ref.clone(), ref, bound) == (0.0, 0)                      # 0 / 0 (element [0, 2]) counts as 0
    got = ref.clone()
    got[1, 1] += 0.5
    got[0, 0] -= 0.5
    assert B.worst_ratio(got, ref, bound) == (2.0, 4)                              # the flat index of the worst element
    assert B.worst_ratio(got.float(), ref, bound.float()) == (2.0, 4)              # ... in float64 whatever comes in
    got[0, 2] = 1e-30
    assert B.worst_ratio(got, ref, bound) == (float("inf"), 2)                     # an error over a zero bound
    got = ref.clone()
    got[1, 0] = float("nan")
    assert B.worst_ratio(got, ref, bound) == (float("inf"), 3)                     # a NaN in got
    assert B.worst_ratio(got.to(torch.bfloat16), ref, bound)[0] == float("inf")


def test_bf16_rounds_ties_to_even_and_keeps_the_dtype():
    # 1 + 2^-8 lies halfway between the bf16 neighbours 1 (even significand) and 1 + 2^-7; 1 + 3 * 2^-8 between 1 + 2^-7 and
    # 1 + 2^-6 (even)
    t = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), 1.0 + 2.0 ** -8 + 2.0 ** -20])
    want = torch.tensor([1.0, 1.0 + 2.0 ** -6, -1.0, 1.0 + 2.0 ** -7])
    assert torch.equal(B.bf16(t), want) and B.bf16(t).dtype == torch.float32
    assert torch.equal(B.bf16(t.double()), want.double()) and B.bf16(t.double()).dtype == torch.float64
    assert B.UB == 2.0 ** -8 and B.U == 2.0 ** -24 and B.F64 == torch.float64 and B.F32 == torch.float32


def test_randn_is_the_seeded_cpu_generator():
    a = B.randn(7, 3, 5)
    assert a.dtype == torch.float32 and a.shape == (3, 5) and torch.equal(a, B.randn(7, 3, 5)) and not torch.equal(a, B.randn(8, 3, 5))
    assert torch.equal(a, torch.randn(3, 5, generator=torch.Generator().manual_seed(7), dtype=torch.float32))


def test_rel_l2():
    ref = torch.tensor([3.0, 4.0], dtype=torch.float64)
    assert B.rel_l2(torch.tensor([3.0, 4.5]), ref) == pytest.approx(0.1)


@pytest.mark.parametrize("f32", [False, True])
def test_guarded_reports_every_written_guard(f32):
    rows, n, ld, col0 = 5, 8, 24, 8
    sent = SENT32 if f32 else SENT16

    def fresh():
        g = Guarded("cpu", rows, n, ld, col0, f32=f32)
        assert g.buf.shape == (rows + 2 * GUARD, ld) and bool((g.buf == sent).all())
        assert g.ptr == g.buf.data_ptr() + (GUARD * ld + col0) * (4 if f32 else 2)
        return g

    g = fresh()
    g.buf[GUARD:GUARD + rows, col0:col0 + n] = 7                     # what a correct kernel writes: the body alone
    body, ok = g.read()
    assert ok and body.shape == (rows, n) and bool((body == 7).all())
    for r, c in ((GUARD - 1, col0), (0, 0), (GUARD + rows, col0 + n - 1), (rows + 2 * GUARD - 1, ld - 1),      # before, behind
                 (GUARD, col0 - 1), (GUARD + rows - 1, col0 + n), (GUARD + 2, 0), (GUARD + 2, ld - 1)):        # the side columns
        g = fresh()
        g.buf[r, c] ^= 1
        assert g.read()[1] is False, (r, c)


def test_guarded_prefill_and_row_multiples():
    c0 = torch.arange(12, dtype=torch.float32).view(6, 2)            # 3 parts of 2 rows: a plain multiple of rows
    g = Guarded("cpu", 3 * 2, 2, 5, f32=True, fill=c0)
    body, ok = g.read()
    assert ok and torch.equal(body.view(torch.float32), c0) and body.view(torch.float32).view(3, 2, 2)[2, 1, 1] == 11.0
    g = Guarded("cpu", 4, 3, fill=float("nan"))
    body, ok = g.read()
    assert ok and bool(torch.isnan(body.view(torch.bfloat16)).all()) and bool((body != SENT16).all())

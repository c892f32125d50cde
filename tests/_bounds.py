"""The number formats and the bound comparison shared by the float64 reference modules (tests/_*_ref.py).  CPU only."""
import torch

UB = 2.0 ** -8             # unit roundoff of bf16 (8 significant bits, round to nearest)
U = 2.0 ** -24             # ... and of fp32
F64 = torch.float64
F32 = torch.float32


def bf16(t):
    """Round to bf16 (nearest even), keep the dtype of ``t``."""
    return t.to(F32).to(torch.bfloat16).to(t.dtype)


def randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=F32)


def worst_ratio(got, ref, bound):
    """-> (max |got - ref| / bound, flat index of that element), in float64 (0 / 0 counts as 0; an error over a zero
    bound is infinite, and so counts a NaN)"""
    err = (got.to(F64) - ref.to(F64)).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound.to(F64))
    r = torch.nan_to_num(r, nan=float("inf"), posinf=float("inf"))      # (posinf: nan_to_num would make it the largest finite value)
    i = int(r.argmax())
    return float(r.reshape(-1)[i]), i


def rel_l2(got, ref):
    return float((got.to(F64) - ref).norm() / ref.norm())

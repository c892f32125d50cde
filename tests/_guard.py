"""Sentinel patterns and the guarded output buffer of the kernel-instance checks (tests/_*_check.py and the GPU tests that lay
their own guards out): a kernel that writes one element outside its output changes a sentinel, and the check reads them all."""
import torch

SENT16 = 0x7FC1            # a bf16 NaN pattern (as int16) no kernel here produces
SENT32 = 0x7FC12345        # ... and an fp32 one (as int32)
GUARD = 256                # guard rows on either side: one tile


class Guarded:
    """A [rows, n] output (bf16, or fp32 with f32=True) inside a sentinel-filled [rows + 2 GUARD, ld] buffer, from column col0 on.
    ``fill`` (a value, or a tensor that broadcasts to [rows, n]) is what the output holds before the kernel runs."""

    def __init__(self, dev, rows, n, ld=None, col0=0, f32=False, fill=None):
        self.rows, self.n, self.ld, self.col0, self.f32 = rows, n, ld or n, col0, f32
        assert col0 + n <= self.ld
        self.sent = SENT32 if f32 else SENT16
        bits = torch.int32 if f32 else torch.int16
        if fill is None:
            self.buf = torch.full((rows + 2 * GUARD, self.ld), self.sent, dtype=bits, device=dev)
        else:
            host = torch.full((rows + 2 * GUARD, self.ld), self.sent, dtype=bits)
            host.view(torch.float32 if f32 else torch.bfloat16)[GUARD:GUARD + rows, col0:col0 + n] = fill
            self.buf = host.to(dev)
        self.ptr = self.buf.data_ptr() + (GUARD * self.ld + col0) * self.buf.element_size()

    def read(self):
        """-> (the output's bit patterns, guards bitwise intact)"""
        o = self.buf.cpu()
        body = o[GUARD:GUARD + self.rows, self.col0:self.col0 + self.n].contiguous()
        mask = torch.ones_like(o, dtype=torch.bool)
        mask[GUARD:GUARD + self.rows, self.col0:self.col0 + self.n] = False
        return body, bool((o[mask] == self.sent).all())

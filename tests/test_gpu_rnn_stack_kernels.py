"""GPU: ``ec_rnn_stack_step_fwd`` alone (csrc/rnn_stack.hip: one act step of an upper recurrent layer -- input projection,
recurrent projection and cell in one launch) against the float64 closed form of tests/_rnn_stack_ref.py, for both cells.

Cases (N, H) -- tests/_rnn_stack_ref.py::KERNEL_CASES:
  (1, 32)    one lane row; whole-K staging
  (33, 64)   a second actor block holding one row
  (3, 96)    twelve unit blocks; H no power of two
  (5, 256)   one LDS-DMA chunk per half
  (37, 512)  two chunks per half; the reference width
each with the mask all one, all zero and mixed, and with x and the previous state dense and at a row pitch.

Bound per output: rel-L2 <= 10 x the worst fp32-vs-float64 rel-L2 of the SAME closed form over this case table
(``_rnn_stack_ref.kernel_bounds()``).  Figures of ``python tests/_rnn_stack_ref.py`` (fp32 torch against float64):
  GRU h 2.80e-7   LSTM h 2.93e-7   LSTM c 2.80e-7
Measured on an MI355X (worst over the table, the kernel against float64):
  GRU h 2.21e-7   LSTM h 2.28e-7   LSTM c 2.14e-7
"""
import os
import sys

import pytest
import torch

from embodied_clip_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _rnn_stack_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
GUARD = 3                       # rows past N in every output
CELLS = (ref.GRU, ref.LSTM)
CASES = [(cell, N, H, kind) for cell in CELLS for (N, H) in ref.KERNEL_CASES for kind in ref.KERNEL_MASKS]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _pitched(t, ld, dev, col0=0):
    """`t` [N, W] as rows of pitch ld starting at column col0 of a larger buffer -> (buffer, pointer of element [0, 0])"""
    buf = torch.full((t.shape[0], ld), -7.0, device=dev)
    buf[:, col0:col0 + t.shape[1]] = t.to(dev)
    return buf, buf.data_ptr() + 4 * col0


def _run(lib, cell, d, mask, dev, pitched, second=True):
    """one launch; h / c are written into one guarded state buffer -> (state out [N + GUARD, ld], dense h copy [N + GUARD, H])"""
    N, H = d["x"].shape
    lstm = cell == ref.LSTM
    SW = (2 if lstm else 1) * H
    ld_x, ld_p, ld_o = (3 * H + 8, 2 * SW + 4, 2 * SW) if pitched else (H, SW, SW)
    xb, xp = _pitched(d["x"], ld_x, dev, 4 if pitched else 0)
    sb, sp = _pitched(d["state"], ld_p, dev, 4 if pitched else 0)
    out = torch.full((N + GUARD, ld_o), SENTINEL, device=dev)
    h2 = torch.full((N + GUARD, H), SENTINEL, device=dev)
    w = {k: d[k].to(dev).contiguous() for k in ("wih", "whh", "bih", "bhh")}
    m = mask.to(dev)
    col0 = ld_o - SW                          # the written slice ends the row: a pitched output starts at column SW
    o_ptr = out.data_ptr() + 4 * col0
    _lib.check(lib.ec_rnn_stack_step_fwd(_lib.RNN_TYPES[cell], xp, ld_x, w["wih"].data_ptr(), w["whh"].data_ptr(), w["bih"].data_ptr(),
                                         w["bhh"].data_ptr(), sp, ld_p, m.data_ptr(), o_ptr, ld_o, o_ptr + 4 * H if lstm else 0, ld_o,
                                         h2.data_ptr() if second else 0, H, N, H, 0), "ec_rnn_stack_step_fwd")
    torch.cuda.synchronize()
    new = out[:, col0:]
    if col0:
        assert (out[:, :col0] == SENTINEL).all()           # nothing in front of the slice is written
    return new, h2


@pytest.mark.parametrize("pitched", [False, True])
@pytest.mark.parametrize("cell,N,H,kind", CASES)
def test_step_matches_float64(dev, cell, N, H, kind, pitched):
    lib = _lib.load()
    bounds = ref.kernel_bounds()
    d = ref.kernel_inputs(cell, N, H)
    mask = ref.kernel_mask(N, kind)
    want = ref.kernel_reference(cell, d, mask)
    new, h2 = _run(lib, cell, d, mask, dev, pitched)
    e = ref.rel_l2(new[:N, :H].cpu(), want[:, :H])
    print(f"{cell} ({N}, {H}) {kind} pitched={pitched}: h rel-L2 {e:.3e} (bound {bounds[(cell, 'h')]:.3e})")
    assert e <= bounds[(cell, "h")], e
    if cell == ref.LSTM:
        ec = ref.rel_l2(new[:N, H:].cpu(), want[:, H:])
        print(f"   c rel-L2 {ec:.3e} (bound {bounds[(cell, 'c')]:.3e})")
        assert ec <= bounds[(cell, "c")], ec
    assert torch.equal(h2[:N], new[:N, :H])                                    # the second copy of h: the same bits
    assert (new[N:] == SENTINEL).all() and (h2[N:] == SENTINEL).all()         # rows past N are never written
    # without the second copy: the same state, nothing else written; a second call: equal bits
    new2, h2b = _run(lib, cell, d, mask, dev, pitched, second=False)
    assert torch.equal(new2, new) and (h2b == SENTINEL).all()


@pytest.mark.parametrize("cell,N,H,kind", CASES)
def test_pitches_give_equal_bits(dev, cell, N, H, kind):
    lib = _lib.load()
    d = ref.kernel_inputs(cell, N, H)
    mask = ref.kernel_mask(N, kind)
    a = _run(lib, cell, d, mask, dev, False)
    b = _run(lib, cell, d, mask, dev, True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("cell,N,H", [(c, N, H) for c in CELLS for (N, H) in ref.KERNEL_CASES])
def test_mask_zero_is_the_cell_on_a_zero_state_with_the_same_x(dev, cell, N, H):
    """m = 0: the bits of the cell run with m = 1 on an all-zero previous state and the SAME x -- the mask never touches x"""
    lib = _lib.load()
    d = ref.kernel_inputs(cell, N, H)
    masked, _ = _run(lib, cell, d, torch.zeros(N), dev, False)
    zero, _ = _run(lib, cell, dict(d, state=torch.zeros_like(d["state"])), torch.ones(N), dev, False)
    assert torch.equal(masked, zero)
    other_x, _ = _run(lib, cell, dict(d, x=d["x"] + 0.5), torch.zeros(N), dev, False)
    assert not torch.equal(other_x[:N], masked[:N])


def test_refusals(dev):
    lib = _lib.load()
    N, H = 4, 64
    d = {k: v.to(dev).contiguous() for k, v in ref.kernel_inputs(ref.LSTM, N, H).items()}
    m = torch.ones(N, device=dev)
    out = torch.zeros(N, 2 * H, device=dev)

    def call(rnn=1, x=None, ld_x=H, ld_p=2 * H, H_=H, c_out=True, ld_h=2 * H):
        return lib.ec_rnn_stack_step_fwd(rnn, d["x"].data_ptr() if x is None else x, ld_x, d["wih"].data_ptr(), d["whh"].data_ptr(),
                                         d["bih"].data_ptr(), d["bhh"].data_ptr(), d["state"].data_ptr(), ld_p, m.data_ptr(), out.data_ptr(),
                                         ld_h, out.data_ptr() + 4 * H if c_out else 0, 2 * H, 0, 0, N, H_, 0)
    assert call() == 0
    assert call(rnn=2) == -1 and call(x=0) == -1 and call(c_out=False) == -1      # EC_ERR_ARG
    assert call(x=d["x"].data_ptr() + 4) == -1                                    # 16-byte alignment
    assert call(H_=40) == -2 and call(ld_x=H - 4) == -2 and call(ld_x=H + 2) == -2 and call(ld_p=H) == -2 and call(ld_h=32) == -2
    torch.cuda.synchronize()

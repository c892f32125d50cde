"""GPU: the two LSTM step entry points alone (``ec_lstm_step_fwd`` / ``ec_lstm_step_bwd``, csrc/lstm.hip) against the float64
closed forms of tests/_lstm_ref.py.

Cases (N, H) -- tests/_lstm_ref.py::KERNEL_CASES:
  (1, 32)    one lane row; whole-K staging; grid.x = 4
  (33, 64)   a second actor block holding one row
  (5, 256)   one LDS-DMA chunk
  (37, 512)  two chunks; the reference width
each with a mask holding both values (at one actor: the two single-value masks) and with the previous state at pitch 2H (rows
[h | c]) and at pitch H (stacked blocks [2, N, H]).  The backward runs fused where the geometry allows (H = 256, 512) and on the
gate-plus-GEMM route at every H.

Bound per output: rel-L2 <= 10 x the worst fp32-vs-float64 rel-L2 of the SAME closed form over this case table
(``_lstm_ref.kernel_bounds()``; 10 is the project's standing margin, tests/test_prev_action_ref.py: it covers a summation order that
differs from torch's).  Figures of ``python tests/_lstm_ref.py`` (fp32 torch against float64):
  h 1.24e-7   c 1.06e-7   gates 7.2e-8   da 7.6e-8   carry_h 2.56e-7   carry_c 6.2e-8   da (fused) 1.07e-7   carry_c (fused) 8.1e-8
Measured on an MI355X (worst over the table, the kernels against float64):
  h 1.16e-7   c 9.7e-8    gates 6.5e-8   da 7.7e-8   carry_h 6.2e-7    carry_c 5.4e-8   da (fused) 1.0e-7    carry_c (fused) 9.8e-8
"""
import os
import sys

import pytest
import torch

from embodied_clip_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _lstm_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
GUARD = 3                       # rows past N in every output
CASE_MASKS = [(N, H, mi) for (N, H) in ref.KERNEL_CASES for mi in range(len(ref.kernel_masks(N)))]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _inputs(N, H, mi):
    return ref.kernel_inputs(N, H, ref.kernel_masks(N)[mi])


def _guarded(N, W, dev, ld=None):
    """[N + GUARD, ld] filled with the sentinel; -> (buffer, the [N, W] view the kernel writes)"""
    ld = ld or W
    buf = torch.full((N + GUARD, ld), SENTINEL, device=dev)
    return buf, buf[:N, :W]


def _fwd(lib, d, N, H, pitch, dev, with_gates=True):
    """one forward step with the previous state at `pitch`; h / c are written at pitch 2H into one guarded state buffer"""
    state = d["state"].to(dev)
    prev = state.contiguous() if pitch == 2 * H else torch.stack([state[:, :H], state[:, H:]]).contiguous()
    out, _ = _guarded(N, 2 * H, dev)
    gates, _ = _guarded(N, 4 * H, dev)
    a_in, whh, bhh, mask = (d[k].to(dev).contiguous() for k in ("a_in", "whh", "bhh", "mask"))
    _lib.check(lib.ec_lstm_step_fwd(a_in.data_ptr(), whh.data_ptr(), bhh.data_ptr(), prev.data_ptr(), pitch, mask.data_ptr(),
                                    out.data_ptr(), 2 * H, out.data_ptr() + 4 * H, 2 * H, gates.data_ptr() if with_gates else 0, N, H, 0),
               "ec_lstm_step_fwd")
    torch.cuda.synchronize()
    return out, gates


def _bwd(lib, d, N, H, fused, dev):
    t = {k: d[k].to(dev).contiguous() for k in ("dhs", "gates", "c", "cp", "mask", "whh", "da_next", "mask_next")}
    ch, _ = _guarded(N, H, dev)
    cc, _ = _guarded(N, H, dev)
    da, _ = _guarded(N, 4 * H, dev)
    ch[:N] = d["carry_h"].to(dev)
    cc[:N] = d["carry_c"].to(dev)
    whhT = t["whh"].t().contiguous()
    _lib.check(lib.ec_lstm_step_bwd(t["dhs"].data_ptr(), t["gates"].data_ptr(), t["c"].data_ptr(), t["cp"].data_ptr(), t["mask"].data_ptr(),
                                    t["whh"].data_ptr(), whhT.data_ptr() if fused else 0, t["da_next"].data_ptr() if fused else 0,
                                    t["mask_next"].data_ptr() if fused else 0, ch.data_ptr(), cc.data_ptr(), da.data_ptr(), N, H, 0),
               "ec_lstm_step_bwd")
    torch.cuda.synchronize()
    return da, ch, cc


def _check(name, got, want, bounds, key=None):
    if not want.any():                                   # exactly zero in every precision (one actor, mask 0)
        assert not got.any(), name
        return 0.0
    e = ref.rel_l2(got.cpu(), want)
    print(f"{name}: rel-L2 {e:.3e} (bound {bounds[key or name]:.3e})")
    assert e <= bounds[key or name], (name, e, bounds[key or name])
    return e


@pytest.mark.parametrize("pitch_2h", [True, False])
@pytest.mark.parametrize("N,H,mi", CASE_MASKS)
def test_forward_step(dev, N, H, mi, pitch_2h):
    lib = _lib.load()
    bounds = ref.kernel_bounds()
    d = _inputs(N, H, mi)
    want = ref.kernel_reference(d)
    pitch = 2 * H if pitch_2h else H
    out, gates = _fwd(lib, d, N, H, pitch, dev)
    _check("h", out[:N, :H], want["h"], bounds)
    _check("c", out[:N, H:], want["c"], bounds)
    _check("gates", gates[:N], want["gates"], bounds)
    assert (out[N:] == SENTINEL).all() and (gates[N:] == SENTINEL).all()          # rows past N are never written
    # gates = NULL: the same h and c, nothing else written; a second call: equal bits
    out2, gates2 = _fwd(lib, d, N, H, pitch, dev, with_gates=False)
    assert torch.equal(out2, out) and (gates2 == SENTINEL).all()
    out3, gates3 = _fwd(lib, d, N, H, pitch, dev)
    assert torch.equal(out3, out) and torch.equal(gates3, gates)


@pytest.mark.parametrize("N,H,mi", CASE_MASKS)
def test_pitches_give_equal_bits(dev, N, H, mi):
    """the previous state as [h | c] rows and as stacked blocks: the same arithmetic on the same numbers"""
    lib = _lib.load()
    d = _inputs(N, H, mi)
    a = _fwd(lib, d, N, H, 2 * H, dev)
    b = _fwd(lib, d, N, H, H, dev)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("N,H,mi", CASE_MASKS)
def test_backward_step_gate_plus_gemm(dev, N, H, mi):
    lib = _lib.load()
    bounds = ref.kernel_bounds()
    d = _inputs(N, H, mi)
    want = ref.kernel_reference(d)
    da, ch, cc = _bwd(lib, d, N, H, False, dev)
    _check("da", da[:N], want["da"], bounds)
    _check("carry_h", ch[:N], want["carry_h"], bounds)
    _check("carry_c", cc[:N], want["carry_c"], bounds)
    assert (da[N:] == SENTINEL).all() and (ch[N:] == SENTINEL).all() and (cc[N:] == SENTINEL).all()
    again = _bwd(lib, d, N, H, False, dev)
    assert all(torch.equal(x, y) for x, y in zip((da, ch, cc), again))


@pytest.mark.parametrize("N,H,mi", [c for c in CASE_MASKS if c[1] % 256 == 0])
def test_backward_step_fused(dev, N, H, mi):
    lib = _lib.load()
    bounds = ref.kernel_bounds()
    d = _inputs(N, H, mi)
    want = ref.kernel_reference(d)
    da, ch, cc = _bwd(lib, d, N, H, True, dev)
    _check("da_fused", da[:N], want["da_fused"], bounds)
    _check("carry_c_fused", cc[:N], want["carry_c_fused"], bounds)
    assert torch.equal(ch[:N].cpu(), d["carry_h"])                               # the fused step does not touch carry_h
    assert (da[N:] == SENTINEL).all() and (ch[N:] == SENTINEL).all() and (cc[N:] == SENTINEL).all()
    again = _bwd(lib, d, N, H, True, dev)
    assert all(torch.equal(x, y) for x, y in zip((da, ch, cc), again))


def test_refusals(dev):
    lib = _lib.load()
    N, H = 4, 64
    d = _inputs(N, H, 0)
    t = {k: v.to(dev).contiguous() for k, v in d.items() if torch.is_tensor(v)}
    out = torch.zeros(N, 2 * H, device=dev)
    args = lambda H_, pitch: (t["a_in"].data_ptr(), t["whh"].data_ptr(), t["bhh"].data_ptr(), t["state"].data_ptr(), pitch, t["mask"].data_ptr(),
                              out.data_ptr(), 2 * H, out.data_ptr() + 4 * H, 2 * H, 0, N, H_, 0)
    assert lib.ec_lstm_step_fwd(*args(40, 80)) == -2                              # EC_ERR_SHAPE: H % 32
    assert lib.ec_lstm_step_fwd(*args(H, H + 4)) == -2                            # a pitch between H and 2H
    assert lib.ec_lstm_step_fwd(0, *args(H, 2 * H)[1:]) == -1                     # EC_ERR_ARG
    # the fused reverse step needs H % 256 == 0
    z = torch.zeros(N, 4 * H, device=dev)
    assert lib.ec_lstm_step_bwd(t["dhs"].data_ptr(), t["gates"].data_ptr(), t["c"].data_ptr(), t["cp"].data_ptr(), t["mask"].data_ptr(), 0,
                                t["whh"].data_ptr(), t["da_next"].data_ptr(), t["mask_next"].data_ptr(), 0, out.data_ptr(), z.data_ptr(),
                                N, H, 0) == -2

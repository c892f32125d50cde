"""GPU: the two-view front's kernels alone (``ec_two_view_fwd`` / ``ec_two_view_bwd``, csrc/two_view.hip) against the float64
reference of tests/_two_view_ref.py, at every case of its table (B, S2, C, H, A1) and on three edge inputs.

Bounds (the policy path's own, tests/_rnn_stack_ref.py FWD_TOL / GRAD_TOL): rel-L2 2e-5 forward, 2e-4 per gradient tensor;
tests/test_two_view_ref.py checks on the CPU that the fp32 evaluation of the reference stays within a tenth of both.  The one
exception is the gradient of visual_attention.2.bias: it is analytically ZERO (softmax is shift-invariant), a relative error
against it is meaningless, so it is held to |g| <= GRAD_TOL * ||grad visual_attention.2.weight||.

Also: two backward calls give equal bits (ordered sums only); frames [a, b) computed alone equal the same rows of the full call
bit for bit -- across the two forward kernels too (B = 770 runs the five-tile kernel, its slices the two-tile one).

Measured on an MI355X, worst over the ten cases and the three edge inputs: forward 5.0e-7 (the full-width row), gradients 1.3e-5
(visual_attention.0.bias at B = 770, 8.5e-6 for its weight there; every other case below 5.8e-6), |grad visual_attention.2.bias|
at most 5.7e-7 of ||grad visual_attention.2.weight||; the logits-at-80 edge 4.7e-7 forward, 5.7e-6 gradients.
"""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _two_view_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = ref.KERNEL_CASES


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _case(case, edge=None):
    """Inputs and the float64 reference, computed once per (case, edge) and shared (never modified)."""
    sd, u, w, dv = ref.kernel_inputs(*case, edge=edge)
    v, grads = ref.front_reference(sd, u, w, dv)
    return dict(sd=sd, u=u, w=w, dv=dv, v=v, grads=grads)


class Front:
    """the two C-ABI calls on device tensors"""

    def __init__(self, case, c, dev):
        from embodied_clip_amd import _lib
        self._lib, self.lib = _lib, _lib.load()
        self.case, self.dev = case, dev
        f = lambda t: t.reshape(-1).float().contiguous().to(dev)
        self.p = {k: f(t) for k, t in c["sd"].items()}
        self.u, self.w = c["u"].to(torch.bfloat16).contiguous().to(dev), c["w"].to(torch.bfloat16).contiguous().to(dev)
        self.dv = c["dv"].float().contiguous().to(dev)

    def fwd(self, a=0, b=None, save=False):
        B, S2, Cc, H, A1 = self.case
        b = B if b is None else b
        n = b - a
        nbytes = self.lib.ec_two_view_workspace_bytes(n, S2, Cc, H, A1, int(save))
        assert nbytes > 0
        ws = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
        v = torch.empty(n, H, device=self.dev)
        u, w = self.u[a:b].contiguous(), self.w[a:b].contiguous()
        p = self.p
        self._lib.check(self.lib.ec_two_view_fwd(u.data_ptr(), w.data_ptr(), p[ref.FRONT[0]].data_ptr(), p[ref.FRONT[1]].data_ptr(),
                                                 p[ref.FRONT[2]].data_ptr(), p[ref.FRONT[3]].data_ptr(), p[ref.W2].data_ptr(),
                                                 p[ref.B2].data_ptr(), v.data_ptr(), n, S2, Cc, H, A1, ws.data_ptr(), nbytes, int(save),
                                                 self._lib.stream_ptr()), "ec_two_view_fwd")
        return v, ws

    def bwd(self, ws):
        B, S2, Cc, H, A1 = self.case
        g = {k: torch.zeros_like(t) for k, t in self.p.items()}
        self._lib.check(self.lib.ec_two_view_bwd(self.u.data_ptr(), self.w.data_ptr(), self.p[ref.W2].data_ptr(), self.dv.data_ptr(),
                                                 g[ref.FRONT[0]].data_ptr(), g[ref.FRONT[1]].data_ptr(), g[ref.FRONT[2]].data_ptr(),
                                                 g[ref.FRONT[3]].data_ptr(), g[ref.W2].data_ptr(), g[ref.B2].data_ptr(), B, S2, Cc, H, A1,
                                                 ws.data_ptr(), ws.numel(), self._lib.stream_ptr()), "ec_two_view_bwd")
        return g


def _check(case, edge, dev):
    c = _case(case, edge)
    k = Front(case, c, dev)
    v, ws = k.fwd(save=True)
    g = k.bwd(ws)
    again = k.bwd(ws)
    torch.cuda.synchronize()
    assert torch.isfinite(v).all()
    fe = ref.rel_l2(v, c["v"])
    ge = ref.grad_errors(g, c["grads"])
    print(case, edge, "forward rel-L2 %.3e; gradients" % fe, {n: "%.3e" % e for n, e in ge.items()})
    assert fe <= ref.FWD_TOL, fe
    for name, e in ge.items():
        assert e <= ref.GRAD_TOL, (name, e)
    for name in g:
        assert torch.equal(g[name], again[name]), name       # two backward calls: equal bits
    return k, v


@pytest.mark.parametrize("case", CASES)
def test_forward_and_gradients_match_reference(dev, case):
    k, v = _check(case, None, dev)
    v2, _ = k.fwd(save=False)                                 # the inference forward (stores nothing): the same bits
    torch.cuda.synchronize()
    assert torch.equal(v2, v)


@pytest.mark.parametrize("edge", ref.EDGES)
def test_edge_inputs(dev, edge):
    """a frame whose u is all zero; logits reaching +-80 through a scaled w_2 (finite, within the bounds); a dead encoder column"""
    case = (5, 49, 64, 32, 32)
    k, v = _check(case, edge, dev)
    if edge == "dead_column":
        assert float(v[:, 1].abs().max()) == 0.0


@pytest.mark.parametrize("case", [(33, 49, 192, 96, 32), (33, 9, 192, 32, 32), (770, 49, 64, 32, 32), (3, 49, 2048, 512, 32)])
def test_sliced_frames_equal_the_full_call(dev, case):
    """frames [a, b) computed alone == the same rows of the full call, bit for bit"""
    B = case[0]
    c = _case(case)
    k = Front(case, c, dev)
    v, _ = k.fwd()
    a, b = (1, 2) if B <= 3 else (B // 3 + 1, B - 2)
    va, _ = k.fwd(0, a)
    vb, _ = k.fwd(a, b)
    vc, _ = k.fwd(b, B)
    torch.cuda.synchronize()
    assert torch.equal(torch.cat([va, vb, vc]), v)


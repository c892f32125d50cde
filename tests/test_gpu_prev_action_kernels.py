"""GPU: the kernels of the previous-action embedding (csrc/prev_action.hip), each alone against the float64 closed forms of
tests/_prev_action_ref.py.

Cases: 3H in {96, 1536} x E in {1, 5, 6, 32, 64} x (A, null) in {(1,0), (6,1), (6,0), (7,1), (84,1), (256,1)}, each at B in
{1, 33, 1000} and four input patterns (random; every frame selects one table row; all masks 0; prev_actions -1 and A), with the
embedding's columns at the end of a weight whose leading dimension is no multiple of 4.

Bounds: the policy path's own (tests/test_gpu_policy.py) -- forward rel-L2 < 2e-5 for the table and the gather-add, per-tensor
gradient rel-L2 < 2e-4 for dPT, dEmb and dWa.  The fp32 torch evaluation of the same closed forms lies at most 1.7e-7 (pt),
1.6e-7 (gi), 4.8e-7 (dPT), 3.2e-7 (dEmb), 6.3e-7 (dWa) from float64 over these cases (`python tests/_prev_action_ref.py`;
tests/test_prev_action_ref.py holds each to a tenth of its bound).  The kernels on an MI355X, worst over all cases: pt 1.9e-7,
gi 1.6e-7, dPT 1.3e-7, dWa 8.3e-7, dEmb 1.6e-6 (at E = 1 and 1536 gate columns; measured when one wave summed a whole row serially -- the kernel now sums
four quarters and folds them, shorter chains; this test prints every figure before it asserts)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _prev_action_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _run(d, A, null, base=0.0):
    """the three kernels on one case -> dict(pt, gi, dpt, demb, dw); demb / dw start at `base`, every output the kernels must
    write whole starts as NaN"""
    from embodied_clip_amd import prev_action as pa
    t = {k: (v.to(DEV).contiguous() if torch.is_tensor(v) else v) for k, v in d.items()}
    B, G = t["gi"].shape
    R, E = t["emb"].shape
    pt = torch.full((R, G), float("nan"), device=DEV)
    pa.prev_action_table(t["emb"], t["w"], t["col0"], bool(null), out=pt)
    gi = t["gi"].clone()
    pa.prev_action_add_(gi, pt, t["prev"], t["masks"], bool(null))
    demb = torch.full((R, E), base, device=DEV)
    dw = torch.full_like(t["w"], base)
    scratch = pa.prev_action_grad_scratch(B, G, A, bool(null), DEV).fill_(float("nan"))
    dpt = pa.prev_action_grad_(t["dgi"], t["prev"], t["masks"], bool(null), t["emb"], t["w"], t["col0"], demb, dw, scratch)
    torch.cuda.synchronize()
    return dict(pt=pt.cpu(), gi=gi.cpu(), dpt=dpt.clone().cpu(), demb=demb.cpu(), dw=dw.cpu())


@pytest.mark.parametrize("G,E,A,null", ref.KERNEL_CASES)
def test_kernels_against_float64(G, E, A, null):
    figs = {}
    for B in ref.BS:
        for pattern in ref.PATTERNS:
            d = ref.kernel_inputs(G, E, A, null, B, pattern)
            want = ref.kernel_reference(d, A, null)
            got, again = _run(d, A, null), _run(d, A, null)
            col0, idx = d["col0"], want["idx"]
            fig = dict(pt=ref.rel_l2(got["pt"], want["pt"]), gi=ref.rel_l2(got["gi"], want["gi"]),
                       dpt=ref.rel_l2(got["dpt"], want["dpt"]), demb=ref.rel_l2(got["demb"], want["demb"]),
                       dwa=ref.rel_l2(got["dw"][:, col0:], want["dwa"]))
            print(f"G {G} E {E} A {A} null {null} B {B} {pattern}: " + " ".join(f"{k} {v:.3e}" for k, v in fig.items()))
            for k, v in fig.items():
                figs[k] = max(figs.get(k, 0.0), v)
            for k in got:                                            # two runs: the same bits
                assert torch.equal(got[k], again[k]), (k, B, pattern)
            assert not got["dw"][:, :col0].any(), "columns in front of the embedding's were written"
            # a frame outside the table keeps its gi row, bit for bit
            assert torch.equal(got["gi"][idx < 0], d["gi"][idx < 0])
            # rows nobody selects: exactly 0
            unselected = torch.ones(A + null, dtype=torch.bool)
            unselected[idx[idx >= 0]] = False
            assert not got["dpt"][unselected].any() and not got["demb"][unselected].any(), (B, pattern)
            if pattern == "masks_zero" and null:
                assert (idx == 0).all() and not got["demb"][1:].any()
            if pattern == "out_of_range" and not null:
                assert not got["dpt"].any() and not got["demb"].any() and not got["dw"].any()
                assert torch.equal(got["gi"], d["gi"])
            for k in ("pt", "gi"):
                assert fig[k] < ref.FWD_TOL, (k, fig[k], B, pattern)
            for k in ("dpt", "demb", "dwa"):
                assert fig[k] < ref.GRAD_TOL, (k, fig[k], B, pattern)
    print(f"worst of G {G} E {E} A {A} null {null}: " + " ".join(f"{k} {v:.3e}" for k, v in figs.items()))


@pytest.mark.parametrize("G,E,A,null", [(96, 6, 6, 1), (1536, 5, 84, 1)])
def test_gradients_add_onto_what_is_there(G, E, A, null):
    d = ref.kernel_inputs(G, E, A, null, 33)
    zero, half = _run(d, A, null), _run(d, A, null, base=0.5)
    col0 = d["col0"]
    assert torch.equal(half["demb"], 0.5 + zero["demb"])
    assert torch.equal(half["dw"][:, col0:], 0.5 + zero["dw"][:, col0:])
    assert torch.equal(half["dw"][:, :col0], torch.full((G, col0), 0.5))
    assert torch.equal(half["dpt"], zero["dpt"])


@pytest.mark.parametrize("G,shift", [(96, 1), (98, 0), (1, 0)])
def test_gather_add_without_float4(G, shift):
    """gi at a base that is not 16-byte aligned, and G no multiple of 4: the one-float route"""
    from embodied_clip_amd import prev_action as pa
    E, A, null, B = 6, 6, 1, 33
    d = ref.kernel_inputs(G, E, A, null, B)
    want = ref.kernel_reference(d, A, null)
    pt = pa.prev_action_table(d["emb"].to(DEV), d["w"].to(DEV), d["col0"], True)
    buf = torch.zeros(B * G + 4, device=DEV)
    gi = buf[shift:shift + B * G].view(B, G)
    gi.copy_(d["gi"])
    pa.prev_action_add_(gi, pt, d["prev"].to(DEV), d["masks"].to(DEV), True)
    torch.cuda.synchronize()
    assert ref.rel_l2(gi.cpu(), want["gi"]) < ref.FWD_TOL
    assert not buf[:shift].any() and not buf[shift + B * G:].any()

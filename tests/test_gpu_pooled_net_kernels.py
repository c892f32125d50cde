"""GPU: the pooled-embedding net's two act-step kernels alone (``ec_pooled_fc_act``, ``ec_pooled_step0_fwd``) against float64.

Bounds.  Both kernels contract on v_mfma_f32_32x32x2_f32, an fp32 FMA chain, and fold a handful of partial sums in a fixed
order: their results are fp32 evaluations of the closed form in another summation order.  The bound of an output is therefore
10 x the worst rel-L2 distance of the fp32 closed form (torch, CPU) from float64 over the kernel's case table -- the rule of
tests/_rnn_stack_ref.py::kernel_bounds -- and never what the kernel gives.  The bounds come to 3 .. 4e-6 (visual_fc; the host's
BLAS decides) and about 2.4e-6 / 2.8e-6 / 2.5e-6 (the step's h on the GRU, h and c on the LSTM); measured on an MI355X visual_fc
lies at 0.8e-7 .. 2.9e-7 and the step's h at 1.1e-7 .. 2.1e-7.
"""
import functools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _pooled_net_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
GRU, LSTM = ref.GRU, ref.LSTM


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from embodied_clip_amd import _lib
    return _lib.load()


def _p(t):
    return 0 if t is None else t.data_ptr()


# ---- visual_fc -------------------------------------------------------------------------------------------------------------------
FC_CASES = [(N, D, H) for N in (1, 33) for (D, H) in ((64, 32), (112, 96), (2048, 512))]


def _fc_inputs(N, D, H):
    g = torch.Generator().manual_seed(D + H + N)
    return torch.randn(N, D, generator=g), torch.randn(H, D, generator=g) / D ** 0.5, 0.1 * torch.randn(H, generator=g)


@functools.lru_cache(maxsize=None)
def _fc_bound():
    worst = 0.0
    for case in FC_CASES:
        e, w, b = _fc_inputs(*case)
        worst = max(worst, ref.rel_l2(torch.relu(F.linear(e, w, b)), torch.relu(F.linear(e.double(), w.double(), b.double()))))
    return 10 * worst


@pytest.mark.parametrize("N,D,H", FC_CASES)
def test_fc_act_kernel(dev, lib, D, H, N):
    from embodied_clip_amd import _lib
    e, w, b = _fc_inputs(N, D, H)
    pre = F.linear(e.double(), w.double(), b.double())
    want = torch.relu(pre)
    bound = _fc_bound()
    assert (want > 0).any() and (want == 0).any()
    pad = 3
    v = torch.full((N + pad, H), -7.0, device=dev)
    ed, wd, bd = e.to(dev), w.to(dev), b.to(dev)
    wfrag = torch.empty(H * D, device=dev)
    with _lib.tensor_guard(ed):
        _lib.check(lib.ec_pooled_fc_act(ed.data_ptr(), wd.data_ptr(), bd.data_ptr(), wfrag.data_ptr(), v.data_ptr(), N, D, H, _lib.stream_ptr()))
    torch.cuda.synchronize()
    err = ref.rel_l2(v[:N], want)
    print(f"fc (N={N}, D={D}, H={H}): rel-L2 {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    assert bool((v[N:] == -7.0).all())                     # rows past N untouched
    clear = pre.abs() > 1e-4                               # away from the kink, the ReLU cuts where the reference cuts
    assert bool((((v[:N] == 0).cpu() == (want == 0)) | ~clear).all())


# ---- layer 0's step ----------------------------------------------------------------------------------------------------------------
def _step_inputs(cell, N, H, seed):
    G = (4 if cell == LSTM else 3) * H
    SW = (2 if cell == LSTM else 1) * H
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    A, NG, K = 6, 12, 4
    d = dict(x=0.7 * r(N, H), wih=r(G, H) / H ** 0.5, whh=r(G, H) / H ** 0.5, bih=0.1 * r(G), bhh=0.1 * r(G), state=0.5 * r(N, SW),
             sb=0.1 * r(G), gt=0.3 * r(NG, G), pt=0.3 * r(A + 1, G), sv=0.3 * r(G, K), sens=r(N, K),
             goal=torch.randint(0, NG, (N,), generator=g), prev=torch.randint(0, A, (N,), generator=g),
             mask=(torch.arange(N) % 3 != 1).float() if N > 1 else torch.zeros(1))
    return d, A, NG, K


def _step_reference(cell, d, parts, A, dtype):
    """the layer's new state [N, SW] in `dtype`; `parts`: which of sb / gt / pt / sv take part"""
    c = lambda t: t.to(dtype) if t.is_floating_point() else t
    t = {k: c(v) for k, v in d.items()}
    H = t["whh"].shape[1]
    m = t["mask"].reshape(-1, 1)
    gi = F.linear(t["x"], t["wih"], t["bih"])
    if "sb" in parts:
        gi = gi + t["sb"]
    if "gt" in parts:
        gi = gi + t["gt"][t["goal"]]
    if "pt" in parts:                                      # null token: row 0 where the mask is zero, else action + 1
        idx = torch.where(t["mask"] == 0, torch.zeros_like(t["prev"]), t["prev"] + 1)
        gi = gi + t["pt"][idx]
    if "sv" in parts:
        gi = gi + t["sens"] @ t["sv"].t()
    hp = m * t["state"][:, :H]
    gh = F.linear(hp, t["whh"], t["bhh"])
    if cell == LSTM:
        cp = m * t["state"][:, H:]
        i, f, g, o = (gi + gh).chunk(4, -1)
        cn = torch.sigmoid(f) * cp + torch.sigmoid(i) * torch.tanh(g)
        return torch.cat([torch.sigmoid(o) * torch.tanh(cn), cn], -1)
    ir, iz, inn = gi.chunk(3, -1)
    hr, hz, hnn = gh.chunk(3, -1)
    r, z = torch.sigmoid(ir + hr), torch.sigmoid(iz + hz)
    return (1 - z) * torch.tanh(inn + r * hnn) + z * hp


PART_SETS = [(), ("sb", "gt", "pt", "sv"), ("gt",), ("pt",), ("sb", "sv")]
STEP_CASES = [(cell, H, N) for cell in (GRU, LSTM) for H in (64, 256, 512) for N in (5, 33)]


def _step_seed(cell, H, N):
    return 31 * H + N + (1 if cell == LSTM else 0)


@functools.lru_cache(maxsize=None)
def _step_bounds():
    """{(cell, "h" | "c"): 10 x the worst fp32-vs-float64 rel-L2 of the closed form over the cases and part sets}"""
    worst = {}
    for (cell, H, N) in STEP_CASES:
        d, A, NG, K = _step_inputs(cell, N, H, _step_seed(cell, H, N))
        for parts in PART_SETS:
            r64, r32 = _step_reference(cell, d, parts, A, torch.float64), _step_reference(cell, d, parts, A, torch.float32)
            worst[(cell, "h")] = max(worst.get((cell, "h"), 0.0), ref.rel_l2(r32[:, :H], r64[:, :H]))
            if cell == LSTM:
                worst[(cell, "c")] = max(worst.get((cell, "c"), 0.0), ref.rel_l2(r32[:, H:], r64[:, H:]))
    return {k: 10 * v for k, v in worst.items()}


@pytest.mark.parametrize("parts", PART_SETS, ids=lambda p: "+".join(p) or "none")
@pytest.mark.parametrize("cell,H,N", STEP_CASES)
def test_step0_kernel(dev, lib, cell, H, N, parts):
    from embodied_clip_amd import _lib
    d, A, NG, K = _step_inputs(cell, N, H, _step_seed(cell, H, N))
    want = _step_reference(cell, d, parts, A, torch.float64)
    lstm = cell == LSTM
    SW = (2 if lstm else 1) * H
    bound_h = _step_bounds()[(cell, "h")]
    t = {k: v.to(dev) for k, v in d.items()}
    # pitched state rows: the previous state inside [N, SW + 8] rows, the new one inside [N + 2, 2 * SW + 4] rows
    ld_prev, ld_out = SW + 8, 2 * SW + 4
    prev_rows = torch.zeros(N, ld_prev, device=dev)
    prev_rows[:, :SW] = t["state"]
    out_rows = torch.full((N + 2, ld_out), -7.0, device=dev)
    h2 = torch.full((N + 2, H), -7.0, device=dev)
    on = lambda k: k in parts
    with _lib.tensor_guard(prev_rows):
        rc = lib.ec_pooled_step0_fwd(
            1 if lstm else 0, t["x"].data_ptr(), H, t["wih"].data_ptr(), t["whh"].data_ptr(), t["bih"].data_ptr(), t["bhh"].data_ptr(),
            _p(t["sb"] if on("sb") else None), _p(t["gt"] if on("gt") else None), _p(t["goal"] if on("gt") else None), NG,
            _p(t["pt"] if on("pt") else None), _p(t["prev"] if on("pt") else None), 1, A, _p(t["sv"] if on("sv") else None),
            _p(t["sens"] if on("sv") else None), K if on("sv") else 0, prev_rows.data_ptr(), ld_prev, t["mask"].data_ptr(),
            out_rows.data_ptr(), ld_out, out_rows.data_ptr() + 4 * H if lstm else 0, ld_out, h2.data_ptr(), H, N, H, _lib.stream_ptr())
    _lib.check(rc, "ec_pooled_step0_fwd")
    torch.cuda.synchronize()
    err_h = ref.rel_l2(out_rows[:N, :H], want[:, :H])
    print(f"step0 {cell} H={H} N={N} parts={parts}: h rel-L2 {err_h:.3e} (bound {bound_h:.3e})")
    assert err_h <= bound_h
    assert torch.equal(h2[:N], out_rows[:N, :H])           # the dense copy for the heads
    if lstm:
        bound_c = _step_bounds()[(cell, "c")]
        err_c = ref.rel_l2(out_rows[:N, H:SW], want[:, H:])
        assert err_c <= bound_c, (err_c, bound_c)
    assert bool((out_rows[N:] == -7.0).all()) and bool((h2[N:] == -7.0).all())      # rows past N untouched
    assert bool((out_rows[:N, SW:] == -7.0).all())                                  # ... and the columns beside the state


def test_step0_parts_matter_and_in_place_is_refused(dev, lib):
    """each table changes the result (so each is read), an out-of-range goal id adds nothing, and in place is EC_ERR_ARG"""
    from embodied_clip_amd import _lib
    cell, N, H = GRU, 5, 64
    d, A, NG, K = _step_inputs(cell, N, H, 5)
    full = _step_reference(cell, d, ("sb", "gt", "pt", "sv"), A, torch.float64)
    for drop in ("sb", "gt", "pt", "sv"):
        rest = tuple(k for k in ("sb", "gt", "pt", "sv") if k != drop)
        assert ref.rel_l2(_step_reference(cell, d, rest, A, torch.float64), full) > 1e-3, drop
    t = {k: v.to(dev) for k, v in d.items()}

    def run(goal, out):
        return lib.ec_pooled_step0_fwd(0, t["x"].data_ptr(), H, t["wih"].data_ptr(), t["whh"].data_ptr(), t["bih"].data_ptr(), t["bhh"].data_ptr(), 0,
                                       t["gt"].data_ptr(), goal.data_ptr(), NG, 0, 0, 0, A, 0, 0, 0, t["state"].data_ptr(), H, t["mask"].data_ptr(),
                                       out.data_ptr(), H, 0, 0, 0, 0, N, H, _lib.stream_ptr())
    out = torch.empty(N, H, device=dev)
    bad = t["goal"].clone()
    bad[0], bad[1] = NG, -1                                 # outside the table: no row is read for these frames
    assert run(bad, out) == 0
    torch.cuda.synchronize()
    want_none = _step_reference(cell, d, (), A, torch.float64)
    want_gt = _step_reference(cell, d, ("gt",), A, torch.float64)
    assert ref.rel_l2(out[:2], want_none[:2]) < 1e-5 and ref.rel_l2(out[2:], want_gt[2:]) < 1e-5
    assert run(t["goal"], t["state"]) == -1

"""GPU: every registered instance of gemm_f32_kernel / gemm_x3_kernel (36 of 36) through ec_gemm_f32 against the float64 references
and element-wise bounds of tests/_policy_gemm_ref.py -- no margin on top of the derived bounds (the CPU suite checks that those
bounds bite and that each case launches the instance it names: tests/test_policy_gemm_ref.py).  One child process per switch setting
(tests/_policy_gemm_check.py), one at a time; a child that ends by signal or at its time limit stops every later child of the whole run
before it starts a process (tests/_child.py).  With them the two relatives of the same arithmetic: ec_split3_bf16 (the planes sum to the input exactly)
and ec_dw_tn_x3 (dw_tn_x3_kernel<3>; dw_tn_x3_kernel<2> is reachable only through the learn pass: tests/test_gpu_learn_routes.py).

Measured worst |error| / bound per instance on an MI355X (every case under 1: the pass threshold is 1.0, not these figures).
x3<tile> = gemm_x3_kernel, f32<tile> = gemm_f32_kernel; operand types A/B (f = fp32, b = bf16), layouts A then B (k = k-contiguous,
r / n = row-contiguous); where the no_x3 setting reaches the instance again its figure follows the slash:
  x3<64, 64>    ff kk 0.012 (3PRODUCTS 0.036)  ff kn 0.041  ff rk 0.005  ff rn 0.005  bf kk 0.008  bf kn 0.007  fb kn 0.003  fb rn 0.002
  x3<128, 128>  ff kk 0.011  ff kn 0.319  ff rk 0.003  ff rn 0.002  bf kk 0.017  bf kn 0.007  fb kn 0.513  fb rn 0.005
  x3<256, 32>   ff kk 0.012  ff kn 0.306  ff rk 0.003  ff rn 0.005  bf kk 0.015  bf kn 0.006  fb kn 0.006  fb rn 0.010
  f32<64, 64>   ff 0.109 / 0.026  bf 0.062 / 0.081  fb 0.033       f32<128, 128>  ff 0.377 / 0.452  bf 0.022 / 0.024  fb 0.010 / 0.014
  f32<256, 32>  ff 0.015  bf 0.022 / 0.052  fb 0.026               f32<32, 256>   ff 0.006 / 0.013  bf 0.026  fb 0.016
The cases at 0.3 .. 0.5 are the rowscale (+ dmask + ACCUMULATE) ones: there the one rounding of the scaled value and of C0 + v is most
of the bound; elsewhere the worst-case accumulation term is, which a random-walk error stays far under (the x3 chain is charged six
additions per k) -- the plane accounting is what holds those to the six products: relative L2 of the kernel 5.6e-8 .. 1.3e-7 against
thresholds 2.7e-7 .. 6.5e-7 (six-product emulation 5.0e-8 .. 1.1e-7, three-product 1.5e-6 .. 4.1e-6).  Every guard element intact,
every parts case bit-identical twice, the fp32-kernel 3PRODUCTS twin bit-identical, the x3 one different.
ec_dw_tn_x3: 0.10 (M = 31, NX = 256), 0.09 (31, 768), 0.16 (64, 256), 0.06 (64, 768), under 0.001 at 49,017 tokens (zero-mean dY: the
error walks, the bound adds).  The file takes 9.4 s in all (launch to synchronize: default 11 ms for 47 cases, no_x3 3 .. 9 ms for 7;
the rest is the float64 references, the emulations behind the L2 thresholds and the start of the two child processes).
"""
import json
import os
import sys

import pytest
import torch

import _policy_gemm_ref as R
from _child import GPU, last_json
from _guard import SENT16, SENT32

pytestmark = pytest.mark.gpu

CHILD_LIMIT = 300


@pytest.mark.parametrize("setting", list(R.SETTINGS))
def test_policy_gemm_in_a_child_process(setting):
    """Every case of the setting once: worst |error| / bound <= 1, every guard element (a tile of rows before and after the output,
    the columns from N up to ldc) bitwise untouched, no NaN left in the written region; the plane accounting of the six-product x3
    cases; a parts case run twice is bit-identical; EC_GEMM_3PRODUCTS changes the bits of an x3 case and none of an fp32-kernel one."""
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_policy_gemm_check.py")
    p = GPU.run([sys.executable, script, setting], drop=R.SWITCHES, env=R.SETTINGS[setting], limit=CHILD_LIMIT)
    print("\n".join(p.stdout.splitlines()[:-1])[-20000:])
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    res = last_json(p)
    cases = R.cases_of(setting)
    assert res["setting"] == setting and [c["cmd"] for c in res["cases"]] == [c["cmd"] for c in cases]
    worst = {}
    for c, want in zip(res["cases"], cases):
        assert c["instance"] == want["instance"]
        worst[c["instance"]] = max(worst.get(c["instance"], 0.0), c["ratio"])
    print("worst per instance", setting, json.dumps(worst, indent=0))
    print("GPU seconds (launch to synchronize)", setting, sum(c["gpu_s"] for c in res["cases"]))
    for c, want in zip(res["cases"], cases):
        d = R.shape(want)
        assert c["guards_ok"], c
        assert c["nan_free"], c
        assert c["ratio"] <= 1.0, c
        assert ("l2" in c) == R.needs_l2(want) and ("twice_same" in c) == d["parts"] and ("twin_equal" in c) == d["p3"], c
        if "l2" in c:
            assert c["l2"] < c["l2_threshold"], c
        if d["parts"]:
            assert c["twice_same"], c
        if d["p3"]:
            assert c["twin_equal"] == (not d["x3"]), c


def _from_bits(bits):
    return torch.tensor(bits, dtype=torch.int64).to(torch.int32).view(torch.float32)


def _split_inputs(n):
    """n fp32 values: +-0; bf16 rounding ties (low half 0x8000 over an even and an odd leading part) and their fp32 neighbours;
    2^-120-scale multiples of 2^-133, the smallest bf16 subnormal; full 24-bit significands at 2^-100; the largest finite values
    whose leading plane stays finite (up to bit pattern 0x7f7f7fff); ordinary values."""
    g = torch.Generator().manual_seed(n)
    ties = [hi << 16 | lo for hi in (0x3F80, 0x3F81, 0x4049, 0x0A7F, 0x7E7F) for lo in (0x7FFF, 0x8000, 0x8001)]
    ties += [b | 0x80000000 for b in ties]
    sign = torch.tensor([1.0, -1.0], dtype=torch.float64).repeat(8)
    top = [0x7F7F7FFF, 0xFF7F7FFF, 0x7F7F0000, 0x7F7E8000, 0x7F7EFFFF, 0x7F000001]
    special = torch.cat([torch.tensor([0.0, -0.0]), _from_bits(ties), _from_bits(top),
                         (torch.randint(2 ** 10, 2 ** 13, (16,), generator=g).double() * sign * 2.0 ** -133).float(),
                         ((1 + torch.rand(16, generator=g, dtype=torch.float64)) * sign * 2.0 ** -100).float()])
    body = torch.randn(n, generator=g) * torch.exp2(torch.randint(-20, 20, (n,), generator=g).float())
    k = min(n, special.numel())
    body[torch.randperm(n, generator=g)[:k]] = special[torch.randperm(special.numel(), generator=g)[:k]]
    return body


@pytest.mark.parametrize("rows,K", [(1, 4), (1, 36), (257, 4), (257, 36)])
def test_split3_planes_sum_exactly(rows, K):
    """ec_split3_bf16: planes[:, 0] + planes[:, 1] + planes[:, 2] in float64 IS W, bit for bit, and nothing outside the planes is
    written.  Range limits: above bit pattern 0x7f7f7fff (|x| >= (2 - 2^-8) 2^127) the leading plane rounds to infinity -- asserted
    below, so the limit is documented by a test; below, a value must be a multiple of 2^-133 (the smallest bf16 subnormal): any
    fp32 value of magnitude 2^-110 or more is, and the 2^-120-scale inputs here are chosen so."""
    from embodied_clip_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    w = _split_inputs(rows * K).view(rows, K)
    assert rows * K < 128 or bool((w == 0).any() and (w.abs() > 3e38).any() and ((w != 0) & (w.abs() < 1e-35)).any())
    n = rows * 3 * K
    buf = torch.full((n + 128,), SENT16, dtype=torch.int16, device=dev)
    _lib.check(lib.ec_split3_bf16(w.to(dev).data_ptr(), buf.data_ptr() + 128, rows, K, _lib.stream_ptr()))
    torch.cuda.synchronize()
    o = buf.cpu()
    assert bool((o[:64] == SENT16).all() and (o[64 + n:] == SENT16).all())
    planes = o[64:64 + n].view(torch.bfloat16).view(rows, 3, K)
    assert torch.equal(planes.double().sum(1), w.double())
    assert torch.equal(planes[:, 0], w.to(torch.bfloat16))                 # the leading plane is the nearest-even rounding
    # the range limit: the leading plane of the values above 0x7f7f7fff is infinite
    big = _from_bits([0x7F7F8000, 0x7F7FFFFF, 0xFF7F8000, 0x7F7F7FFF]).repeat(rows * K // 4).view(rows, K)
    pb = torch.empty(rows, 3, K, dtype=torch.bfloat16, device=dev)
    _lib.check(lib.ec_split3_bf16(big.to(dev).data_ptr(), pb.data_ptr(), rows, K, _lib.stream_ptr()))
    torch.cuda.synchronize()
    lead = pb.cpu()[:, 0].float().view(-1, 4)
    assert bool(torch.isinf(lead[:, :3]).all() and torch.isfinite(lead[:, 3]).all())
    assert torch.equal(pb.cpu().double().sum(1).view(-1, 4)[:, 3], big.double().view(-1, 4)[:, 3])


@pytest.mark.parametrize("M,NX", [(31, 256), (64, 768), (1000 * 49 + 17, 256), (31, 768), (64, 256), (1000 * 49 + 17, 768)])
def test_dw_tn_x3_within_the_derived_bound(M, NX):
    """ec_dw_tn_x3 (dw_tn_x3_kernel<3> + dw_reduce_kernel) against float64 with the bound of _policy_gemm_ref.dw_reference: a single
    ragged K-tile, two full ones, and 49,017 tokens over every split; `part` and dW sit between sentinel guards."""
    from embodied_clip_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    op = R.dw_operands(M, NX)
    ns = lib.ec_dw_tn_x3_splits(M, NX)
    assert ns == R.dw_splits(M, NX)[0]
    planes = torch.empty(M, 3, 128, dtype=torch.bfloat16, device=dev)
    _lib.check(lib.ec_split3_bf16(op["dy"].to(dev).data_ptr(), planes.data_ptr(), M, 128, _lib.stream_ptr()))
    G = 128 * NX
    part = torch.full(((ns + 2) * G,), SENT32, dtype=torch.int32, device=dev)
    part[G:(ns + 1) * G] = torch.full((ns * G,), float("nan")).view(torch.int32).to(dev)
    dw = torch.full((3 * G,), SENT32, dtype=torch.int32)
    dw.view(torch.float32)[G:2 * G] = op["w0"].reshape(-1)
    dw = dw.to(dev)
    x = op["x"].to(dev)
    _lib.check(lib.ec_dw_tn_x3(planes.data_ptr(), x.data_ptr(), part.data_ptr() + 4 * G, dw.data_ptr() + 4 * G, M, NX, _lib.stream_ptr()))
    torch.cuda.synchronize()
    po, do = part.cpu(), dw.cpu()
    assert bool((po[:G] == SENT32).all() and (po[(ns + 1) * G:] == SENT32).all() and (do[:G] == SENT32).all() and (do[2 * G:] == SENT32).all())
    assert not bool(torch.isnan(po[G:(ns + 1) * G].view(torch.float32)).any())
    ref, bound = R.dw_reference(op, ns)
    r, at = R.worst_ratio(do[G:2 * G].view(torch.float32).view(128, NX), ref, bound)
    print(f"dw_tn_x3 M={M} NX={NX} splits {ns}: ratio {r:.2e} at {[at // NX, at % NX]}")
    assert r <= 1.0, (M, NX, r, at)

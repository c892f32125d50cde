"""GPU: the class embedding alone.  The three kernels of the CLS-only last block (vit_cls.hip), each through its stage entry point,
against the float64 references and element-wise bounds of tests/_vit_cls_ref.py -- no margin on top of the derived bounds (the CPU
suite checks that they bite: tests/test_vit_cls_ref.py); then ``ViTEmbedder.embed_cls`` and the preprocessor's ``cls_shortcut`` on
BOTH routes (EC_VIT_CLS_TAIL = 1: the CLS tail, 0: the general route; the switch is read once per process, hence the children)
and on the library's default, against ``oracle.clip_vit.vit_embedder(class_emb_only=True)`` with the tolerances
tests/test_gpu_vit.py states for this path: rel-L2 < 1e-2 against the bf16-emulating oracle, < 3e-2 against the fp32 oracle.
Each test prints its figures before it asserts.

Measured on an MI355X (worst |error| / bound; every case under 1, so no bound carries a margin):
  ec_gemm_rows_bf16     0.94 (M = 130, N = 32, K = 64, residual, bf16 written as fp32); the fp32 store 0.02
  ec_vit_cls_attn       class row 0.45, every row as the query 0.47
  ec_vit_cls_rows_ln    0.995 (the one bf16 rounding of the result is the whole budget)
  embed_cls             rel-L2 2.9e-3 .. 7.2e-3 against the emulating oracle, 3.6e-3 .. 8.1e-3 against the fp32 oracle on both
                        routes (the oracles differ by 3.5e-3 .. 8.3e-3 on these towers); the two routes 1.5e-3 .. 2.6e-3 apart"""
import os
import sys

import pytest
import torch

import _vit_cls_ref as R
from _child import GPU
from _guard import SENT16, SENT32
from _vit_cls_towers import TOWERS, golden_case, tower_case
from embodied_clip_amd import _lib
from oracle import clip_vit as ovit

pytestmark = pytest.mark.gpu

PAD = 8                    # rows behind every output that must keep the sentinel


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-20))


# ---- ec_gemm_rows_bf16 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.gemm_cases(), ids=R.gemm_id)
def test_gemm_rows_against_float64(lib, dev, c):
    op = R.gemm_inputs(c)
    ref, bound = R.gemm_ref(c, op)
    M, N, K = c["M"], c["N"], c["K"]
    ldo = N + 32                                       # the output has a pitch of its own; the columns past N keep the sentinel
    f32 = c["store"] != R.STORE_BF16
    out = torch.full((M + PAD, ldo), SENT32 if f32 else SENT16, dtype=torch.int32 if f32 else torch.int16, device=dev)
    d = {k: (v.to(dev) if v is not None else None) for k, v in op.items()}
    ldr = op["res"].shape[1] if op["res"] is not None else 0
    _lib.check(lib.ec_gemm_rows_bf16(d["A"].data_ptr(), c["lda"], d["W"].data_ptr(), _lib.ptr(d["bias"]), _lib.ptr(d["res"]), ldr,
                                     out.data_ptr(), ldo, M, N, K, c["act"], c["store"], _lib.stream_ptr()), "ec_gemm_rows_bf16")
    torch.cuda.synchronize()
    o = out.cpu()
    got = o[:M, :N].contiguous().view(torch.float32 if f32 else torch.bfloat16)
    sent = SENT32 if f32 else SENT16
    r = R.worst_ratio(got, ref, bound)
    print(f"ratio ec_gemm_rows_bf16 {R.gemm_id(c)}: {r:.3f}")
    assert bool((o[M:] == sent).all()) and bool((o[:M, N:] == sent).all()), "written outside [M, N]"
    if c["store"] == R.STORE_BF16_AS_F32:
        assert torch.equal(got, got.to(torch.bfloat16).float()), "store 1 delivers bf16 values"
    assert r <= 1.0, r


# ---- ec_vit_cls_attn ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,L,heads", R.ATTN_CASES)
def test_cls_attn_against_float64(lib, dev, B, L, heads):
    """row 0 of every frame as the query, then every other row in its place: in the 'reverse' inputs row i is dominated by key
    L - 1 - i, so every key of every (frame, head) dominates one call"""
    D = heads * 64
    qkv, q_rows, kv = R.attn_inputs(B, L, heads)
    ref, bound, _ = R.attn_ref(qkv, B, L, heads)
    dq, dkv = q_rows.to(dev), kv.to(dev)
    out = torch.full((L, B + PAD, D), SENT16, dtype=torch.int16, device=dev)
    for i in range(L):
        _lib.check(lib.ec_vit_cls_attn(dq[i].data_ptr(), dkv.data_ptr(), out[i].data_ptr(), B, L, D, heads, _lib.stream_ptr()),
                   "ec_vit_cls_attn")
    torch.cuda.synchronize()
    o = out.cpu()
    got = o[:, :B].contiguous().view(torch.bfloat16)
    r0 = R.worst_ratio(got[0], ref[0], bound[0])
    r = R.worst_ratio(got, ref, bound)
    print(f"ratio ec_vit_cls_attn B={B} L={L} heads={heads}: class row {r0:.3f}, every row as the query {r:.3f}")
    assert bool((o[:, B:] == SENT16).all()), "rows past B were written"
    assert r0 <= 1.0 and r <= 1.0, (r0, r)


# ---- ec_vit_cls_rows_ln ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", R.LN_DIMS)
def test_cls_rows_ln_against_float64(lib, dev, D):
    worst = 0.0
    for pm in R.LN_PITCH:
        for rows in R.LN_ROWS:
            for family in R.LN_FAMILIES:
                buf, gamma, beta = R.ln_inputs(family, rows, D, pm)
                ref, bound = R.layernorm_ref(buf[:, :D].to(R.F64), gamma, beta)
                out = torch.full((rows + PAD, D), SENT16, dtype=torch.int16, device=dev)
                dx, dg, db = buf.to(dev), gamma.to(dev), beta.to(dev)
                _lib.check(lib.ec_vit_cls_rows_ln(dx.data_ptr(), pm * D, dg.data_ptr(), db.data_ptr(), out.data_ptr(), rows, D,
                                                  _lib.stream_ptr()), "ec_vit_cls_rows_ln")
                torch.cuda.synchronize()
                o = out.cpu()
                r = R.worst_ratio(o[:rows].view(torch.bfloat16), ref, bound)
                print(f"ratio ec_vit_cls_rows_ln D={D} pitch={pm}D rows={rows} {family}: {r:.3f}")
                assert bool((o[rows:] == SENT16).all()), (pm, rows, family)
                assert r <= 1.0, (pm, rows, family, r)
                worst = max(worst, r)
    print(f"worst ec_vit_cls_rows_ln D={D}: {worst:.3f}")


# ---- the tower: embed_cls on both routes and the default ---------------------------------------------------------------
@pytest.fixture(scope="module")
def oracles():
    """{name: (emulating oracle, fp32 oracle)}, computed once"""
    out = {}
    for t in TOWERS:
        sd, rgb = tower_case(t)
        x = rgb.permute(0, 3, 1, 2).contiguous()
        out[t["name"]] = tuple(ovit.vit_embedder(x, sd, heads=t["heads"], drop_last=1, class_emb_only=True, emulate_bf16=e).float()
                               for e in (True, False))
    sd, rgb = golden_case()
    x = rgb.permute(0, 3, 1, 2).contiguous()
    out["golden_b32"] = tuple(ovit.vit_embedder(x, sd, heads=12, drop_last=1, class_emb_only=True, emulate_bf16=e).float()
                              for e in (True, False))
    return out


@pytest.fixture(scope="module")
def routes(tmp_path_factory):
    """{switch: {name: embedding}} from one child process per setting of EC_VIT_CLS_TAIL (None: unset, the library's rule)"""
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_vit_cls_route_check.py")
    got = {}
    for sw in ("1", "0", None):
        path = str(tmp_path_factory.mktemp("cls") / ("route_%s.pt" % sw))
        p = GPU.run([sys.executable, script, path], drop=("EC_VIT_CLS_TAIL",), env={} if sw is None else {"EC_VIT_CLS_TAIL": sw}, limit=300)
        assert p.returncode == 0, (sw, p.stderr[-2000:])
        got[sw] = torch.load(path)
    return got


@pytest.mark.parametrize("sw", ["1", "0", None], ids=["cls_tail", "general", "default"])
@pytest.mark.parametrize("name", [t["name"] for t in TOWERS] + ["golden_b32"])
def test_embed_cls_matches_the_oracle(routes, oracles, name, sw):
    got = routes[sw][name]
    emul, full = oracles[name]
    assert got.shape == full.shape and got.dtype == torch.float32
    assert torch.equal(got, got.to(torch.bfloat16).float()), "bf16 values in fp32, as to_f32(..., class_emb_only=True) delivers"
    e, f, o = _rel(got, emul), _rel(got, full), _rel(emul, full)
    print(f"embed_cls {name} EC_VIT_CLS_TAIL={sw}: rel-L2 vs emulating oracle {e:.2e}, vs fp32 oracle {f:.2e} (oracle vs oracle {o:.2e})")
    assert e < 1e-2, e
    assert f < 3e-2, f


def test_the_two_routes_are_different_code_and_agree(routes):
    """the forced routes are not one route twice (some value differs in the last bf16 place somewhere) and agree to bf16 accuracy"""
    differs = False
    for name in routes["1"]:
        a, b = routes["1"][name], routes["0"][name]
        differs = differs or not torch.equal(a, b)
        r = _rel(a, b)
        print(f"embed_cls {name}: CLS tail vs general route rel-L2 {r:.2e}")
        assert r < 1e-2, (name, r)
        assert torch.equal(routes[None][name], a) or torch.equal(routes[None][name], b), name      # the default is one of the two
    assert differs

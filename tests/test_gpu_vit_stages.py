"""GPU: every transformer tower stage ALONE, through its stage entry point (the towers' own launch code), against the float64
references and element-wise bounds of tests/_vit_stage_ref.py -- no margin on top of the derived bounds (the CPU suite checks
that those bounds bite: tests/test_vit_stage_ref.py).  Each test prints its worst |error| / bound before it asserts.

Measured worst |error| / bound on an MI355X (every case under 1, so no bound carries a margin):
  ec_mha_bf16            MFMA core 0.70 (D = 768: 0.69), general core 0.71 non-causal, 0.77 causal
  attnpool core          0.45 (2, 64, 65, 1024 tokens)
  ec_layernorm_bf16      0.996  (the one bf16 rounding of the result is the whole budget: 2^-8 |ref| is attained)
  ec_vit_assemble_bf16   0.992; its records: sum 0.001, M2 0.08
  ec_row_stats_bf16      sum 0.05, M2 0.12
  ec_ln_fold_bf16        Wg bit-equal; s 0.03, c 0.07
  ec_gemm_bf16_ln        producer 0.995, its records sum 0.09 / M2 0.25, consumer 0.985 (default and EC_VIT_BM192=0), 0.974
                         (EC_VIT_WIDE=2); the same figures when the consumer reads ec_row_stats_bf16 records"""
import json
import os
import sys

import pytest
import torch

import _vit_stage_ref as R
from _child import GPU, last_json
from _guard import SENT16 as SENT
from embodied_clip_amd import _lib
from embodied_clip_amd import synthetic as syn

pytestmark = pytest.mark.gpu

SHAPE = -2
PAD = 8                    # rows behind every output that must keep the sentinel


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _out_rows(rows, D, dev):
    return torch.full((rows + PAD, D), SENT, dtype=torch.int16, device=dev)


def _read(out, rows):
    """-> the bf16 rows the kernel wrote, and whether everything behind them still is the sentinel"""
    o = out.cpu()
    return o[:rows].view(torch.bfloat16), bool((o[rows:] == SENT).all())


def _run_mha(lib, dev, qkv, B, L, D, heads, causal):
    out = _out_rows(B * L, D, dev)
    d = qkv.to(dev)
    _lib.check(lib.ec_mha_bf16(d.data_ptr(), out.data_ptr(), B, L, D, heads, int(causal), _lib.stream_ptr()), "ec_mha_bf16")
    torch.cuda.synchronize()
    return _read(out, B * L)


@pytest.mark.parametrize("L,causal,family", R.MHA_CASES, ids=lambda v: str(v))
def test_mha_against_float64(lib, dev, L, causal, family):
    """ec_mha_bf16 at B = 3, heads = 2, D = 128: the MFMA core (non-causal, L <= 64: one or two key / query fragments, with and
    without padding) and the general core (the 64-key chunk edges, the limit of 512 tokens, causal with a dominant diagonal and
    with queries that ask for the first forbidden key)."""
    B, D, heads = 3, 128, 2
    qkv = R.attention_inputs(family, B, L, D, heads)
    ref, bound, _ = R.attention_ref(qkv, B, L, D, heads, causal)
    got, pad_ok = _run_mha(lib, dev, qkv, B, L, D, heads, causal)
    r = R.worst_ratio(got, ref, bound)
    print(f"ratio ec_mha_bf16 L={L} causal={causal} {family}: {r:.3f}")
    assert pad_ok, "rows past B * L were written"
    assert r <= 1.0, r


def test_mha_vit_b32_width(lib, dev):
    """D = 768, 12 heads, 50 tokens: the head stride of the product geometry."""
    c = R.MHA_WIDE_CASE
    args = (c["B"], c["L"], c["D"], c["heads"])
    qkv = R.attention_inputs(c["family"], *args)
    ref, bound, _ = R.attention_ref(qkv, *args, c["causal"])
    got, pad_ok = _run_mha(lib, dev, qkv, *args, c["causal"])
    r = R.worst_ratio(got, ref, bound)
    print(f"ratio ec_mha_bf16 D=768 heads=12 L=50: {r:.3f}")
    assert pad_ok and r <= 1.0, (pad_ok, r)


def test_mha_refuses_what_no_core_handles(lib, dev):
    buf = torch.zeros(3 * 513 * 3 * 128, dtype=torch.int16, device=dev)
    out = _out_rows(3 * 513, 128, dev)
    for causal in (0, 1):
        assert lib.ec_mha_bf16(buf.data_ptr(), out.data_ptr(), 3, 513, 128, 2, causal, _lib.stream_ptr()) == SHAPE
    assert lib.ec_mha_bf16(buf.data_ptr(), out.data_ptr(), 3, 50, 128, 4, 0, _lib.stream_ptr()) == SHAPE      # D / heads = 32
    torch.cuda.synchronize()
    assert bool((out == SENT).all())


@pytest.mark.parametrize("D", R.LN_DIMS)
def test_layernorm_against_float64(lib, dev, D):
    """ec_layernorm_bf16 (layernorm_kernel<0>): D = 64, 192, 768 take the strided path, 256 and 1024 the vector path; 1..5 rows
    cover a partly filled and a second workgroup; plain, mean-dominated, near-constant rows and a spread gamma."""
    worst = 0.0
    for rows in R.LN_ROWS:
        for family in R.LN_FAMILIES:
            x, gamma, beta = R.layernorm_inputs(family, rows, D)
            ref, bound = R.layernorm_ref(x.to(R.F64), gamma, beta)
            out = _out_rows(rows, D, dev)
            dx, dg, db = x.to(dev), gamma.to(dev), beta.to(dev)
            _lib.check(lib.ec_layernorm_bf16(dx.data_ptr(), dg.data_ptr(), db.data_ptr(), out.data_ptr(), rows, D, _lib.stream_ptr()),
                       "ec_layernorm_bf16")
            torch.cuda.synchronize()
            got, pad_ok = _read(out, rows)
            r = R.worst_ratio(got, ref, bound)
            print(f"ratio ec_layernorm_bf16 D={D} rows={rows} {family}: {r:.3f}")
            assert pad_ok, (rows, family)
            assert r <= 1.0, (rows, family, r)
            worst = max(worst, r)
    print(f"worst ec_layernorm_bf16 D={D}: {worst:.3f}")


def _check_records(rec, y_bf16, D, what):
    (s, m2, n), (bs, bm) = R.record_ref(y_bf16.to(R.F64), R.ln_depth(D))
    rs, rm = R.worst_ratio(rec[:, 0], s, bs), R.worst_ratio(rec[:, 1], m2, bm)
    print(f"ratio {what} record sum {rs:.3f} M2 {rm:.3f}")
    assert bool((rec[:, 2] == n).all()) and bool((rec[:, 3] == 0).all()), what
    assert rs <= 1.0 and rm <= 1.0, (what, rs, rm)


@pytest.mark.parametrize("B,L,D", R.ASSEMBLE_SHAPES)
@pytest.mark.parametrize("with_records", (False, True))
def test_assemble_against_float64(lib, dev, B, L, D, with_records):
    """ec_vit_assemble_bf16 (layernorm_kernel<1>): class token / patch rows + positional embedding + ln_pre, and the record of the
    ROUNDED output row."""
    pemb, cls, pos, gamma, beta = R.assemble_inputs(B, L, D)
    v64, _, v_err = R.assemble_rows(pemb, cls, pos, B, L, D)
    ref, bound = R.layernorm_ref(v64, gamma, beta, v_err=v_err)
    rows = B * L
    out = _out_rows(rows, D, dev)
    stats = torch.full((rows + PAD, 4), -7.0, dtype=torch.float32, device=dev)
    d = [t.to(dev) for t in (pemb, cls, pos, gamma, beta)]
    _lib.check(lib.ec_vit_assemble_bf16(*[t.data_ptr() for t in d], out.data_ptr(), stats.data_ptr() if with_records else None,
                                        B, L, D, _lib.stream_ptr()), "ec_vit_assemble_bf16")
    torch.cuda.synchronize()
    got, pad_ok = _read(out, rows)
    r = R.worst_ratio(got, ref, bound)
    print(f"ratio ec_vit_assemble_bf16 {(B, L, D)} records={with_records}: {r:.3f}")
    assert pad_ok and r <= 1.0, (pad_ok, r)
    st = stats.cpu()
    if with_records:
        _check_records(st[:rows], got, D, f"ec_vit_assemble_bf16 {(B, L, D)}")
        assert bool((st[rows:] == -7.0).all())
    else:
        assert bool((st == -7.0).all())


@pytest.mark.parametrize("B,L,D", R.ASSEMBLE_SHAPES)
def test_row_stats_against_float64(lib, dev, B, L, D):
    rows = B * L
    x = R.residual_stream("mean_dominated", rows, D) if D % 128 == 0 else R.layernorm_inputs("mean_dominated", rows, D)[0]
    stats = torch.full((rows + PAD, 4), -7.0, dtype=torch.float32, device=dev)
    dx = x.to(dev)
    _lib.check(lib.ec_row_stats_bf16(dx.data_ptr(), stats.data_ptr(), rows, D, _lib.stream_ptr()), "ec_row_stats_bf16")
    torch.cuda.synchronize()
    st = stats.cpu()
    _check_records(st[:rows], x, D, f"ec_row_stats_bf16 {(rows, D)}")
    assert bool((st[rows:] == -7.0).all())


@pytest.mark.parametrize("N,K", R.FOLD_SHAPES)
def test_ln_fold_against_float64(lib, dev, N, K):
    """ec_ln_fold_bf16: Wg bit-equal to bf16(fp32(W) gamma), s over the ROUNDED Wg, c = beta . W + b."""
    W, gamma, beta, b = R.fold_inputs(N, K)
    Wg_ref, (s, bs), (c, bc) = R.fold_ref(W, gamma, beta, b)
    Wg = torch.full((N + PAD, K), SENT, dtype=torch.int16, device=dev)
    sv = torch.full((N + PAD,), -7.0, device=dev)
    cv = torch.full((N + PAD,), -7.0, device=dev)
    d = [t.to(dev) for t in (W, gamma, beta, b)]
    _lib.check(lib.ec_ln_fold_bf16(*[t.data_ptr() for t in d], Wg.data_ptr(), sv.data_ptr(), cv.data_ptr(), N, K, _lib.stream_ptr()),
               "ec_ln_fold_bf16")
    torch.cuda.synchronize()
    got, pad_ok = _read(Wg, N)
    assert pad_ok and torch.equal(got.view(torch.int16), Wg_ref.view(torch.int16))
    sv, cv = sv.cpu(), cv.cpu()
    rs, rc = R.worst_ratio(sv[:N], s, bs), R.worst_ratio(cv[:N], c, bc)
    print(f"ratio ec_ln_fold_bf16 {(N, K)} s {rs:.3f} c {rc:.3f}")
    assert rs <= 1.0 and rc <= 1.0, (rs, rc)
    assert bool((sv[N:] == -7.0).all()) and bool((cv[N:] == -7.0).all())


@pytest.mark.parametrize("setting", list(R.GEMM_SETTINGS))
def test_gemm_ln_chain_in_a_child_process(setting):
    """ec_gemm_bf16_ln, producer -> consumer, per tile setting (read once per process, hence the child): default (128-wide tiles of
    192 rows), EC_VIT_BM192=0 (128 x 256), EC_VIT_WIDE=2 (256-wide: records of count 256).  np = 1, 3, 6, 8 (2, 3, 4 wide)."""
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_vit_gemm_ln_check.py")
    p = GPU.run([sys.executable, script, setting], drop=("EC_VIT_BM192", "EC_VIT_WIDE"), env=R.GEMM_SETTINGS[setting], limit=300)
    assert p.returncode == 0, p.stderr[-2000:]
    res = last_json(p)
    assert res["setting"] == setting and len(res["cases"]) == len(R.gemm_cases(setting))
    worst = {}
    for c in res["cases"]:
        print("ratio ec_gemm_bf16_ln", setting, json.dumps(c))
        assert c["np_out"] == R.gemm_expected_np(setting, c["D"]), c
        assert c["pad_ok"] and c["rec_exact"], c
        for k in ("producer", "rec_sum", "rec_m2", "consumer", "consumer_row_stats"):
            worst[k] = max(worst.get(k, 0.0), c[k])
            assert c[k] <= 1.0, (k, c)
    print("worst ec_gemm_bf16_ln", setting, json.dumps(worst))


def _attnpool_sd(HW, C, out_dim, sharp):
    n = lambda seed, *shape: torch.from_numpy(syn.hash_normal(seed, int(torch.tensor(shape).prod()))).float().reshape(*shape)
    sd = {"attnpool.positional_embedding": n(1, HW + 1, C) * C ** -0.5}
    for i, name in enumerate(("q_proj", "k_proj", "v_proj")):
        sd[f"attnpool.{name}.weight"] = n(10 + i, C, C) * C ** -0.5 * (sharp if name != "v_proj" else 1.0)
        sd[f"attnpool.{name}.bias"] = n(20 + i, C) * 0.1
    sd["attnpool.c_proj.weight"] = n(30, out_dim, C) * C ** -0.5
    sd["attnpool.c_proj.bias"] = n(31, out_dim) * 0.1
    return sd, n


@pytest.mark.parametrize("HW", (1, 63, 64, 1023))
def test_attnpool_core_token_counts(dev, HW):
    """ec_attnpool_forward at 2, 64, 65 and ATTNPOOL_MAX_L = 1024 tokens (C = 128, 2 heads, out_dim 64, batch 2): the CLS-query
    core is read out of the call's workspace (q, k | v in, att out: the layout ec_attnpool_workspace_bytes sums up) and held to
    the attention bound; the whole call to the oracle at the existing tolerance.  q / k projections x 3: a sharper softmax."""
    from embodied_clip_amd.encoder import AttentionPool
    from oracle import clip_resnet as ocr
    B, C, heads, out_dim, Lt = 2, 128, 2, 64, HW + 1
    sd, n = _attnpool_sd(HW, C, out_dim, 3.0)
    feat = (n(40, B, HW, 1, C).abs() * 0.7).to(torch.bfloat16)
    pool = AttentionPool(sd, device=dev, num_heads=heads)
    out = pool.forward(feat.to(dev)).cpu()
    ws = pool._ws.cpu()
    al = lambda v: (v + 255) // 256 * 256
    off = al(B * Lt * C * 2) + al(B * C * 2)
    kv = ws[off:off + B * Lt * 2 * C * 2].view(torch.bfloat16).reshape(B, Lt, 2, heads, 64).to(R.F64)
    off += al(B * Lt * 2 * C * 2)
    q = ws[off:off + B * C * 2].view(torch.bfloat16).reshape(B, heads, 64).to(R.F64)
    off += al(B * C * 2)
    att = ws[off:off + B * C * 2].view(torch.bfloat16).reshape(B, heads, 64)
    k, v = kv[:, :, 0].permute(0, 2, 1, 3), kv[:, :, 1].permute(0, 2, 1, 3)          # [B, heads, Lt, 64]
    p = torch.softmax((k @ q[..., None])[..., 0] * R.ATT_SCALE, dim=-1)               # [B, heads, Lt]
    ref = (p[..., None] * v).sum(2)
    bound = 1.05 * 2.0 ** -7 * (p[..., None] * v.abs()).sum(2)
    r = R.worst_ratio(att, ref, bound)
    print(f"ratio attnpool_core tokens={Lt}: {r:.3f} (largest p {float(p.max()):.3f})")
    assert r <= 1.0, r
    full = ocr.attnpool(feat.float().reshape(B, HW, 1, C).permute(0, 3, 1, 2).contiguous(), sd, num_heads=heads)
    rel = float((out - full).norm() / full.norm())
    assert out.shape == full.shape == (B, out_dim) and rel < 1.5e-2, rel


def test_attnpool_refuses_1025_tokens(dev, lib):
    from embodied_clip_amd.encoder import AttentionPool
    sd, n = _attnpool_sd(1024, 128, 64, 1.0)
    pool = AttentionPool(sd, device=dev, num_heads=2)
    with pytest.raises(_lib.EcError, match="shape"):
        pool.forward(torch.zeros(2, 1024, 1, 128, dtype=torch.bfloat16, device=dev))


def test_unfolded_tower_width_192(dev):
    """A width-192 tower (3 heads, 3 blocks): D % 128 != 0, so no LayerNorm fold is built and run_blocks takes the LayerNorm
    launches -- the first test of that branch.  Tolerances of test_mha_core_and_layernorm_small_vit."""
    from embodied_clip_amd.encoder import ViTEmbedder
    from oracle import clip_vit as ovit
    sd = syn.vit_visual_state_dict(9, width=192, layers=4, heads=3, patch_size=32, input_resolution=224, output_dim=64)
    rgb = syn.synthetic_rgb(79, 3)
    vit = ViTEmbedder(sd, device=dev, heads=3)
    tok = vit.to_f32(vit.forward(rgb.to(dev))).cpu()
    x = rgb.permute(0, 3, 1, 2)
    ref = ovit.vit_embedder(x, sd, heads=3, drop_last=1)
    ref_emul = ovit.vit_embedder(x, sd, heads=3, drop_last=1, emulate_bf16=True)
    rel = lambda a, b: float((a - b).norm() / b.norm())
    assert tok.shape == ref.shape == (3, 50, 192)
    print(f"unfolded tower width 192: rel-L2 {rel(tok, ref_emul):.2e} emulated, {rel(tok, ref):.2e} fp32")
    assert rel(tok, ref_emul) < 1e-2, rel(tok, ref_emul)
    assert rel(tok, ref) < 3e-2, rel(tok, ref)

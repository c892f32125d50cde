"""Float64 references, element-wise error bounds, fp32/bf16 emulations and named wrong versions of the tile kernels of
conv_igemm.hip (conv_igemm_kernel: 4 / 8 waves; conv_igemm8_kernel: 8 waves, ping-pong), and the list of cases that reaches every
registered instance of the two through the public entry points.  CPU only.  tests/test_conv_tile_ref.py checks here, without a
GPU, that every case launches the instance it names, that the instances named are all but the exempt ones, and that the bounds
bite on reduced cases (fewer frames): the emulation of the kernel's arithmetic stays under them and each wrong version exceeds
them at least 4 x somewhere.  tests/test_gpu_conv_tiles.py then holds the kernels to the same bounds on the full cases.

Every reference takes the SAME bf16 (and fp32) operands the kernel gets and works in float64: the implicit-GEMM matrix A (one row
per kernel row m, K = (ky, kx, ci), zeros outside the frame) times W^T.

Number formats: bf16 keeps 8 significant bits, so round-to-nearest has unit roundoff UB = 2^-8; fp32 has U = 2^-24.

Bound of one output element, z = sum_k a_k w_k + bias (+ res) before the activation:
  * products: bf16 x bf16 has 16 significant bits, exact in fp32.
  * accumulation: both kernels keep ONE fp32 accumulator per output element for the whole K walk and feed it a chain of
    ceil(K / 64) * 4 v_mfma_f32_32x32x16_bf16 steps (K-tiles of 64 in order, four k-steps of 16 each; K is padded with zeros to a
    multiple of 64; the three-plane GEMM walks every K-tile once per plane: 3 K terms).  Each step adds 16 products to the
    accumulator; the order inside a step is not documented, so a step is charged as 16 sequential fp32 additions.  That makes
    c(K) = 64 ceil(K / 64) additions in all -- which is also what ANY summation order of that many terms is bounded by -- plus
    one for the bias and one for the residual:
        e = (c(K) + 2) U (sum_k |a_k w_k| + |bias| + |res|)                 (first order)
  * activation: none and ReLU have Lipschitz constant 1, QuickGELU z sigmoid(1.702 z) 1.1.  QuickGELU is computed as
    z * rcp(1 + exp2(-1.702 z log2 e)) with v_exp / v_rcp (1 ulp = 2 U relative each): the two products in the exponent move
    exp by 2 * 1.702 |z| U relative, v_exp by 2 U; t / (1 + t) = 1 - s of that reaches the sigmoid s, plus U for the addition, 2 U
    for v_rcp and U for the last product:
        g = U |ref| ((1 - s) (3.404 |z| + 2) + 4)
  * pooled epilogue (ReLU whatever `act` says, then the quad add): v_i = relu(z_i) of the window's four pixels are added in two
    DPP steps (depth 2) and scaled by 0.25 (exact):  fp = 0.25 (sum_i e_i + 2 U sum_i v_i).
  * ONE rounding of the result to bf16: UB (|ref| + fp).  (The three-plane GEMM writes fp32: U (|ref| + fp).)
  bound = 1.05 * (UB (|ref| + fp) + fp), fp = e | 1.1 e + g | the pooled fp:  5 % on top, as in _vit_stage_ref.py.
"""
import zlib

import torch

from _bounds import F64, U, UB, bf16, randn as _randn, worst_ratio  # noqa: F401  (re-exported for the checks)

ACT_NONE, ACT_RELU, ACT_QUICKGELU = 0, 1, 2
CHUNK = 8192               # rows of A formed at a time

C8 = "conv_igemm8_kernel<%s>"      # <BN, KS, POOL, ABL, X3, S2, BM, XP>
C4 = "conv_igemm_kernel<%s>"       # <BM, BN, WM, WN, KS, POOL, PF, MV, NS, ILV, S2>

# The library reads its switches once per process: one recorder / GPU child process per setting.  EC_CONV_BIG=4 takes the 8-wave
# stride-1 kernels from 8,192 rows on (and leaves everything smaller, or with Cin % 64 != 0 or K < 512, to the 4-wave tiles);
# EC_CONV_T224=1 takes the 224-row tile wherever M % 196 == 0; `b` turns the long segments and the ring off.
SETTINGS = {
    "a": {"EC_CONV_BIG": "4", "EC_CONV_T224": "1"},
    "b": {"EC_CONV_BIG": "4", "EC_CONV8_LONGSEG": "0", "EC_CONV_RING": "0"},
}
SWITCHES = ("EC_CONV_BIG", "EC_CONV8_MIN_TILES", "EC_CONV8_BN128", "EC_CONV8_LONGSEG", "EC_CONV_T224", "EC_CONV_T64", "EC_CONV_RING",
            "EC_CONV_REGW", "EC_VIT_WIDE", "EC_VIT_BM192")

# conv_igemm instances no case below can reach: instance -> the test that covers it
EXEMPT = {
    C8 % "128, 1, false, 512, false, false, 192, 3": "tests/test_gpu_vit_stages.py::test_gemm_ln_chain_in_a_child_process[default]",
    C8 % "128, 1, false, 0, false, false, 192, 3": "tests/test_gpu_vit_stages.py::test_gemm_ln_chain_in_a_child_process (ec_gemm_bf16_ln only)",
    C8 % "128, 1, false, 512, true, false, 256, 2": "tests/test_gpu_policy.py::test_learn_pass_policy_gemm_modes_match_oracle_at_pingpong_size",
    C8 % "128, 1, false, 0, true, false, 256, 2": "tests/test_gpu_policy.py::test_learn_pass_policy_gemm_modes_match_oracle_at_pingpong_size",
}

# (setting, command, instance, input family).  conv: B H W Cin Cout ks pool act res ldo; s2: B H W Cin Cout ks act res;
# gemm: M N K act res; x3: M N K act (tools/launch_log.cpp).  Families: "zm" zero-mean activations, "pos" non-negative ones (post-ReLU,
# as the trunk produces) against weights with a positive mean, so that the sums do not cancel.
# Shapes: 43 frames of 14 x 14 are 8,428 rows = 32 tiles of 256 + 236 rows, every tile straddling frames; 3 x 14 x 14 = 588 = 3 x 196;
# 16 x 18 is the non-square map; Cin = 32 splits a tap inside a K-tile, Cin = 192 is no power of two; K = 520 and 200 are no
# multiples of 64.  The stride-2 8-wave rules want 150 tiles of 256 rows: 195 frames of 28 x 28 give 38,220 rows = 149 tiles + 76 rows.
CASES = [
    # ---- setting a: 8-wave, stride 1 (wide, and narrow with long segments)
    ("a", "conv 43 14 14 64 256 3 0 1 0 0", C8 % "256, 3, false, 0, false, false, 256, 3", "pos"),
    ("a", "conv 43 14 14 64 256 3 1 1 0 0", C8 % "256, 3, true, 0, false, false, 256, 3", "zm"),
    ("a", "conv 43 14 14 64 128 3 0 0 1 0", C8 % "128, 3, false, 512, false, false, 256, 3", "zm"),
    ("a", "conv 43 14 14 64 128 3 1 1 0 200", C8 % "128, 3, true, 512, false, false, 256, 3", "pos"),
    ("a", "gemm 8428 256 512 2 0", C8 % "256, 1, false, 0, false, false, 256, 3", "zm"),
    ("a", "conv 11 28 28 512 256 1 1 1 0 0", C8 % "256, 1, true, 0, false, false, 256, 3", "pos"),
    ("a", "gemm 8428 128 512 1 1", C8 % "128, 1, false, 512, false, false, 256, 3", "pos"),
    ("a", "conv 11 28 28 512 128 1 1 1 0 0", C8 % "128, 1, true, 512, false, false, 256, 3", "zm"),
    ("a", "x3 300 128 256 1", C8 % "128, 1, false, 512, true, false, 256, 3", "pos"),
    # ---- setting a: 8-wave, stride 2
    ("a", "s2 195 28 28 64 256 3 1 0", C8 % "256, 3, false, 0, false, true, 256, 3", "pos"),
    ("a", "s2 195 28 28 512 256 1 0 1", C8 % "256, 1, false, 0, false, true, 256, 3", "zm"),
    ("a", "s2 195 28 28 64 128 3 1 1", C8 % "128, 3, false, 512, false, true, 256, 3", "zm"),
    ("a", "s2 195 28 28 512 128 1 0 0", C8 % "128, 1, false, 512, false, true, 256, 3", "pos"),
    # ---- setting a: 4-wave kernel, 224-row tiles (196 real rows)
    ("a", "conv 3 14 14 192 256 3 0 1 0 0", C4 % "224, 128, 1, 4, 3, false, false, 196, 0, false, false", "pos"),
    ("a", "gemm 392 128 520 0 1", C4 % "224, 128, 1, 4, 1, false, false, 196, 0, false, false", "zm"),
    # ---- 64 x 64 ring tiles
    ("a", "conv 5 7 7 128 128 3 0 1 1 0", C4 % "64, 64, 2, 2, 3, false, false, 64, 4, true, false", "pos"),
    ("a", "gemm 300 128 520 2 0", C4 % "64, 64, 2, 2, 1, false, false, 64, 4, true, false", "zm"),
    # ---- 128 x 128 tiles: single stage (K < 512), residual prefetch, ring on 8 waves
    ("a", "conv 3 16 18 32 128 3 0 0 0 0", C4 % "128, 128, 2, 2, 3, false, false, 128, 0, false, false", "zm"),
    ("a", "conv 3 14 14 32 128 3 1 1 0 0", C4 % "128, 128, 2, 2, 3, true, false, 128, 0, false, false", "pos"),
    ("a", "gemm 300 128 200 2 0", C4 % "128, 128, 2, 2, 1, false, false, 128, 0, false, false", "zm"),
    ("a", "conv 3 14 14 64 128 1 1 1 0 0", C4 % "128, 128, 2, 2, 1, true, false, 128, 0, false, false", "pos"),
    ("a", "gemm 300 128 200 1 1", C4 % "128, 128, 2, 2, 1, false, true, 128, 0, false, false", "pos"),
    ("a", "gemm 300 256 136 0 1", C4 % "128, 128, 2, 2, 1, false, true, 128, 0, false, false", "zm"),
    ("a", "conv 17 16 18 64 512 3 0 1 0 0", C4 % "128, 128, 2, 4, 3, false, false, 128, 3, true, false", "pos"),
    ("a", "gemm 4890 512 520 0 1", C4 % "128, 128, 2, 4, 1, false, false, 128, 3, true, false", "zm"),
    ("a", "conv 3 14 14 64 128 3 1 1 0 0", C4 % "128, 128, 2, 4, 3, true, false, 128, 3, true, false", "zm"),
    ("a", "conv 3 14 14 512 128 1 1 1 0 0", C4 % "128, 128, 2, 4, 1, true, false, 128, 3, true, false", "pos"),
    # ---- 256 x 64 and 256 x 32 tiles
    ("a", "conv 3 16 18 128 64 3 0 1 0 104", C4 % "256, 64, 4, 1, 3, false, false, 256, 0, false, false", "pos"),
    ("a", "conv 3 16 18 128 64 3 1 1 0 0", C4 % "256, 64, 4, 1, 3, true, false, 256, 0, false, false", "zm"),
    ("a", "gemm 700 64 200 1 1", C4 % "256, 64, 4, 1, 1, false, false, 256, 0, false, false", "zm"),
    ("a", "conv 3 14 14 128 64 1 1 1 0 0", C4 % "256, 64, 4, 1, 1, true, false, 256, 0, false, false", "pos"),
    ("a", "conv 3 16 18 128 32 3 0 0 1 0", C4 % "256, 32, 4, 1, 3, false, false, 256, 0, false, false", "zm"),
    ("a", "conv 3 14 14 128 32 3 1 1 0 0", C4 % "256, 32, 4, 1, 3, true, false, 256, 0, false, false", "pos"),
    ("a", "gemm 700 32 200 2 0", C4 % "256, 32, 4, 1, 1, false, false, 256, 0, false, false", "zm"),
    ("a", "conv 3 14 14 128 32 1 1 1 0 0", C4 % "256, 32, 4, 1, 1, true, false, 256, 0, false, false", "zm"),
    # ---- 4-wave kernel, stride 2
    ("a", "s2 3 28 28 64 128 3 1 0", C4 % "64, 64, 2, 2, 3, false, false, 64, 4, false, true", "pos"),
    ("a", "s2 3 28 28 512 128 1 0 1", C4 % "64, 64, 2, 2, 1, false, false, 64, 4, false, true", "zm"),
    ("a", "s2 17 32 36 64 512 3 0 1", C4 % "128, 128, 2, 4, 3, false, false, 128, 3, true, true", "zm"),
    ("a", "s2 17 32 36 512 512 1 1 0", C4 % "128, 128, 2, 4, 1, false, false, 128, 3, true, true", "pos"),
    ("a", "s2 3 28 28 32 128 3 1 0", C4 % "128, 128, 2, 2, 3, false, false, 128, 0, false, true", "pos"),
    ("a", "s2 3 28 28 64 128 1 1 1", C4 % "128, 128, 2, 2, 1, false, false, 128, 0, false, true", "zm"),
    ("a", "s2 5 28 28 64 64 3 1 1", C4 % "256, 64, 4, 1, 3, false, false, 256, 0, false, true", "zm"),
    ("a", "s2 5 28 36 64 64 1 0 0", C4 % "256, 64, 4, 1, 1, false, false, 256, 0, false, true", "pos"),
    # ---- setting b: 8-wave narrow tiles without long segments, the 64 x 64 single-stage loop
    ("b", "conv 43 14 14 64 128 3 0 1 1 0", C8 % "128, 3, false, 0, false, false, 256, 3", "pos"),
    ("b", "conv 43 14 14 64 128 3 1 1 0 0", C8 % "128, 3, true, 0, false, false, 256, 3", "zm"),
    ("b", "gemm 8428 128 512 2 0", C8 % "128, 1, false, 0, false, false, 256, 3", "zm"),
    ("b", "conv 11 28 28 512 128 1 1 1 0 0", C8 % "128, 1, true, 0, false, false, 256, 3", "pos"),
    ("b", "x3 300 128 256 0", C8 % "128, 1, false, 0, true, false, 256, 3", "zm"),
    ("b", "s2 195 28 28 64 128 3 0 1", C8 % "128, 3, false, 0, false, true, 256, 3", "pos"),
    ("b", "s2 195 28 28 512 128 1 1 0", C8 % "128, 1, false, 0, false, true, 256, 3", "zm"),
    ("b", "conv 5 7 7 128 128 3 0 0 1 0", C4 % "64, 64, 2, 2, 3, false, false, 64, 0, false, false", "zm"),
    ("b", "gemm 300 128 520 1 1", C4 % "64, 64, 2, 2, 1, false, false, 64, 0, false, false", "pos"),
]
CASES = [dict(setting=s, cmd=c, instance=i, family=f) for s, c, i, f in CASES]


def cases_of(setting):
    return [c for c in CASES if c["setting"] == setting]


def shape(case):
    """The command's numbers by name, the kernel rows M (before pooling), the output rows and the tile (rows MV, columns BN) of the
    case's instance."""
    f = case["cmd"].split()
    v = [int(t) for t in f[1:]]
    d = dict(kind=f[0], pool=0, res=0, ldo=0, s2=f[0] == "s2", x3=f[0] == "x3")
    if f[0] == "conv":
        d.update(zip(("B", "H", "W", "Cin", "Cout", "ks", "pool", "act", "res", "ldo"), v))
    elif f[0] == "s2":
        d.update(zip(("B", "H", "W", "Cin", "Cout", "ks", "act", "res"), v))
    elif f[0] == "gemm":
        d.update(B=1, H=1, W=v[0], Cout=v[1], Cin=v[2], ks=1, act=v[3], res=v[4])
    elif f[0] == "x3":
        d.update(B=1, H=1, W=v[0], Cout=v[1], Cin=v[2], ks=1, act=v[3])
    else:
        raise KeyError(f[0])
    d["K"] = d["ks"] ** 2 * d["Cin"]
    d["M"] = d["B"] * (d["H"] // 2) * (d["W"] // 2) if d["s2"] else d["B"] * d["H"] * d["W"]
    d["rows"] = d["M"] // 4 if d["pool"] else d["M"]
    d["ldo"] = d["ldo"] or d["Cout"]
    name, args = case["instance"].split("<")
    t = [a.strip() for a in args.rstrip(">").split(",")]
    d["MV"], d["BN"] = (int(t[6]), int(t[0])) if name == "conv_igemm8_kernel" else (int(t[7]), int(t[1]))
    d["tile_rows"] = d["MV"] // 4 if d["pool"] else d["MV"]         # output rows of one tile
    return d


def reduced(case):
    """The same case with fewer frames (conv, s2: at most 3; GEMMs: two 256-row tiles and the ragged rest): same generator, same
    bound formula, a size the CPU checks afford."""
    f = case["cmd"].split()
    if f[0] in ("conv", "s2"):
        f[1] = str(min(int(f[1]), 3))
    else:
        M = int(f[1])
        f[1] = str(M if M <= 768 else 512 + (M % 256 or 76))
    return dict(case, cmd=" ".join(f))


def operands(case):
    """-> dict: x bf16 [B, H, W, Cin]; w bf16 [Cout, K] (x3: [Cout, 3, K], three planes of an fp32 matrix, leading plane first);
    bias fp32 [Cout]; res bf16 [M, Cout] or None.  Seeded by the command."""
    d = shape(case)
    s = zlib.crc32(case["cmd"].encode())
    x = _randn(s, d["B"], d["H"], d["W"], d["Cin"])
    w = _randn(s + 1, d["Cout"], d["K"]) * d["K"] ** -0.5
    if case["family"] == "pos":
        x = 0.7 * x.abs()
        w = w + 0.05 * d["K"] ** -0.5
    elif case["family"] != "zm":
        raise KeyError(case["family"])
    bias = 0.5 * _randn(s + 2, d["Cout"])
    res = _randn(s + 3, d["M"], d["Cout"]).to(torch.bfloat16) if d["res"] else None
    if d["x3"]:
        p0 = bf16(w)
        p1 = bf16(w - p0)
        p2 = bf16(w - p0 - p1)
        wq = torch.stack([p0, p1, p2], 1).to(torch.bfloat16).contiguous()
    else:
        wq = w.to(torch.bfloat16).contiguous()
    return dict(x=x.to(torch.bfloat16).contiguous(), w=wq, bias=bias.contiguous(), res=res)


def _pixels(d, odd=False, raster=False):
    """(b, y, x) of the centre tap of every kernel row m: raster order; pooled: m = 4 q + 2 dy + dx with q the pooled raster index;
    stride 2: output pixel (yo, xo) reads (2 yo, 2 xo).  odd: (2 yo + 1, 2 xo + 1).  raster: the pooled decode left out."""
    B, H, W = d["B"], d["H"], d["W"]
    if d["s2"]:
        b, yo, xo = torch.meshgrid(torch.arange(B), torch.arange(H // 2), torch.arange(W // 2), indexing="ij")
        o = 1 if odd else 0
        return b.reshape(-1), 2 * yo.reshape(-1) + o, 2 * xo.reshape(-1) + o
    if d["pool"] and not raster:
        b, yp, xp, s = torch.meshgrid(torch.arange(B), torch.arange(H // 2), torch.arange(W // 2), torch.arange(4), indexing="ij")
        return b.reshape(-1), (2 * yp + (s >> 1)).reshape(-1), (2 * xp + (s & 1)).reshape(-1)
    b, y, x = torch.meshgrid(torch.arange(B), torch.arange(H), torch.arange(W), indexing="ij")
    return b.reshape(-1), y.reshape(-1), x.reshape(-1)


def _a_rows(xf, d, pix, lo, hi, dtype, clamp=False, swap=False):
    """Rows lo .. hi of the implicit-GEMM matrix A of xf (bf16 [B, H, W, Cin]) in `dtype`: [hi - lo, K], K = (ky, kx, ci)."""
    b, y, x = (t[lo:hi] for t in pix)
    if d["ks"] == 1:
        return xf[b, y, x].to(dtype)
    cols = []
    for ky in range(3):
        for kx in range(3):
            dy, dx = (kx - 1, ky - 1) if swap else (ky - 1, kx - 1)
            yy, xx = y + dy, x + dx
            ok = (yy >= 0) & (yy < d["H"]) & (xx >= 0) & (xx < d["W"])
            v = xf[b, yy.clamp(0, d["H"] - 1), xx.clamp(0, d["W"] - 1)].to(dtype)
            cols.append(v if clamp else v * ok[:, None].to(dtype))
    return torch.cat(cols, 1)


def _wmat(op, dtype):
    """W as [Cout, K'] (the three planes side by side along K for x3) and how often A repeats along K'."""
    w = op["w"].to(dtype)
    return (w.reshape(w.shape[0], -1), 3) if w.dim() == 3 else (w, 1)


def _products(case, op, dtype=F64, want_abs=False, drop=None, **pix_kw):
    """A W^T [M, Cout] in `dtype`, in chunks of rows; want_abs: also |A| |W|^T.  drop = (row lo, row hi, col hi, k lo): the 64
    products from k lo on left out for those rows and the columns below col hi."""
    d = shape(case)
    xf = op["x"]
    wm, rep = _wmat(op, dtype)
    pix = _pixels(d, odd=pix_kw.pop("odd", False), raster=pix_kw.pop("raster", False))
    M = d["M"]
    z = torch.empty(M, d["Cout"], dtype=dtype)
    s = torch.empty(M, d["Cout"], dtype=dtype) if want_abs else None
    for lo in range(0, M, CHUNK):
        hi = min(M, lo + CHUNK)
        a = _a_rows(xf, d, pix, lo, hi, dtype, **pix_kw)
        if rep > 1:
            a = a.repeat(1, rep)
        z[lo:hi] = a @ wm.T
        if want_abs:
            s[lo:hi] = a.abs() @ wm.abs().T
        if drop is not None:
            r0, r1, c1, k0 = drop
            a0, a1 = max(r0, lo), min(r1, hi)
            if a0 < a1:
                for p in range(rep):
                    ks = slice(p * d["K"] + k0, p * d["K"] + k0 + 64)
                    z[a0:a1, :c1] -= a[a0 - lo:a1 - lo, ks] @ wm[:c1, ks].T
    return z, s


def quickgelu(z, c=1.702):
    return z * torch.sigmoid(c * z)


def _finish(d, z, bias, res, act=None, pool_first=False, gelu_c=1.702):
    """bias, residual, activation (pooled: ReLU and the mean of the four rows of a window) in the dtype of z; no rounding."""
    v = z + bias.to(z.dtype)[None, :]
    if res is not None:
        v = v + res.to(z.dtype)
    if d["pool"]:
        q = v.reshape(-1, 4, v.shape[-1])
        return torch.relu(q.mean(1)) if pool_first else 0.25 * ((torch.relu(q[:, 0]) + torch.relu(q[:, 1])) + (torch.relu(q[:, 2]) + torch.relu(q[:, 3])))
    act = d["act"] if act is None else act
    if act == ACT_RELU:
        return torch.relu(v)
    if act == ACT_QUICKGELU:
        return quickgelu(v, gelu_c)
    return v


def c_of_k(d):
    """fp32 additions charged to one accumulator (module docstring)"""
    return 64 * -(-d["K"] // 64) * (3 if d["x3"] else 1)


def reference(case, op=None):
    """-> ref, bound: float64 [rows, Cout]"""
    d = shape(case)
    op = op or operands(case)
    z, s = _products(case, op, want_abs=True)
    b = op["bias"].to(F64)[None, :]
    r = op["res"].to(F64) if op["res"] is not None else None
    pre = z + b + (r if r is not None else 0.0)
    e = (c_of_k(d) + 2) * U * (s + b.abs() + (r.abs() if r is not None else 0.0))
    ref = _finish(d, z, op["bias"], r)
    if d["pool"]:
        v = torch.relu(pre).reshape(-1, 4, d["Cout"]).sum(1)
        fp = 0.25 * (e.reshape(-1, 4, d["Cout"]).sum(1) + 2 * U * v)
    elif d["act"] == ACT_QUICKGELU:
        sg = torch.sigmoid(1.702 * pre)
        fp = 1.1 * e + U * ref.abs() * ((1 - sg) * (3.404 * pre.abs() + 2) + 4)
    else:
        fp = e
    ub = U if d["x3"] else UB
    return ref, 1.05 * (ub * (ref.abs() + fp) + fp)


def emulate(case, op=None):
    """The kernel's rounding points in fp32: fp32 products and sums, + bias, + residual, activation (pooled: ReLU, the fp32 mean of
    four), ONE rounding to bf16 (x3: none, the output is fp32)."""
    d = shape(case)
    op = op or operands(case)
    z, _ = _products(case, op, dtype=torch.float32)
    out = _finish(d, z, op["bias"], op["res"].to(torch.float32) if op["res"] is not None else None)
    return out if d["x3"] else bf16(out)


WRONG = ("drop_ktile", "pad_clamp", "tap_transposed", "res_next_row", "bias_n4", "pool_before_relu", "pool_quad_order",
         "ragged_shift", "gelu_1", "s2_odd")


def wrong_kinds(case):
    """The wrong versions that apply to the case."""
    d = shape(case)
    k = ["drop_ktile", "bias_n4"]
    if d["ks"] == 3:
        k += ["pad_clamp", "tap_transposed"]
    if d["res"]:
        k.append("res_next_row")
    if d["pool"]:
        k += ["pool_before_relu", "pool_quad_order"]
    if d["M"] % d["MV"]:
        k.append("ragged_shift")
    if not d["pool"] and d["act"] == ACT_QUICKGELU:
        k.append("gelu_1")
    if d["s2"]:
        k.append("s2_odd")
    return k


def wrong(case, kind, op=None):
    """Named wrong versions, in float64 (no rounding: the deviation is the mistake alone).
      drop_ktile        the 64 products of the middle K-tile left out, on the rows of ONE tile (the second row tile where there is
                        one) and the columns of the first column tile
      pad_clamp         zero padding replaced by edge clamp
      tap_transposed    tap decode transposed: tap (ky, kx) reads the pixel at (dy, dx) = (kx - 1, ky - 1)
      res_next_row      the residual of row m + 1
      bias_n4           the bias of channel n + 4
      pool_before_relu  the mean of the window, then the ReLU
      pool_quad_order   the quad decode of the pooled rows left out: rows m = 4 q .. 4 q + 3 taken as four raster neighbours
      ragged_shift      the output rows of the last, ragged tile shifted by one (the last one gets the activation of the bias)
      gelu_1            QuickGELU with 1.0 in place of 1.702
      s2_odd            stride 2 sampling the odd pixels (2 yo + 1, 2 xo + 1)"""
    d = shape(case)
    op = op or operands(case)
    bias = op["bias"].to(F64)
    r = op["res"].to(F64) if op["res"] is not None else None
    if kind not in wrong_kinds(case):
        raise KeyError((kind, case["cmd"]))
    if kind == "drop_ktile":
        nt = -(-d["M"] // d["MV"])
        t = 1 if nt > 1 else 0
        nk = -(-d["K"] // 64)
        k0 = min((nk // 2) * 64, d["K"] - 64)
        z, _ = _products(case, op, drop=(t * d["MV"], min(d["M"], (t + 1) * d["MV"]), d["BN"], k0))
        return _finish(d, z, bias, r)
    if kind == "pad_clamp":
        return _finish(d, _products(case, op, clamp=True)[0], bias, r)
    if kind == "tap_transposed":
        return _finish(d, _products(case, op, swap=True)[0], bias, r)
    if kind == "s2_odd":
        return _finish(d, _products(case, op, odd=True)[0], bias, r)
    if kind == "pool_quad_order":
        return _finish(d, _products(case, op, raster=True)[0], bias, r)
    z, _ = _products(case, op)
    if kind == "res_next_row":
        return _finish(d, z, bias, torch.roll(r, -1, 0))
    if kind == "bias_n4":
        return _finish(d, z, torch.roll(bias, -4), r)
    if kind == "pool_before_relu":
        return _finish(d, z, bias, r, pool_first=True)
    if kind == "gelu_1":
        return _finish(d, z, bias, r, gelu_c=1.0)
    if kind == "ragged_shift":
        out = _finish(d, z, bias, r)
        lo = (d["M"] // d["MV"]) * d["tile_rows"]
        last = _finish(d, torch.zeros(4 if d["pool"] else 1, d["Cout"], dtype=F64), bias, None)
        return torch.cat([out[:lo], out[lo + 1:], last], 0)
    raise KeyError(kind)

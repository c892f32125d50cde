"""Float64 references, element-wise error bounds, fp32 / bf16 emulations and named wrong versions of the fused MFMA kernels of the
trunk outside conv_igemm.hip, and the list of cases that reaches every registered instance of their nine templates through the
public entry points.  CPU only.  tests/test_trunk_fused_ref.py checks here, without a GPU, that every case launches the instance
it names, that the instances named are all but the exempt ones, that the case list has the edges each kernel needs, and that the
bounds bite: the emulation of the kernel's arithmetic stays under them and each wrong version exceeds them at least 4 x somewhere.
tests/test_gpu_trunk_fused.py then holds the kernels to the same bounds.

  conv3x3_narrow.hip  conv3x3_narrow_kernel (gather), conv3x3_rows_kernel (28-pixel row tiles), conv3x3_rowsN_kernel (RT rows)
  conv_pair.hip       conv1x1_pair_kernel, conv1x1_pair512_kernel, conv1x1_regw_kernel
  conv_bneck.hip      conv3x3_img_kernel, bneck23_kernel (conv2 + conv3, and with F1 conv1 in front)
  conv_basic.hip      basic_tail_s2_kernel

Every reference takes the SAME bf16 (and fp32) operands the kernel gets and works in float64.  bf16 has unit roundoff UB = 2^-8,
fp32 U = 2^-24 (as in _conv_tile_ref.py, whose derivation this follows).

One stored element, v = act(sum_k a_k w_k + extras):
  * products: bf16 x bf16 has 16 significant bits, exact in fp32.
  * accumulation: every kernel here keeps ONE fp32 accumulator per output element (per wave) and feeds it v_mfma_f32_32x32x16_bf16
    steps of 16 products in K order; the order inside a step is not documented, so a step is charged as 16 sequential additions.
    An element whose longest chain of additions has n links is off by at most  e = n U (sum_k |a_k w_k| + |extras|).  n per kernel,
    read off its K walk:
      narrow / rows / rowsN   9 Cin products (9 Cin / 16 steps, no padding of K) + the bias (rows, rowsN: the bias IS the initial
                              accumulator; gather: added after): n = 9 Cin + 1
      pair, GEMM 1            64 products (TWO: 128, both matrices into the same accumulator) + bias (TWO: + 1 for b0 + b1, summed
                              in fp32 when the biases are staged) + residual: n = 64 (1 + TWO) + 1 + TWO + RES
      pair, GEMM 2            256 products + bias: n = 257          pair512: GEMM 1 n = 128 + 2, GEMM 2 n = 512 + 1
      regw                    n = K + 1 + RES
      img                     the eight waves split K: a wave walks 9 C / 8 products (both channel chunks of the pooled geometry
                              into the same accumulator), the partials are folded ((w0 + w4) + (w1 + w5)) + ((w2 + w6) + (w3 + w7)):
                              3 more links, then the bias: n = 9 C / 8 + 3 + 1
      bneck23                 conv2 n = 9 C + 1, conv3 n = C + 2 (bias, identity); conv1 of bneck123 n = 4 C + 1 (the zero-filled
                              K-tile past the end and the rows >= 196 add zeros: exact)
      tail                    n = 9 planes + inplanes + 1 (bias_cat arrives summed)
  * ReLU has Lipschitz constant 1: it passes e on unchanged.
  * pooled epilogues of the 3x3 kernels (narrow, rows, img): v_i = relu(.) of the window's four pixels are added in two levels and
    scaled by 0.25 (exact):  fp = 0.25 (sum_i e_i + 2 U sum_i v_i).
  * ONE rounding of each stored tensor to bf16: UB (|ref| + fp).
  bound = 1.05 (UB (|ref| + fp) + fp): 5 % on top, as elsewhere.

Two-stage kernels.  The pair kernels return their intermediate y, so each stage is isolated exactly: y is held to its own bound;
z is held against float64 of the KERNEL'S OWN returned bf16 y (GEMM 2 reads exactly those values out of registers / LDS); the pooled
y is the mean of the ROUNDED y, (r0 + r1) + (r2 + r3) in fp32 (2 links, n = 2) and is held against the mean of the kernel's own y.
With y = NULL the pooled kernel must return z and the pooled y bit for bit as with y stored.

bneck23 / bneck123 keep c2 (and c1) in LDS: their bf16 roundings are not observable.  The reference rounds its own float64 c2 to
bf16.  The kernel's fp32 value of that element lies within d of the float64 one (d = its accumulation bound e, plus, for
bneck123, what flipped c1 elements can move it), so the two round to the SAME bf16 value unless a rounding tie of the bf16 grid
lies within d of the float64 value; then they may differ by one bf16 ulp of that value (an element within d of zero: by at most
2.1 d, the ReLU's corner).  Exactly those elements are "at risk", and the next stage's element n is charged
    flip_n = sum_k risk_k ulp_k |w_next[n, k]|
on top of its own e (bneck123: c1's risk goes into c2's d, c2's risk into y's bound).  An ulp is at most 2 UB of its value, so
flip_n <= 2 UB sum over the elements at risk of c2_k |w3[n, k]|: with a share r of the K elements at risk and sums that do not
cancel (family "sum": non-negative activations, weights of mean 1 and deviation 1/2 in units of 1.5 / K) that is about 2 r of the
output's own rounding term UB |y|.  The allowance is only as small as that share, so the module states a CAP on it, RISK_CAP =
1/8 of the intermediate elements of a case: under it the allowance stays near a quarter of the rounding term and the bound stays
a rounding bound.  reference() reports the share; the CPU test and the GPU check assert the cap (a condition on the operands, not
a measurement of the kernel: with zero-mean operands sum |a w| is ~ sqrt(K) times |sum a w|, d exceeds half an ulp and every
element is at risk -- such operands are not used for these two kernels).
"""
import re
import zlib

import torch

from _bounds import F64, U, UB, bf16, randn as _randn, worst_ratio  # noqa: F401  (worst_ratio: re-exported for the checks)

CHUNK = 8192
RISK_CAP = 0.125

SETTINGS = {
    "default": {},
    "rowsn0": {"EC_CONV_ROWSN": "0"},
    "rowsn2": {"EC_CONV_ROWSN": "2"},
    "rowsn3": {"EC_CONV_ROWSN": "3"},
    "narrow2": {"EC_CONV_NARROW": "2"},
}
SWITCHES = ("EC_CONV_NARROW", "EC_CONV_ROWSN", "EC_CONV_REGW", "EC_RN50_POOLOUT", "EC_CONV_BIG", "EC_CONV8_MIN_TILES", "EC_CONV_T224",
            "EC_CONV_T64", "EC_CONV_RING")

TEMPLATES = ("conv3x3_narrow_kernel", "conv3x3_rows_kernel", "conv3x3_rowsN_kernel", "conv1x1_pair_kernel", "conv1x1_pair512_kernel",
             "conv1x1_regw_kernel", "conv3x3_img_kernel", "bneck23_kernel", "basic_tail_s2_kernel")
PACK = "bneck_pack_kernel"         # weight packing in front of img (1 launch), bneck23 (2) and bneck123 (3)

GATHER, ROWS, ROWSN = "conv3x3_narrow_kernel<%s>", "conv3x3_rows_kernel<%s>", "conv3x3_rowsN_kernel<%s>"
PAIR, PAIR512, REGW = "conv1x1_pair_kernel<%s>", "conv1x1_pair512_kernel", "conv1x1_regw_kernel<%s>"
IMG, BNECK, TAIL = "conv3x3_img_kernel<%s>", "bneck23_kernel<%s>", "basic_tail_s2_kernel<%s>"

# instances of the nine templates no public entry point reaches: instance -> the test that covers it
EXEMPT = {
    REGW % "128, 512, true, true, true":
        "tests/test_gpu_encoder.py::test_pooled_copy_from_layer2s_last_conv3_is_bit_identical_to_the_pooling_pass",
}

# (setting, command, instance, input family).  Commands (tools/launch_log.cpp): conv B H W Cin Cout ks pool act res ldo; pair M K0 N N2
# two res; pairpool B H W K0 N N2 y; img B H C pool ldo; bneck23 / bneck123 B H W C; tail B Ho Wo planes inplanes Cout.
# Shapes: W = 56 is two 28-pixel segments (pooled: four of 14); 12 x 18 is a non-square map whose width is no multiple of 28 / 14
# and whose 216 pixels (54 pooling windows) are no multiple of a 32-pixel (8-window) tile, so tiles straddle rows and frames; four
# frames make M % 32 == 0.  Persistent loops:
# 513 x 8 x 56 / (4 x 28) = 2,052 tiles on 256 x 8 waves; 110 x 7 x 2 = 1,540 on 256 x 6; 608 x 216 / 32 = 4,104 on 256 x 16;
# M = 32 x 1,031: 1,031 tiles on 256 x 4 waves (pair) or 256 workgroups (pair512, regw: 4 x 256 + 7).  tail: Cout = 256 takes the
# 128 x 128 tiles from ceil(M / 128) = 256 on: 167 x 14 x 14 = 32,732 rows (256 tiles, the last of 92 rows), 166 frames stay on
# 64 x 64 (32,536 = 508 x 64 + 24).
CASES = [
    # ---- conv3x3_rowsN_kernel
    ("default", "conv 3 6 56 64 64 3 0 1 0 0", ROWSN % "64, 64, 2, 4, 2", "pos"),
    ("default", "conv 3 8 56 32 32 3 0 1 0 0", ROWSN % "32, 32, 4, 8, 1", "zm"),
    ("default", "conv 513 8 56 32 32 3 0 1 0 0", ROWSN % "32, 32, 4, 8, 1", "pos"),
    ("rowsn2", "conv 3 8 56 32 32 3 0 1 0 0", ROWSN % "32, 32, 4, 4, 2", "pos"),
    ("rowsn3", "conv 3 6 56 64 64 3 0 1 0 0", ROWSN % "64, 64, 2, 4, 3", "zm"),
    # ---- conv3x3_rows_kernel: H no multiple of RT (the row-tile kernel's own fallback), and everything with EC_CONV_ROWSN=0
    ("default", "conv 2 7 56 64 64 3 0 1 0 0", ROWS % "64, 64, false, 6", "zm"),
    ("default", "conv 110 7 56 64 64 3 0 1 0 0", ROWS % "64, 64, false, 6", "pos"),
    ("default", "conv 2 7 56 32 32 3 0 1 0 0", ROWS % "32, 32, false, 16", "pos"),
    ("default", "conv 2 6 56 32 64 3 0 1 0 0", ROWS % "32, 64, false, 16", "zm"),
    ("default", "conv 2 6 56 32 64 3 1 1 0 0", ROWS % "32, 64, true, 16", "pos"),
    ("default", "conv 2 6 56 64 64 3 1 1 0 0", ROWS % "64, 64, true, 8", "zm"),
    ("rowsn0", "conv 3 6 56 64 64 3 0 1 0 0", ROWS % "64, 64, false, 6", "pos"),
    ("rowsn0", "conv 3 8 56 32 32 3 0 1 0 0", ROWS % "32, 32, false, 16", "zm"),
    # ---- conv3x3_narrow_kernel (gather)
    ("default", "conv 4 12 18 32 32 3 0 1 0 0", GATHER % "32, 32, false, 16", "zm"),
    ("default", "conv 608 12 18 32 32 3 0 1 0 0", GATHER % "32, 32, false, 16", "pos"),
    ("default", "conv 4 12 18 32 64 3 0 1 0 0", GATHER % "32, 64, false, 16", "pos"),
    ("default", "conv 4 12 18 32 64 3 1 1 0 0", GATHER % "32, 64, true, 16", "zm"),
    ("narrow2", "conv 4 12 18 64 64 3 0 1 0 0", GATHER % "64, 64, false, 16", "pos"),
    ("narrow2", "conv 4 12 18 64 64 3 1 1 0 0", GATHER % "64, 64, true, 16", "zm"),
    # ---- conv1x1_pair_kernel <TWO, RES, N2, PL>, conv1x1_pair512_kernel
    ("default", "pair 32992 64 256 64 1 1", PAIR % "true, true, 64, false", "zm"),
    ("default", "pair 320 64 256 64 1 0", PAIR % "true, false, 64, false", "pos"),
    ("default", "pair 320 64 256 64 0 1", PAIR % "false, true, 64, false", "pos"),
    ("default", "pair 320 64 256 64 0 0", PAIR % "false, false, 64, false", "zm"),
    ("default", "pair 320 64 256 128 0 1", PAIR % "false, true, 128, false", "zm"),
    ("default", "pair 320 64 256 128 0 0", PAIR % "false, false, 128, false", "pos"),
    ("default", "pairpool 3 8 16 64 256 128 1", PAIR % "false, true, 128, true", "zm"),
    ("default", "pairpool 3 8 16 64 256 128 0", PAIR % "false, true, 128, true", "pos"),
    ("default", "pair 32992 128 512 128 0 1", PAIR512, "zm"),
    # ---- conv1x1_regw_kernel <K, N, RES, RELU, PL>: 1,031 tiles
    ("default", "conv 1031 4 8 256 512 1 0 0 0 0", REGW % "256, 512, false, false, false", "zm"),
    ("default", "conv 1031 4 8 512 256 1 0 1 0 0", REGW % "512, 256, false, true, false", "pos"),
    ("default", "conv 1031 4 8 128 512 1 0 1 1 0", REGW % "128, 512, true, true, false", "zm"),
    # ---- conv3x3_img_kernel <C, HW, FN, NCH, POOL>: B = 33 is more than 256 workgroups
    ("default", "img 1 14 256 0 0", IMG % "256, 14, 1, 1, false", "pos"),
    ("default", "img 3 14 256 0 0", IMG % "256, 14, 1, 1, false", "zm"),
    ("default", "img 33 14 256 0 0", IMG % "256, 14, 1, 1, false", "pos"),
    ("default", "img 1 7 512 0 0", IMG % "512, 7, 2, 1, false", "zm"),
    ("default", "img 3 7 512 0 0", IMG % "512, 7, 2, 1, false", "pos"),
    ("default", "img 33 7 512 0 0", IMG % "512, 7, 2, 1, false", "zm"),
    ("default", "img 1 14 512 1 0", IMG % "512, 14, 1, 2, true", "pos"),
    ("default", "img 3 14 512 1 640", IMG % "512, 14, 1, 2, true", "zm"),
    ("default", "img 33 14 512 1 0", IMG % "512, 14, 1, 2, true", "pos"),
    # ---- bneck23_kernel <C, HW, F1, WEMU>
    ("default", "bneck23 1 14 14 256", BNECK % "256, 14, false, false", "sum"),
    ("default", "bneck23 3 14 14 256", BNECK % "256, 14, false, false", "sum"),
    ("default", "bneck123 1 14 14 256", BNECK % "256, 14, true, false", "sum"),
    ("default", "bneck123 3 14 14 256", BNECK % "256, 14, true, false", "sum"),
    # ---- basic_tail_s2_kernel <BM, BN>
    ("default", "tail 167 14 14 64 128 256", TAIL % "128, 128", "zm"),
    ("default", "tail 166 14 14 64 128 256", TAIL % "64, 64", "pos"),
]
CASES = [dict(setting=s, cmd=c, instance=i, family=f) for s, c, i, f in CASES]


def cases_of(setting):
    return [c for c in CASES if c["setting"] == setting]


def launches_of(case):
    """The launch sequence of the case's command: the weight packing in front, where the entry point needs packed weights."""
    n = {"img": 1, "bneck23": 2, "bneck123": 3}.get(case["cmd"].split()[0], 0)
    return [PACK] * n + [case["instance"]]


def strip_args(kernel):
    """`name<...>(argument types)` of the recorder -> `name<...>`"""
    return re.sub(r"\(.*\)$", "", kernel)


def shape(case):
    """The command's numbers by name, and the tile walk of the case's instance: M kernel rows (pixels before pooling), N output
    channels, nt tiles, GW tiles taken per sweep of the persistent grid (0: one workgroup per tile, no loop)."""
    f = case["cmd"].split()
    v = [int(t) for t in f[1:]]
    tpl, _, targs = case["instance"].partition("<")
    t = [a.strip() for a in targs.rstrip(">").split(",")] if targs else []
    d = dict(kind=f[0], tpl=tpl, pool=0, res=0, two=0, act=1, ldo=0, B=1, GW=0)
    if f[0] == "conv":
        d.update(zip(("B", "H", "W", "Cin", "N", "ks", "pool", "act", "res", "ldo"), v))
        d["M"] = d["B"] * d["H"] * d["W"]
        if d["ks"] == 1:
            d.update(kind="regw", K=d["Cin"], nt=d["M"] // 32)
            d["GW"] = min(d["nt"], 256)
        else:
            d["K"] = 9 * d["Cin"]
            if tpl == "conv3x3_narrow_kernel":
                d.update(nt=d["M"] // 32, NW=int(t[3]))
            elif tpl == "conv3x3_rows_kernel":
                d.update(nt=d["M"] // 28, NW=int(t[3]), RT=2 if d["pool"] else 1, SEG=14 if d["pool"] else 28)
            else:
                d.update(RT=int(t[2]), NW=int(t[3]), SEG=28)
                d["nt"] = d["M"] // (28 * d["RT"])
            d["GW"] = min(-(-d["nt"] // d["NW"]), 256) * d["NW"]
    elif f[0] == "pair":
        d.update(zip(("M", "K", "N", "N2", "two", "res"), v))
        d["nt"] = d["M"] // 32
        d["GW"] = min(d["nt"], 256) if d["K"] == 128 else min(-(-d["nt"] // 4), 256) * 4
    elif f[0] == "pairpool":
        d.update(zip(("B", "H", "W", "K", "N", "N2", "ystored"), v))
        d.update(M=d["B"] * d["H"] * d["W"], res=1, pool=1)
        d["nt"] = d["M"] // 32
        d["GW"] = min(-(-d["nt"] // 4), 256) * 4
    elif f[0] == "img":
        d.update(zip(("B", "H", "Cin", "pool", "ldo"), v))
        d.update(W=d["H"], N=d["Cin"], K=9 * d["Cin"], M=d["B"] * d["H"] ** 2, FN=int(t[2]), NCH=int(t[3]))
    elif f[0] in ("bneck23", "bneck123"):
        d.update(zip(("B", "H", "W", "C"), v))
        d.update(M=d["B"] * d["H"] * d["W"], N=4 * d["C"], res=1)
    elif f[0] == "tail":
        d.update(zip(("B", "H", "W", "P", "I", "N"), v))
        d.update(M=d["B"] * d["H"] * d["W"], K=9 * d["P"] + d["I"], BM=int(t[0]))
        d["nt"] = -(-d["M"] // d["BM"])
    else:
        raise KeyError(f[0])
    d["rows"] = d["M"] // 4 if d["pool"] and d["kind"] in ("conv", "img") else d["M"]
    d["ldo"] = d["ldo"] or d["N"]
    d["loops"] = bool(d["GW"]) and d["nt"] > d["GW"]
    return d


def reduced(case):
    """The same case with at most 4 frames, for the CPU checks; the cases that make the persistent loop go round stay as they are."""
    d = shape(case)
    f = case["cmd"].split()
    if d["loops"] or f[0] == "pair":
        return case
    f[1] = str(min(int(f[1]), 4))
    return dict(case, cmd=" ".join(f))


def _pair_of(seed, family, rows, K, N):
    """activations [rows, K] and weights [N, K] of a family, fp32"""
    x = _randn(seed, rows, K)
    w = _randn(seed + 1, N, K) * K ** -0.5
    if family == "pos":
        x, w = 0.7 * x.abs(), w + 0.05 * K ** -0.5
    elif family == "sum":
        x, w = 0.7 * x.abs(), (1.0 + 0.5 * _randn(seed + 1, N, K)) * (1.5 / K)
    elif family != "zm":
        raise KeyError(family)
    return x, w


def operands(case):
    """-> dict of the entry point's tensors (bf16; biases fp32), seeded by the command and the family."""
    d = shape(case)
    s = zlib.crc32((case["cmd"] + case["family"]).encode())
    fam, k = case["family"], d["kind"]
    h = lambda t: t.to(torch.bfloat16).contiguous()                      # noqa: E731
    bias = lambda i, n: (0.5 * _randn(s + 10 + i, n)).contiguous()       # noqa: E731
    resid = lambda n: h(_randn(s + 20, d["M"], n).abs() if fam != "zm" else _randn(s + 20, d["M"], n))     # noqa: E731
    if k in ("conv", "img"):
        x, _ = _pair_of(s, fam, d["M"], d["Cin"], 1)
        _, w = _pair_of(s + 2, fam, 1, d["K"], d["N"])
        return dict(x=h(x.reshape(d["B"], d["H"], d["W"], d["Cin"])), w=h(w), bias=bias(0, d["N"]))
    if k == "regw":
        x, w = _pair_of(s, fam, d["M"], d["K"], d["N"])
        return dict(x=h(x), w=h(w), bias=bias(0, d["N"]), res=resid(d["N"]) if d["res"] else None)
    if k in ("pair", "pairpool"):
        a0, w0 = _pair_of(s, fam, d["M"], d["K"], d["N"])
        a1, w1 = _pair_of(s + 2, fam, d["M"], d["K"], d["N"])
        _, w2 = _pair_of(s + 4, fam, 1, d["N"], d["N2"])
        op = dict(a0=h(a0), w0=h(w0), b0=bias(0, d["N"]), w2=h(w2), b2=bias(2, d["N2"]), a1=None, w1=None, b1=None,
                  res=resid(d["N"]) if d["res"] else None)
        if d["two"]:
            op.update(a1=h(a1), w1=h(w1), b1=bias(1, d["N"]))
        return op
    if k in ("bneck23", "bneck123"):
        C = d["C"]
        x, w1 = _pair_of(s, fam, d["M"], 4 * C, C)
        c1, _ = _pair_of(s + 2, fam, d["M"], C, 1)
        _, w2 = _pair_of(s + 3, fam, 1, 9 * C, C)
        _, w3 = _pair_of(s + 4, fam, 1, C, 4 * C)
        return dict(x=h(x), c1=h(c1.reshape(d["B"], d["H"], d["W"], C)), w1=h(w1), w2=h(w2), w3=h(w3), b1=0.1 * bias(1, C),
                    b2=0.1 * bias(2, C), b3=0.1 * bias(3, 4 * C))
    if k == "tail":
        c1, _ = _pair_of(s, fam, d["M"], d["P"], 1)
        _, w = _pair_of(s + 1, fam, 1, d["K"], d["N"])
        x, _ = _pair_of(s + 2, fam, 4 * d["M"], d["I"], 1)
        return dict(c1=h(c1.reshape(d["B"], d["H"], d["W"], d["P"])), x=h(x.reshape(d["B"], 2 * d["H"], 2 * d["W"], d["I"])),
                    w=h(w), bias=bias(0, d["N"]))
    raise KeyError(k)


# ---------------------------------------------------------------------------------------------------------------- building blocks
def _pix(B, H, W, rows=None):
    """(b, y, x) of raster rows (all, or the given ones)"""
    m = torch.arange(B * H * W) if rows is None else rows
    return m // (H * W), (m // W) % H, m % W


def _im2col(x, pix, dtype, seam=0, leak=False):
    """Rows of the implicit-GEMM matrix of a 3x3 / pad 1 conv over x [B, H, W, C] for the pixels pix: [n, 9 C], K = (ky, kx, ci), zeros
    outside the frame.  seam: the halo column across an inner seam of `seam` pixels reads as zero.  leak: the row above the top /
    below the bottom row of a frame is the neighbouring frame's last / first row."""
    B, H, W, _ = x.shape
    b, y, xx = pix
    cols = []
    for ky in range(3):
        for kx in range(3):
            yy, xc, bb = y + ky - 1, xx + kx - 1, b
            if leak:
                up, dn = (yy < 0) & (b > 0), (yy >= H) & (b < B - 1)
                bb = torch.where(up, b - 1, torch.where(dn, b + 1, b))
                yy = torch.where(up, torch.full_like(yy, H - 1), torch.where(dn, torch.zeros_like(yy), yy))
            ok = (yy >= 0) & (yy < H) & (xc >= 0) & (xc < W)
            if seam and kx == 0:
                ok &= ~((xx % seam == 0) & (xx > 0))
            if seam and kx == 2:
                ok &= ~((xx % seam == seam - 1) & (xx < W - 1))
            cols.append(x[bb, yy.clamp(0, H - 1), xc.clamp(0, W - 1)].to(dtype) * ok[:, None].to(dtype))
    return torch.cat(cols, 1)


def _mm(rows_of, n, w, dtype, want_abs):
    """rows_of(lo, hi) @ w^T in chunks of rows -> z [n, N] (and |.| |w|^T)"""
    wt = w.to(dtype).T.contiguous()
    z = torch.empty(n, w.shape[0], dtype=dtype)
    s = torch.empty_like(z) if want_abs else None
    for lo in range(0, n, CHUNK):
        hi = min(n, lo + CHUNK)
        a = rows_of(lo, hi)
        z[lo:hi] = a @ wt
        if want_abs:
            s[lo:hi] = a.abs() @ wt.abs()
    return z, s


def _conv3(x, w, dtype, want_abs=False):
    B, H, W, _ = x.shape
    pix = _pix(B, H, W)
    return _mm(lambda lo, hi: _im2col(x, tuple(t[lo:hi] for t in pix), dtype), B * H * W, w, dtype, want_abs)


def _gemm(a, w, dtype, want_abs=False):
    return _mm(lambda lo, hi: a[lo:hi].to(dtype), a.shape[0], w, dtype, want_abs)


def _pool(v, B, H, W, raster=False):
    """0.25 ((v00 + v01) + (v10 + v11)) of v [B H W, N] -> [B H/2 W/2, N]; raster: four consecutive rows of v instead of the quad"""
    if raster:
        q = v.reshape(-1, 4, v.shape[-1])
        return 0.25 * ((q[:, 0] + q[:, 1]) + (q[:, 2] + q[:, 3]))
    q = v.reshape(B, H // 2, 2, W // 2, 2, v.shape[-1])
    return (0.25 * ((q[:, :, 0, :, 0] + q[:, :, 0, :, 1]) + (q[:, :, 1, :, 0] + q[:, :, 1, :, 1]))).reshape(-1, v.shape[-1])


def _bnd(ref, fp):
    return 1.05 * (UB * (ref.abs() + fp) + fp)


def tile_rows(d, t):
    """Raster pixel rows (before pooling) of tile t of the case's kernel."""
    k, tpl = d["kind"], d["tpl"]
    if k == "conv" and tpl != "conv3x3_narrow_kernel":
        nseg, RT, SEG = d["W"] // d["SEG"], d["RT"], d["SEG"]
        sg, rr, b = t % nseg, (t // nseg) % (d["H"] // RT), t // (nseg * (d["H"] // RT))
        y, x = torch.meshgrid(torch.arange(RT * rr, RT * rr + RT), torch.arange(SEG * sg, SEG * sg + SEG), indexing="ij")
        return ((b * d["H"] + y) * d["W"] + x).reshape(-1)
    if k == "conv" and d["pool"]:
        m = torch.arange(32 * t, 32 * t + 32)
        q, s2, Wp = m // 4, m % 4, d["W"] // 2
        b, r2 = q // ((d["H"] // 2) * Wp), q % ((d["H"] // 2) * Wp)
        return (b * d["H"] + 2 * (r2 // Wp) + s2 // 2) * d["W"] + 2 * (r2 % Wp) + s2 % 2
    if k == "pairpool":
        tpr = d["W"] // 8
        tpi = (d["H"] // 4) * tpr
        b, ty, tx = t // tpi, (t % tpi) // tpr, t % tpr
        y, x = torch.meshgrid(torch.arange(4 * ty, 4 * ty + 4), torch.arange(8 * tx, 8 * tx + 8), indexing="ij")
        return ((b * d["H"] + y) * d["W"] + x).reshape(-1)
    if k in ("img", "bneck23", "bneck123"):            # t = 32-pixel block of an image, 7 (2 at 7 x 7) per image
        pixn = d["H"] * d["W"]
        nb = -(-pixn // 32)
        b, i = t // nb, t % nb
        return b * pixn + torch.arange(32 * i, min(32 * i + 32, pixn))
    step = d.get("BM", 32)
    return torch.arange(step * t, min(step * t + step, d["M"]))


def _pick_tile(d):
    """The tile the single-tile mistakes hit: the second one where there is one (img / bneck: the last block of image 0: 4 real rows)."""
    if d["kind"] in ("img", "bneck23", "bneck123"):
        return -(-(d["H"] * d["W"]) // 32) - 1
    return 1 if d["nt"] > 1 else 0


# ---------------------------------------------------------------------------------------------------------------- the computations
def _img_wave_k(d, wv):
    """K indices (tap-major, channel-minor) that wave wv of conv3x3_img_kernel accumulates: K-tiles [wv KPW, (wv + 1) KPW) of each
    resident channel chunk, KPW = 9 (C / NCH / 32) / 8"""
    ktt = d["Cin"] // 32 // d["NCH"]             # K-tiles of 32 per tap inside a chunk
    kpw = 9 * ktt // 8
    idx = []
    for c in range(d["NCH"]):
        for q in range(wv * kpw, (wv + 1) * kpw):
            k0 = (q // ktt) * d["Cin"] + (c * ktt + q % ktt) * 32
            idx += range(k0, k0 + 32)
    return torch.tensor(idx)


def _near_tie(pre, dlt):
    """-> (at risk, charge): elements whose bf16(relu(pre)) can differ when pre (float64) moves by dlt"""
    v = pre.clamp_min(1e-300)
    ulp = torch.exp2(torch.floor(torch.log2(v)) - 7)
    fr = v / ulp
    dist = ((fr - torch.floor(fr)) - 0.5).abs() * ulp
    zero = pre.abs() <= dlt
    tie = (dist <= dlt) & (pre > dlt)
    return zero | tie, torch.where(zero, 2.1 * dlt, torch.where(tie, ulp, torch.zeros_like(v)))


def _run(case, op, mode, kind=None, got=None):
    """mode "ref": float64, -> {output: (ref, bound)} (+ "risk": share of intermediate elements at risk);  "emu": the kernel's
    rounding points in fp32 -> {output: bf16 values};  "wrong": float64 with the mistake `kind`, no rounding of the outputs.
    got: the outputs under test (two-stage kernels: the reference of a later stage starts from them)."""
    d = shape(case)
    ref = mode == "ref"
    dt = torch.float32 if mode == "emu" else F64
    fin = bf16 if mode == "emu" else (lambda t: t)
    k = d["kind"]
    T = tile_rows(d, _pick_tile(d)) if kind in ("drop_kstep", "second_product_dropped") else None
    out = {}

    def bias_of(b):
        return (torch.roll(b, -4) if kind == "bias_n4" else b).to(dt)[None, :]

    def stale(v):
        """the last tile wave 0 takes, computed from the operand of the tile before it in that wave's loop"""
        if kind == "stale_prefetch":
            last = ((d["nt"] - 1) // d["GW"]) * d["GW"]
            v = v.clone()
            v[tile_rows(d, last)] = v[tile_rows(d, last - d["GW"])]
        return v

    if k in ("conv", "img"):
        x, w = op["x"], op["w"]
        B, H, W = d["B"], d["H"], d["W"]
        K = d["K"]
        if mode == "emu" and k == "img":            # the eight K-split partials, folded in the kernel's order
            pix = _pix(B, H, W)
            part = []
            for wv in range(8):
                idx = _img_wave_k(d, wv)
                part.append(_mm(lambda lo, hi: _im2col(x, tuple(t[lo:hi] for t in pix), dt)[:, idx], d["M"], w[:, idx], dt, False)[0])
            z, s = ((part[0] + part[4]) + (part[1] + part[5])) + ((part[2] + part[6]) + (part[3] + part[7])), None
        else:
            z, s = _conv3(x, w, dt, ref)
        if kind in ("seam_halo_zero", "frame_border_leak"):       # on the first two frames
            rows = torch.arange(min(B, 2) * H * W)
            a = _im2col(x, _pix(B, H, W, rows), dt, seam=d.get("SEG", 0) if kind == "seam_halo_zero" else 0, leak=kind == "frame_border_leak")
            z = z.clone()
            z[rows] = a @ w.to(dt).T
        if kind == "drop_kstep":                                  # one 16-channel step, on one tile (img: one 32-channel slice of it)
            k0 = 16 * (K // 32)
            nc = 32 if k == "img" else d["N"]
            a = _im2col(x, _pix(B, H, W, T), dt)
            z[T, :nc] -= a[:, k0:k0 + 16] @ w[:nc, k0:k0 + 16].to(dt).T
        if kind == "fold_drops_partial":                          # wave 5's partial of image 0, first slice
            rows, ks = torch.arange(H * W), _img_wave_k(d, 5)
            a = _im2col(x, _pix(B, H, W, rows), dt)
            z[rows, :32 * d["FN"]] -= a[:, ks] @ w[:32 * d["FN"], ks].to(dt).T
        b = bias_of(op["bias"])
        pre = stale(z + b)
        if d["pool"]:
            if kind == "pool_before_relu":
                o = torch.relu(_pool(pre, B, H, W))
            else:
                o = _pool(torch.relu(pre), B, H, W, raster=kind == "pool_row_major")
        else:
            o = torch.relu(pre) if d["act"] else pre
        if not ref:
            return {"out": fin(o)}
        n = (K // 8 + 3 + 1) if k == "img" else K + 1
        e = n * U * (s + b.abs())
        fp = 0.25 * (_pool(e, B, H, W) * 4 + 2 * U * _pool(torch.relu(pre), B, H, W) * 4) if d["pool"] else e
        return {"out": (o, _bnd(o, fp))}

    if k == "regw":
        z, s = _gemm(op["x"], op["w"], dt, ref)
        if kind == "drop_kstep":
            k0 = 16 * (d["K"] // 32)
            z[T] -= op["x"][T, k0:k0 + 16].to(dt) @ op["w"][:, k0:k0 + 16].to(dt).T
        b = bias_of(op["bias"])
        r = op["res"].to(dt) if d["res"] else None
        act = torch.relu if d["act"] else (lambda t: t)
        if kind == "res_after_relu":
            o = act(z + b) + r
        else:
            o = act(stale(z + b + (r if r is not None else 0.0)))
        if not ref:
            return {"out": fin(o)}
        e = (d["K"] + 1 + d["res"]) * U * (s + b.abs() + (r.abs() if r is not None else 0.0))
        return {"out": (o, _bnd(o, e))}

    if k in ("pair", "pairpool"):
        B, H, W = d["B"], d.get("H", 0), d.get("W", 0)
        z1, s1 = _gemm(op["a0"], op["w0"], dt, ref)
        if kind == "drop_kstep":
            z1[T] -= op["a0"][T, 32:48].to(dt) @ op["w0"][:, 32:48].to(dt).T
        b = bias_of(op["b0"])
        babs = op["b0"].to(dt).abs()[None, :]
        full = z1 + b
        if d["two"]:
            z2, s2 = _gemm(op["a1"], op["w1"], dt, ref)
            bsum = (op["b0"] + op["b1"]).to(dt)[None, :] if mode == "emu" else b + op["b1"].to(dt)[None, :]
            one = full
            full = z1 + z2 + bsum
            if kind == "second_product_dropped":                   # a0 . w0 + b0 alone, on one tile
                full[T] = one[T]
            babs = babs + op["b1"].to(dt).abs()[None, :]
            s1 = s1 + s2 if ref else None
        r = op["res"].to(dt) if d["res"] else None
        pre = full + (r if r is not None else 0.0)
        y = torch.relu(full) + r if kind == "res_after_relu" else torch.relu(stale(pre))
        if ref:
            n1 = d["K"] * (1 + d["two"]) + 1 + d["two"] + d["res"]
            e = n1 * U * (s1 + babs + (r.abs() if r is not None else 0.0))
            out["y"] = (y, _bnd(y, e))
            yk = got["y"].to(F64)                                   # the kernel's own y from here on
        else:
            yk = fin(y)                                             # ("wrong": unrounded, so that only the mistake deviates)
        if d["pool"]:
            if ref:
                yp = _pool(yk, B, H, W)
                out["yp"] = (yp, _bnd(yp, 2 * U * yp))
            elif kind == "pool_before_relu":
                out["yp"] = fin(torch.relu(_pool(pre, B, H, W)))
            else:
                out["yp"] = fin(_pool(yk, B, H, W, raster=kind == "pool_row_major"))
        w2 = op["w2"]
        if kind == "w2_kperm":                                      # channels 4..7 and 8..11 of GEMM 2's K swapped
            perm = torch.arange(d["N"])
            perm[4:8], perm[8:12] = torch.arange(8, 12), torch.arange(4, 8)
            w2 = w2[:, perm]
        zz, sz = _gemm(yk, w2, dt, ref)
        b2 = op["b2"].to(dt)[None, :]
        z = torch.relu(zz + b2)
        if ref:
            out["z"] = (z, _bnd(z, (d["N"] + 1) * U * (sz + b2.abs())))
            return out
        out.update(y=fin(y), z=fin(z))
        return out

    if k in ("bneck23", "bneck123"):
        B, H, W, C = d["B"], d["H"], d["W"], d["C"]
        x = op["x"]
        risks, n_mid = 0.0, 0
        if k == "bneck123":
            z1, s1 = _gemm(x, op["w1"], dt, ref)
            b1 = op["b1"].to(dt)[None, :]
            v1 = torch.relu(z1 + b1)
            c1 = bf16(v1)
            if ref:
                risk1, ch1 = _near_tie(z1 + b1, (4 * C + 1) * U * (s1 + b1.abs()))
                risks, n_mid = risks + float(risk1.sum()), n_mid + risk1.numel()
            c1 = c1.reshape(B, H, W, C)
        else:
            c1 = op["c1"]
        z2, s2 = _conv3(c1, op["w2"], dt, ref)
        if kind == "frame_border_leak":
            z2 = _mm(lambda lo, hi: _im2col(c1, _pix(B, H, W, torch.arange(lo, hi)), dt, leak=True), d["M"], op["w2"], dt, False)[0]
        b2 = op["b2"].to(dt)[None, :]
        v2 = torch.relu(z2 + b2)
        c2 = bf16(v2)
        z3, s3 = _gemm(c2, op["w3"], dt, ref)
        if kind == "drop_kstep":                                     # conv3, K-step 8 of 16, one block x the 32 channels of wave 1
            z3[T, 32:64] -= c2[T, 128:144] @ op["w3"][32:64, 128:144].to(dt).T
        b3 = bias_of(op["b3"])
        r = x.to(dt)
        y = torch.relu(z3 + b3) + r if kind == "res_after_relu" else torch.relu(z3 + b3 + r)
        if not ref:
            return {"out": fin(y)}
        d2 = (9 * C + 1) * U * (s2 + b2.abs())
        if k == "bneck123":                                          # what flipped c1 elements move c2 by
            pix = _pix(B, H, W)
            d2 = d2 + _mm(lambda lo, hi: _im2col(ch1.reshape(B, H, W, C), tuple(t[lo:hi] for t in pix), F64), d["M"], op["w2"].abs(), F64,
                          False)[0]
        risk2, ch2 = _near_tie(z2 + b2, d2)
        risks, n_mid = risks + float(risk2.sum()), n_mid + risk2.numel()
        flip = ch2 @ op["w3"].to(F64).abs().T
        e3 = (C + 2) * U * (s3 + b3.abs() + r.abs())
        return {"out": (y, _bnd(y, e3 + flip)), "risk": risks / n_mid}

    if k == "tail":
        B, H, W, P = d["B"], d["H"], d["W"], d["P"]
        c1, x, w = op["c1"], op["x"], op["w"]
        o2 = 1 if kind == "s2_tap_odd" else 0
        xs = x[:, o2::2, o2::2].reshape(d["M"], d["I"])
        if kind == "ktile_source":                                   # the first K-tile of x read from c1 (its centre tap) instead
            xs = torch.cat([c1.reshape(d["M"], P)[:, :64], xs[:, 64:]], 1)
        pix = _pix(B, H, W)
        leak = kind == "frame_border_leak"

        def rows_of(lo, hi):
            return torch.cat([_im2col(c1, tuple(t[lo:hi] for t in pix), dt, leak=leak), xs[lo:hi].to(dt)], 1)
        z, s = _mm(rows_of, d["M"], w, dt, ref)
        if kind == "drop_kstep":
            k0 = 16 * (d["K"] // 32)
            z[T, :64] -= rows_of(int(T[0]), int(T[-1]) + 1)[:, k0:k0 + 16] @ w[:64, k0:k0 + 16].to(dt).T
        b = bias_of(op["bias"])
        o = torch.relu(z + b)
        if not ref:
            return {"out": fin(o)}
        return {"out": (o, _bnd(o, (d["K"] + 1) * U * (s + b.abs())))}
    raise KeyError(k)


def outputs(case):
    """names of the tensors the case's kernel stores, in the order the checks report them"""
    k = shape(case)["kind"]
    return ("y", "yp", "z") if k == "pairpool" else ("y", "z") if k == "pair" else ("out",)


def reference(case, op=None, got=None):
    """-> {output: (ref, bound)} float64 (bneck: + "risk", the share of intermediate elements at risk).  got: the outputs under
    test; the pair kernels' z and pooled y are referred to got["y"]."""
    return _run(case, op or operands(case), "ref", got=got)


def emulate(case, op=None):
    return _run(case, op or operands(case), "emu")


WRONG = ("drop_kstep", "bias_n4", "seam_halo_zero", "frame_border_leak", "pool_before_relu", "pool_row_major", "second_product_dropped",
         "res_after_relu", "w2_kperm", "stale_prefetch", "fold_drops_partial", "s2_tap_odd", "ktile_source")


def wrong_kinds(case):
    """The wrong versions that apply to the case (the mistakes themselves: the docstrings at their places in _run)."""
    d = shape(case)
    k = d["kind"]
    kinds = ["drop_kstep", "bias_n4"]
    if k == "conv" and d["tpl"] != "conv3x3_narrow_kernel":
        kinds.append("seam_halo_zero")
    if k in ("conv", "img", "bneck23", "bneck123", "tail") and d["B"] >= 2:
        kinds.append("frame_border_leak")
    if d["pool"]:
        kinds += ["pool_before_relu", "pool_row_major"]
    if d["two"]:
        kinds.append("second_product_dropped")
    if d["res"] and d["act"] and k not in ("bneck23", "bneck123"):     # (family "sum" never reaches the ReLU's corner: no difference there)
        kinds.append("res_after_relu")
    if k in ("pair", "pairpool"):
        kinds.append("w2_kperm")
    if d["loops"]:
        kinds.append("stale_prefetch")
    if k == "img":
        kinds.append("fold_drops_partial")
    if k == "tail":
        kinds += ["s2_tap_odd", "ktile_source"]
    return kinds


def wrong(case, kind, op=None):
    if kind not in wrong_kinds(case):
        raise KeyError((kind, case["cmd"]))
    return _run(case, op or operands(case), "wrong", kind=kind)


def worst_of(case, got, op=None):
    """-> ({output: (worst |got - ref| / bound, flat index)}, share at risk or None) of the outputs `got` of the case"""
    refs = reference(case, op, got)
    return {o: worst_ratio(got[o], *refs[o]) for o in outputs(case)}, refs.get("risk")

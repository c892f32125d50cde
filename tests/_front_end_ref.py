"""Float64 references, element-wise error bounds, fp32/bf16 emulations and named wrong versions of the kernels in front of and
behind the trunk -- the stems (stem_elementwise.hip stem_conv1_kernel, stem_depth.hip stem_conv1_depth_kernel, stem7.hip
stem7_pool_kernel), the 2 x 2 average pool, the two layout kernels and the spatial mean -- and the list of cases that reaches
every registered instance of them through the public entry points.  CPU only.  tests/test_front_end_ref.py checks here, without a
GPU, that every case launches the instance it names, that the instances named are all but the exempt ones, that the list has the
edges, and that the bounds bite: the emulation of each kernel's arithmetic stays under them and each wrong version exceeds them
at least 4 x somewhere.  tests/test_gpu_front_end.py then holds the kernels to the same bounds.

Number formats: bf16 keeps 8 significant bits, round-to-nearest has unit roundoff UB = 2^-8; fp32 has U = 2^-24.  Every bound
gets 5 % on top (second-order terms), as in _conv_tile_ref.py.

The MFMA stems round their operands to bf16 INSIDE the kernel (ec_pack2 / ec_f2bf, round-to-nearest-even): stem_conv1_kernel
<32 | 64, *> and stem_conv1_depth_kernel<32 | 64> the window values and the weights, stem7_pool_kernel the frame while it is
staged (its weights arrive in bf16).  Each such case is held to TWO references:
  * tight (pins the rounding): float64 of the operands rounded exactly as the kernel rounds them.  bf16 x bf16 products are
    exact in fp32; one fp32 accumulator, charged as 16 sequential additions per v_mfma_f32_32x32x16_bf16 k-step (RGB stem 2
    steps = 32, depth stem 1 = 16, stem7 11 = 176) plus one for the bias:
        e = (c + 1) U (sum_k |a_k w_k| + |bias|);   ReLU has Lipschitz constant 1;   bound = 1.05 (UB (|ref| + e) + e)
    This needs the rounded operand to be a function of the kernel's INPUTS alone.  An fp32 frame is its own window value.  The
    depth stem's d * scale + shift and the uint8 stems' u * sc + sh (sc = 1 / (255 std), sh = -mean / std, formed in fp32 on
    the host as ec_stem_conv1_u8 / ec_stem7_pool form them: host_consts) are compiled with -ffp-contract=fast, one fma or a
    multiply and an add.  u8_rounding_condition: for every (channel, byte value) both evaluations round to the SAME bf16, which
    makes the rounded operand independent of the compiler's choice; it holds for all 768 values of each constant set in CONSTS
    (the lopsided third set was chosen so that it does: nothing is excluded from the random frames).  The depth cases take
    depths on a 2^-10 grid and scales / shifts for which both evaluations are EXACT (depth_affine_exact).
  * loose (what the stem loses against upstream's fp32 arithmetic): float64 of the unrounded window values and the fp32 weights;
    |bf(a) bf(w) - a w| <= |a w| (2 UB + UB^2) is added to e (stem7: UB |a w|, only the frame is rounded), plus the fp32
    evaluation of the affine where there is one: U (|u sc| + |a|) |w| per term.
The fp32 VALU routes (COUT = 48, RGB and depth) round no operand: a chain of 27 (depth 9) fp32 FMAs that starts from the bias,
e = 28 U (10 U) (sum |a w| + |bias|), one output rounding; on uint8 frames the reference takes the exact affine and the bound the
U (|u sc| + |a|) |w| above, whichever way the compiler evaluates it.

stem7_pool_kernel rounds each conv pixel (7 x 7, stride 2, pad 3, bias, ReLU) to bf16 and max-pools the bit patterns: the pooled
reference is the 3 x 3 / stride-2 / pad-1 max of the float64 conv, out-of-frame pixels left out (zero fill is the same: every
value is >= 0), and since |max a_i - max b_i| <= max |a_i - b_i| the pooled bound is the max of the window's conv bounds.
avgpool2_kernel: 0.25 (((a + b) + c) + d) in fp32, e = 0.25 * 3 U (|a| + |b| + |c| + |d|), one bf16 rounding.
spatial_mean_kernel: a sequential fp32 sum of HW terms, one division, fp32 out: e = (HW - 1) U sum |x| / HW, bound
1.05 (U (|ref| + e) + e).  nhwc_to_nchw_kernel and nchw_to_nhwc_bf16_kernel are bit-exact against a permute (and ec_f2bf).

Staging branches of the two 3 x 3 stems (chosen inside the kernel; staging_branch restates the rule): `vector` (16-byte loads
through a buffer descriptor: W % 4 == 0, the depth stem also a 16-byte aligned frame pointer, and the launch's frames under
2^32 - 16 bytes), `scalar` otherwise.  The branch between them -- plain float4 loads, W % 4 == 0 with 4 GiB of frames or more in
one launch -- is UNREACHABLE for a test: it needs a 4 GiB frame tensor.  The RGB stem and stem7 have no fallback for a frame
pointer that is not 16-byte (fp32) / 4-byte (uint8) aligned and no caller produces one, so no case runs them on one; the depth
stem's own alignment rule sends such a pointer to scalar staging (single floats), which the `off1` cases run.
"""
import os
import re
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from _bounds import F64, U, UB, bf16, worst_ratio  # noqa: F401  (worst_ratio: re-exported for the checks)

SOURCES = ("stem_elementwise.hip", "stem7.hip", "stem_depth.hip", "resize.hip")        # under embodied_clip_amd/csrc
TEMPLATES = ("stem_conv1_kernel", "stem7_pool_kernel", "stem_conv1_depth_kernel", "avgpool2_kernel", "nhwc_to_nchw_kernel",
             "nchw_to_nhwc_bf16_kernel", "spatial_mean_kernel", "spatial_mean_pair_kernel", "spatial_mean_pair_scalar_kernel",
             "resize_crop_kernel")
STEM, STEM7, DSTEM = "stem_conv1_kernel<%d, %s>", "stem7_pool_kernel<%s>", "stem_conv1_depth_kernel<%d>"
AVG, TONCHW, TONHWC, MEAN = "avgpool2_kernel", "nhwc_to_nchw_kernel", "nchw_to_nhwc_bf16_kernel", "spatial_mean_kernel"

# front-end instances no case below names: instance -> the test that holds it exactly
EXEMPT = {
    "spatial_mean_pair_kernel": "tests/test_gpu_rgbd_pooled_kernels.py::test_pair_kernel_against_float64",
    "spatial_mean_pair_scalar_kernel": "tests/test_gpu_rgbd_pooled_kernels.py::test_pair_kernel_against_float64",
    "resize_crop_kernel": "tests/test_gpu_preprocess.py (bit-exact with the Pillow fixture)",
}

# (mean, std) of the uint8 stems.  clip / imagenet: the constants of the two preprocessors; lopsided: channels far apart, so
# that a channel mix-up is loud -- chosen so that u8_rounding_condition holds for all of its 768 values.
CONSTS = {
    "clip": ((0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)),
    "imagenet": ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225)),
    "lopsided": ((0.125, 0.45, 0.875), (0.25, 0.55, 1.0)),
}
U8_EXCLUDED = {}           # constant set -> [(channel, byte value)] kept out of the random frames (at most 4 of 768): none needed

GRID7 = 512                # persistent grid of stem7_pool_kernel
TPH7, TPW7 = 4, 14         # its pooled tile
AVG_SWEEP = 4096 * 256     # 16-byte vectors one sweep of avgpool2_kernel's grid takes
LDS_LIMIT = 64 * 1024      # layout kernels: HW * 65 floats


def _stem(B, H, W, cout, u8, fam, consts=None):
    return dict(cmd="stem %d %d %d %d %d" % (B, H, W, cout, u8), instance=STEM % (cout, "true" if u8 else "false"), family=fam,
                consts=consts)


_SETS = ("clip", "imagenet", "lopsided")
CASES = []
# stem_conv1: per instance the vector-staged even frame (2 x 2 tiles, ragged 3 and 2) and the scalar-staged odd one (W * 3 = 105,
# bottom and right padding read); once per route the minimal vector row (one output row) and an even W that stages scalar
for i, cout in enumerate((32, 48, 64)):
    for u8 in (0, 1):
        CASES.append(_stem(2, 38, 36, cout, u8, "zm" if (i + u8) % 2 == 0 else "pos", _SETS[i] if u8 else None))
        CASES.append(_stem(3, 33, 35, cout, u8, "pos" if (i + u8) % 2 == 0 else "zm", _SETS[(i + 1) % 3] if u8 else None))
CASES += [_stem(2, 2, 4, 32, 1, "zm", "lopsided"), _stem(2, 2, 4, 48, 0, "pos"),
          _stem(2, 34, 34, 64, 0, "zm"), _stem(2, 34, 34, 48, 1, "pos", "clip")]
# stem7_pool: the minimum; non-square with 3 x 2 ragged tiles and every border; 520 tiles on the grid of 512
for j, (B, H, W) in enumerate(((2, 8, 8), (3, 40, 72), (65, 128, 8))):
    for u8 in (0, 1):
        CASES.append(dict(cmd="stem7 %d %d %d %d" % (B, H, W, u8), instance=STEM7 % ("true" if u8 else "false"),
                          family="zm" if (j + u8) % 2 == 0 else "pos", consts=("imagenet", "clip", "lopsided")[j] if u8 else None))
# stem_conv1_depth: vector staging; scalar staging; the vector shape one float into its allocation (-> scalar staging)
for i, cout in enumerate((32, 48, 64)):
    I = DSTEM % cout
    CASES += [dict(cmd="dstem 2 34 36 %d" % cout, instance=I, family="zm" if i % 2 == 0 else "pos", affine=(4.0, -2.0)),
              dict(cmd="dstem 3 33 31 %d" % cout, instance=I, family="pos" if i % 2 == 0 else "zm", affine=(0.5, 0.25)),
              dict(cmd="dstem 2 34 36 %d" % cout, instance=I, family="pos", affine=(4.0, -2.0), variant="off1")]
CASES += [dict(cmd=c, instance=AVG, family="zm") for c in ("avgpool 3 6 10 16 0", "avgpool 2 4 6 24 40", "avgpool 2 256 520 128 0")]
_LAYOUTS = ((3, 49, 128), (2, 1, 64), (1, 252, 192))
CASES += [dict(cmd="tonchw %d %d %d" % s, instance=TONCHW, family="zm") for s in _LAYOUTS]
CASES += [dict(cmd="tonhwc %d %d %d" % s, instance=TONHWC, family="zm") for s in _LAYOUTS]
CASES += [dict(cmd="mean %d %d %d" % s, instance=MEAN, family="pos") for s in ((3, 49, 128), (2, 1, 3), (5, 196, 13), (1, 49, 2048))]
for _c in CASES:
    _c.setdefault("variant", "")
    _c.setdefault("consts", None)
del _c

COL0 = 8                   # first column of the avgpool column-block output (16-byte aligned)

# nchw_to_nhwc_bf16: the flag's meaning, one run per variant on every tonhwc case.  (preset flag, what is planted at the LAST
# channel of the LAST slab at the LAST pixel of the last frame, flag afterwards)
FLAG_VARIANTS = {
    "all_bf16": (0, None, 0),
    "one_inexact": (0, 1.0 + 2.0 ** -12, 1),
    "nan": (0, float("nan"), 0),
    "minus_zero": (0, -0.0, 0),
    "preset": (1, None, 1),
}


def case_id(case):
    return case["cmd"].replace(" ", "_") + ("-" + case["variant"] if case["variant"] else "")


def strip_args(kernel):
    """`name<...>(argument types)` of the recorder -> `name<...>`"""
    return re.sub(r"\(.*\)$", "", kernel)


def kernels_in_sources(root):
    """Names of the __global__ functions of SOURCES, in file order."""
    names = []
    for f in SOURCES:
        with open(os.path.join(root, "embodied_clip_amd", "csrc", f)) as fh:
            names += re.findall(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", fh.read())
    return names


def bf16_trunc(t):
    """fp32 -> bf16 by dropping the low 16 bits (the wrong rounding), as fp32."""
    return (t.to(torch.float32).contiguous().view(torch.int32) & -65536).view(torch.float32)


def f2bf_bits(t):
    """ec_f2bf on the bit pattern of fp32 ``t`` (common.h) -> int16 patterns; what nchw_to_nhwc_bf16_kernel stores, NaNs included."""
    u = t.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFFFFFF
    return (u >> 16).to(torch.int32).to(torch.int16)           # wraps to the same 16 bits


def shape(case):
    """The command's numbers by name; rows x N of the output as the child lays it out; the MFMA k-step charge."""
    f = case["cmd"].split()
    v = [int(t) for t in f[1:]]
    d = dict(kind=f[0], u8=0, ldo=0, mfma=False, exact=False, out_dtype="bf16", off=1 if case["variant"] == "off1" else 0)
    if f[0] == "stem":
        d.update(zip(("B", "H", "W", "Cout", "u8"), v))
        d.update(Ho=(d["H"] - 1) // 2 + 1, Wo=(d["W"] - 1) // 2 + 1, mfma=d["Cout"] % 32 == 0, C=3, adds=32 if d["Cout"] % 32 == 0 else 27)
    elif f[0] == "dstem":
        d.update(zip(("B", "H", "W", "Cout"), v))
        d.update(Ho=(d["H"] - 1) // 2 + 1, Wo=(d["W"] - 1) // 2 + 1, mfma=d["Cout"] % 32 == 0, C=1, adds=16 if d["Cout"] % 32 == 0 else 9)
    elif f[0] == "stem7":
        d.update(zip(("B", "H", "W", "u8"), v))
        d.update(Cout=64, Hc=d["H"] // 2, Wc=d["W"] // 2, Ho=d["H"] // 4, Wo=d["W"] // 4, mfma=True, C=3, adds=176)
        d["tiles_y"], d["tiles_x"] = -(-d["Ho"] // TPH7), -(-d["Wo"] // TPW7)
        d["ntiles"] = d["B"] * d["tiles_x"] * d["tiles_y"]
    elif f[0] == "avgpool":
        d.update(zip(("B", "H", "W", "Cout", "ldo"), v))
        d.update(Ho=d["H"] // 2, Wo=d["W"] // 2)
        d["vectors"] = d["B"] * d["Ho"] * d["Wo"] * d["Cout"] // 8
    elif f[0] in ("tonchw", "tonhwc", "mean"):
        d.update(zip(("B", "HW", "C"), v))
        d["exact"] = f[0] != "mean"
        d["out_dtype"] = "bf16" if f[0] == "tonhwc" else "f32"
        d["rows"], d["N"] = {"tonchw": (d["B"] * d["C"], d["HW"]), "tonhwc": (d["B"] * d["HW"], d["C"]), "mean": (d["B"], d["C"])}[f[0]]
    else:
        raise KeyError(f[0])
    if "Ho" in d:
        d["rows"], d["N"] = d["B"] * d["Ho"] * d["Wo"], d["Cout"]
    d["ldo"] = d["ldo"] or d["N"]
    d["kinds"] = ("tight", "loose") if d["mfma"] else ("tight",)
    return d


def staging_branch(case):
    """The staging branch stem_conv1_kernel / stem_conv1_depth_kernel takes for the case (None: another kernel): the kernels' rule
    restated -- W % 4, for the depth stem the frame pointer's alignment (the child allocates 256-byte aligned tensors; `off1` starts
    one float in), and the launch's frame bytes against 2^32 - 16."""
    d = shape(case)
    if d["kind"] not in ("stem", "dstem"):
        return None
    vec = d["W"] % 4 == 0
    if d["kind"] == "dstem":
        vec = vec and (4 * d["off"]) % 16 == 0
    nbytes = d["B"] * d["H"] * d["W"] * d["C"] * (1 if d["u8"] else 4)
    return "scalar" if not vec else ("vector" if nbytes < 2 ** 32 - 16 else "float4")


def reduced(case):
    """The same case at a size the CPU checks afford: only the grid-stride avgpool case shrinks (8 rows of its frames)."""
    d = shape(case)
    if d["kind"] == "avgpool" and d["vectors"] > AVG_SWEEP:
        return dict(case, cmd="avgpool 1 8 %d %d %d" % (d["W"], d["Cout"], 0))
    return case


# ---- the uint8 and depth affines ----------------------------------------------------------------------------------------------

def host_consts(name):
    """sc = 1 / (255 std), sh = -mean / std in fp32, operation by operation as the entry points form them -> two float32[3]"""
    mean, std = (np.asarray(t, dtype=np.float32) for t in CONSTS[name])
    return np.float32(1.0) / (np.float32(255.0) * std), -mean / std


def u8_affine(name, rot=0):
    """-> (exact [3, 256] float64, fused fp32, unfused fp32) of u * sc[c] + sh[c]; rot: the constants of channel c + rot"""
    sc, sh = host_consts(name)
    sc, sh = np.roll(sc, -rot), np.roll(sh, -rot)
    u = np.arange(256, dtype=np.float32)[None, :]
    exact = u.astype(np.float64) * sc.astype(np.float64)[:, None] + sh.astype(np.float64)[:, None]   # 8 x 24 bits + 24 bits: exact
    fused = exact.astype(np.float32)
    unfused = (u * sc[:, None]).astype(np.float32) + sh[:, None]
    return exact, fused, unfused.astype(np.float32)


def u8_rounding_condition(name):
    """(channel, byte value) pairs whose fused and unfused fp32 evaluation round to different bf16 values: must be empty (or
    listed in U8_EXCLUDED) for the tight reference of the uint8 cases to be a function of the inputs."""
    _e, fused, unfused = u8_affine(name)
    a, b = bf16(torch.from_numpy(fused)), bf16(torch.from_numpy(unfused))
    return [(int(c), int(u)) for c, u in (a != b).nonzero().tolist()]


def depth_affine_exact(case, op=None):
    """d * scale + shift of the case's depths: the product and the sum both exact in fp32 (so fused == unfused == float64)"""
    op = op or operands(case)
    scale, shift = case["affine"]
    d = op["x"].to(F64)
    p = d * scale
    return bool((p.float().to(F64) == p).all() and ((p + shift).float().to(F64) == p + shift).all())


# ---- operands ---------------------------------------------------------------------------------------------------------------

def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(seed, *shape_):
    return torch.randn(*shape_, generator=_gen(seed), dtype=torch.float32)


def pack_stem7(w):
    """bf16 [64, 7, 7, 3] -> the kernel's [64, 176]: k = ky * 24 + kx * 3 + ci, zeros elsewhere"""
    p = torch.zeros(64, 8, 24, dtype=w.dtype)
    p[:, :7, :21] = w.reshape(64, 7, 21)
    return p.reshape(64, 192)[:, :176].contiguous()


def operands(case):
    """-> dict of the entry point's tensors, seeded by the command, the family and the variant.
    stem / dstem: x fp32 | uint8 [B, H, W(, 3)], w fp32 [K, Cout] (k = (ky, kx, ci)), bias fp32; stem7: w bf16 [64, 7, 7, 3];
    avgpool / tonchw / mean: x bf16; tonhwc: x fp32 [B, C, HW], every value a bf16."""
    d = shape(case)
    s = zlib.crc32((case["cmd"] + case["family"] + case["variant"]).encode())
    k = d["kind"]
    if k in ("stem", "dstem", "stem7"):
        B, H, W, C, N = d["B"], d["H"], d["W"], d["C"], d["Cout"]
        if d["u8"]:
            x = torch.randint(0, 256, (B, H, W, 3), generator=_gen(s), dtype=torch.int32)
            for c, u in U8_EXCLUDED.get(case["consts"], ()):
                xc = x[..., c]
                xc[xc == u] = u ^ 1
            x.view(-1)[:6] = torch.tensor([0, 0, 0, 255, 255, 255], dtype=torch.int32)     # both ends of the range in every channel
            x = x.to(torch.uint8)
        elif k == "dstem":
            x = torch.randint(0, 1024, (B, H, W), generator=_gen(s), dtype=torch.int32).float() / 1024.0
        else:
            x = _randn(s, B, H, W, 3)
        ks = 7 if k == "stem7" else 3
        K = ks * ks * C
        w = _randn(s + 1, K, N) * K ** -0.5
        if case["family"] == "pos":
            w = w + 0.3 * K ** -0.5
        elif case["family"] != "zm":
            raise KeyError(case["family"])
        bias = 0.3 * _randn(s + 2, N) + (0.2 if k == "stem7" else 0.0)
        if k == "stem7":
            w = w.T.reshape(64, 7, 7, 3).to(torch.bfloat16).contiguous()
        return dict(x=x.contiguous(), w=w.contiguous(), bias=bias.contiguous())
    if k == "avgpool":
        return dict(x=_randn(s, d["B"], d["H"], d["W"], d["Cout"]).to(torch.bfloat16))
    if k == "tonchw":
        return dict(x=_randn(s, d["B"], d["HW"], d["C"]).to(torch.bfloat16))
    if k == "tonhwc":
        return dict(x=bf16(_randn(s, d["B"], d["C"], d["HW"])))
    if k == "mean":
        return dict(x=(_randn(s, d["B"], d["HW"], d["C"]) + 0.5).to(torch.bfloat16))
    raise KeyError(k)


# ---- window values and implicit-GEMM rows ------------------------------------------------------------------------------------

def window_values(case, op, rot=0):
    """-> (a, ein): the kernel's fp32 window values [B, H, W, C] as float64 (uint8: the fused evaluation; the depth affine is
    exact) and, per value, the bound on |kernel's fp32 value - the exact affine| -- U (|u sc| + |a|) on uint8 frames, else 0.
    Also returned under "exact": the exact affine itself (uint8), else a."""
    d = shape(case)
    x = op["x"]
    if d["u8"]:
        exact, fused, _unf = u8_affine(case["consts"], rot)
        sc, _sh = host_consts(case["consts"])
        idx = x.to(torch.int64)
        ch = torch.arange(3)[None, None, None, :].expand_as(idx)
        ex = torch.from_numpy(exact)[ch, idx]
        a = torch.from_numpy(fused).to(F64)[ch, idx]
        ein = U * (idx.to(F64) * torch.from_numpy(np.roll(sc, -rot).astype(np.float64))[ch].abs() + ex.abs())
        return a, ein, ex
    if d["kind"] == "dstem":
        scale, shift = case["affine"]
        a = (x.to(F64) * scale + shift)[..., None]
        return a, torch.zeros_like(a), a
    a = x.to(F64)
    return a, torch.zeros_like(a), a


def _taps(v, ks, pad, Ho, Wo, padval=None, bottom_next=False):
    """Rows of the implicit-GEMM matrix of a ks x ks / stride-2 conv over v [B, H, W, C]: output (oy, ox) reads input
    (2 oy - pad + ky, 2 ox - pad + kx); [B, Ho, Wo, ks ks C], k = (ky, kx, ci); zeros outside the frame (padval [C]: that value;
    bottom_next: the row below the frame is the next frame's row 0)."""
    B, H, W, C = v.shape
    vp = torch.zeros(B, H + 2 * pad + 2, W + 2 * pad + 2, C, dtype=v.dtype)
    if padval is not None:
        vp[:] = padval.to(v.dtype)
    vp[:, pad:pad + H, pad:pad + W] = v
    if bottom_next:
        vp[:, pad + H, pad:pad + W] = torch.roll(v[:, 0], -1, 0)
    return torch.cat([vp[:, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2] for ky in range(ks) for kx in range(ks)], -1)


def _wmat(case, op, dtype=F64):
    """weights as [K, Cout], k = (ky, kx, ci)"""
    if shape(case)["kind"] == "stem7":
        return op["w"].to(dtype).reshape(64, 147).T.contiguous()
    return op["w"].to(dtype)


def _geom(d):
    """(kernel size, padding, conv rows, conv columns)"""
    return (7, 3, d["Hc"], d["Wc"]) if d["kind"] == "stem7" else (3, 1, d["Ho"], d["Wo"])


def _pool7(conv):
    """3 x 3 / stride-2 / pad-1 max of conv [B, Hc, Wc, 64] >= 0 (zero fill == leaving the out-of-frame pixels out)"""
    return F.max_pool2d(conv.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)


def _finish(d, z, bias):
    """bias + ReLU (stem7: + the max-pool) -> [rows, N]"""
    v = torch.relu(z + bias.to(z.dtype))
    if d["kind"] == "stem7":
        v = _pool7(v)
    return v.reshape(-1, d["Cout"])


def _bnd(ref, fp, ub=UB):
    return 1.05 * (ub * (ref.abs() + fp) + fp)


def _stem_reference(case, op):
    d = shape(case)
    ks, pad, Hc, Wc = _geom(d)
    a, ein, ex = window_values(case, op)
    w = _wmat(case, op)
    bias = op["bias"].to(F64)
    out = {}
    if d["mfma"]:
        ar, wr = bf16(a), bf16(w)                          # what the kernel feeds the MFMA (stem7: w is bf16 already)
        A = _taps(ar, ks, pad, Hc, Wc)
        z, s = A @ wr, A.abs() @ wr.abs()
        e = (d["adds"] + 1) * U * (s + bias.abs())
        cb = _bnd(torch.relu(z + bias), e)
        out["tight"] = (_finish(d, z, bias), (_pool7(cb) if d["kind"] == "stem7" else cb).reshape(-1, d["Cout"]))
        Ax = _taps(ex, ks, pad, Hc, Wc)
        zl, sl = Ax @ w, Ax.abs() @ w.abs()
        lost = sl * (UB if d["kind"] == "stem7" else 2 * UB + UB * UB) + _taps(ein, ks, pad, Hc, Wc) @ w.abs()
        cl = _bnd(torch.relu(zl + bias), e + lost)
        out["loose"] = (_finish(d, zl, bias), (_pool7(cl) if d["kind"] == "stem7" else cl).reshape(-1, d["Cout"]))
    else:
        Ax = _taps(ex, ks, pad, Hc, Wc)
        z, s = Ax @ w, Ax.abs() @ w.abs()
        e = (d["adds"] + 1) * U * (s + bias.abs()) + _taps(ein, ks, pad, Hc, Wc) @ w.abs()
        out["tight"] = (_finish(d, z, bias), _bnd(torch.relu(z + bias), e).reshape(-1, d["Cout"]))
    return out


def _avg_reference(x):
    """x bf16 [B, H, W, C] -> (ref, bound) float64 [B Ho Wo, C], frame by frame"""
    refs, bnds = [], []
    for b in range(x.shape[0]):
        q = x[b].to(F64).reshape(x.shape[1] // 2, 2, x.shape[2] // 2, 2, x.shape[3])
        ref = 0.25 * (q[:, 0, :, 0] + q[:, 0, :, 1] + q[:, 1, :, 0] + q[:, 1, :, 1])
        e = 0.25 * 3 * U * q.abs().sum((1, 3))
        refs.append(ref.reshape(-1, x.shape[3]))
        bnds.append(_bnd(refs[-1], e.reshape(-1, x.shape[3])))
    return torch.cat(refs), torch.cat(bnds)


def reference(case, op=None):
    """-> {kind: (ref, bound)}, float64 [rows, N]; kinds: shape(case)["kinds"].  Exact kernels: bound is None and ref holds the
    expected values (tonchw: fp32; tonhwc: the int16 bit patterns of the bf16 output)."""
    d = shape(case)
    op = op or operands(case)
    k = d["kind"]
    if k in ("stem", "dstem", "stem7"):
        return _stem_reference(case, op)
    x = op["x"]
    if k == "avgpool":
        return {"tight": _avg_reference(x)}
    if k == "mean":
        xd = x.to(F64)
        ref = xd.mean(1)
        e = (d["HW"] - 1) * U * xd.abs().sum(1) / d["HW"]
        return {"tight": (ref, _bnd(ref, e, U))}
    if k == "tonchw":
        return {"tight": (x.float().permute(0, 2, 1).reshape(d["rows"], d["N"]).contiguous(), None)}
    if k == "tonhwc":
        return {"tight": (f2bf_bits(x.permute(0, 2, 1).contiguous()).reshape(d["rows"], d["N"]), None)}
    raise KeyError(k)


# ---- emulations of the kernels' arithmetic ---------------------------------------------------------------------------------------

def _fma_chain(A, w, bias):
    """acc = bias; acc = fma(a_k, w_k, acc) for k in order, fp32 (each fma: the exact product and sum rounded once, via float64)"""
    acc = bias.to(torch.float32).expand(*A.shape[:-1], w.shape[1]).contiguous()
    Af, wf = A.to(torch.float32), w.to(torch.float32)
    for k in range(A.shape[-1]):
        acc = (Af[..., k:k + 1].to(F64) * wf[k].to(F64) + acc.to(F64)).to(torch.float32)
    return acc


def emulate(case, op=None, truncate=False, unfused=False):
    """The kernel's rounding points -> [rows, N] (bf16 values as fp32; fp32 for the mean).  MFMA stems: operands to bf16 (truncate:
    the window values by truncation -- the wrong version), fp32 products and sums, + bias, ReLU, one rounding (stem7: then the max).
    VALU stems: the fp32 FMA chain from the bias.  unfused: uint8 window values as a multiply and an add."""
    d = shape(case)
    op = op or operands(case)
    k = d["kind"]
    if k in ("stem", "dstem", "stem7"):
        ks, pad, Hc, Wc = _geom(d)
        a = window_values(case, op)[0].to(torch.float32)
        if unfused and d["u8"]:
            idx = op["x"].to(torch.int64)
            a = torch.from_numpy(u8_affine(case["consts"])[2])[torch.arange(3)[None, None, None, :].expand_as(idx), idx]
        w, bias = _wmat(case, op, torch.float32), op["bias"]
        if d["mfma"]:
            A = _taps(bf16_trunc(a) if truncate else bf16(a), ks, pad, Hc, Wc)
            conv = bf16(torch.relu(A @ bf16(w) + bias))
        else:
            conv = bf16(torch.relu(_fma_chain(_taps(a, ks, pad, Hc, Wc), w, bias)))
        return (_pool7(conv) if k == "stem7" else conv).reshape(-1, d["Cout"])
    x = op["x"].to(torch.float32)
    if k == "avgpool":
        q = x.reshape(d["B"], d["Ho"], 2, d["Wo"], 2, d["Cout"])
        return bf16(0.25 * (((q[:, :, 0, :, 0] + q[:, :, 0, :, 1]) + q[:, :, 1, :, 0]) + q[:, :, 1, :, 1])).reshape(-1, d["Cout"])
    if k == "mean":
        s = torch.zeros(d["B"], d["C"])
        for hw in range(d["HW"]):
            s = s + x[:, hw]
        return s / float(d["HW"])
    if k == "tonchw":
        return x.permute(0, 2, 1).reshape(d["rows"], d["N"]).contiguous()
    if k == "tonhwc":
        return f2bf_bits(x.permute(0, 2, 1).contiguous()).reshape(d["rows"], d["N"])
    raise KeyError(k)


# ---- named wrong versions -------------------------------------------------------------------------------------------------------

WRONG = ("drop_tap", "seam33", "pad_then_norm", "chan_rot", "trunc", "bottom_next", "pool_unzeroed", "stale_patch", "avg_drop4",
         "mean_skip_last")
TIGHT_ONLY = ("trunc",)    # stays under the loose bound: the reason for the tight reference


def wrong_kinds(case):
    """The wrong versions that apply to the case."""
    d = shape(case)
    k = []
    if d["kind"] in ("stem", "dstem", "stem7"):
        k.append("drop_tap")
        if d["kind"] != "stem7" and d["W"] >= 32:
            k.append("seam33")
        if d["u8"] or (d["kind"] == "dstem" and case["affine"][1] != 0):
            k.append("pad_then_norm")
        if d["u8"]:
            k.append("chan_rot")
        if d["mfma"]:
            k.append("trunc")
        if d["kind"] != "stem7" and d["H"] % 2:
            k.append("bottom_next")
        if d["kind"] == "stem7":
            k.append("pool_unzeroed")
            if d["ntiles"] > GRID7:
                k.append("stale_patch")
    elif d["kind"] == "avgpool":
        k.append("avg_drop4")
    elif d["kind"] == "mean":
        k.append("mean_skip_last")
    return k


def wrong(case, kind, op=None):
    """Named wrong versions -> [rows, N].  In float64 on the operands of the tight reference (no rounding of the result: the deviation
    is the mistake alone), but `trunc`, which is the emulation with the window values truncated.
      drop_tap        the tap (ky, kx) = (1, 2) left out (every channel of it)
      seam33          the 33rd column of a tile's input patch reads as zero: tap kx = 2 of the output columns ox % 16 == 15
      pad_then_norm   the frame padded with raw zeros BEFORE the affine: the padding is sh[c] (depth: shift) instead of 0
      chan_rot        uint8: channel c normalised with the constants of channel c + 1
      trunc           window values (stem7: the staged frame) truncated to bf16 instead of rounded
      bottom_next     odd H: the padding row below the frame is row 0 of the next frame
      pool_unzeroed   stem7: the conv pixels at row / column -1, computed from the zero-padded frame like any other, take part in
                      the max (relu(bias + a partial window) instead of nothing)
      stale_patch     stem7: the tiles past one sweep of the grid (tile >= 512) computed from the patch of the workgroup's FIRST tile
      avg_drop4       0.25 (a + b + c)
      mean_skip_last  the sum stops one pixel early (still divided by HW)"""
    d = shape(case)
    op = op or operands(case)
    if kind not in wrong_kinds(case):
        raise KeyError((kind, case["cmd"]))
    if kind == "trunc":
        return emulate(case, op, truncate=True)
    if kind == "avg_drop4":
        q = op["x"].to(F64).reshape(d["B"], d["Ho"], 2, d["Wo"], 2, d["Cout"])
        return (0.25 * (q[:, :, 0, :, 0] + q[:, :, 0, :, 1] + q[:, :, 1, :, 0])).reshape(-1, d["Cout"])
    if kind == "mean_skip_last":
        return op["x"].to(F64)[:, :-1].sum(1) / d["HW"]
    ks, pad, Hc, Wc = _geom(d)
    rnd = bf16 if d["mfma"] else (lambda t: t)
    a = window_values(case, op, rot=1 if kind == "chan_rot" else 0)[0 if d["mfma"] else 2]
    w, bias = rnd(_wmat(case, op)), op["bias"].to(F64)
    padval = None
    if kind == "pad_then_norm":
        padval = torch.from_numpy(host_consts(case["consts"])[1].astype(np.float64)) if d["u8"] else torch.tensor([case["affine"][1]], dtype=F64)
        padval = rnd(padval)
    if kind == "pool_unzeroed":
        A = _taps(rnd(a), ks, pad + 2, Hc + 1, Wc + 1)                 # conv rows / columns -1 .. Hc - 1
        conv = torch.relu(A @ w + bias)
        return F.max_pool2d(conv.permute(0, 3, 1, 2), 3, 2, 0).permute(0, 2, 3, 1).reshape(-1, 64)
    A = _taps(rnd(a), ks, pad, Hc, Wc, padval=padval, bottom_next=kind == "bottom_next")
    C = d["C"]
    if kind == "drop_tap":
        A = A.clone()
        A[..., (1 * ks + 2) * C:(1 * ks + 3) * C] = 0
    if kind == "seam33":
        A = A.clone()
        for ky in range(3):
            A[:, :, 15::16, (ky * 3 + 2) * C:(ky * 3 + 3) * C] = 0
    out = _finish(d, A @ w, bias)
    if kind == "stale_patch":
        per = d["tiles_x"] * d["tiles_y"]
        assert GRID7 % per == 0                                          # tile t and tile t - 512: the same place in another frame
        out = out.reshape(d["B"], -1).clone()
        first = GRID7 // per
        out[first:] = out[:d["B"] - first]
        out = out.reshape(-1, 64)
    return out

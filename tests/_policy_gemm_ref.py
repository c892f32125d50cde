"""Float64 references, element-wise error bounds, fp32 emulations and named wrong versions of the two kernel families of
gemm_f32.hip (gemm_f32_kernel<BM, BN, WM, WN, ABF, BBF> on the fp32 MFMA, gemm_x3_kernel<BM, BN, WM, WN, ABF, BBF, AKC, BKC> on the
bf16x3 split) behind ec_gemm_f32, and the list of cases that reaches every registered instance of the two.  CPU only.
tests/test_policy_gemm_ref.py checks here, without a GPU, that every case launches the instance it names (tools/launch_log.cpp, the
`f32` command), that the instances named are all the registered ones, and that the bounds bite on reduced cases (fewer rows): the
emulation stays under them and each wrong version exceeds them at least 4 x somewhere.  tests/test_gpu_policy_gemm.py then holds the
kernels to the same bounds on the full cases.

The library registers 12 gemm_f32_kernel instances (4 tiles x {fp32/fp32, bf16 A, bf16 B}) and 24 gemm_x3_kernel instances (the 3
tiles launch_x3 is instantiated for -- 64 x 64, 128 x 128, 256 x 32 -- x 8 type / layout combinations): 36, all reachable.

    C[m, n] (+)= epi( sum_k A(m, k) B(k, n) ),   A(m, k) = A[m sam + k sak],   B(k, n) = B[k sbk + n sbn]
    epi, in the kernel's order:  + bias[n]  ->  + gbias[gidx[m / group] or m / group][n]  ->  ReLU  ->  * rowscale[m]
                                 ->  (dmask[m, n] > 0 ? v : 0)  ->  store | C += v | atomicAdd(C, v) per K slice | part z = v
    (bias and gbias are added by K slice 0 only).

Every reference takes the SAME fp32 / bf16 operands the kernel gets and works in float64; S = sum_k |a_k b_k| comes with it.

Number formats: fp32 has unit roundoff U = 2^-24, bf16 (8 significant bits) UB = 2^-8.  K is walked in tiles of 32, padded with
zeros; a K slice z of a split-K launch walks t_z = its number of K-tiles (nk_per = ceil(ceil(K / 32) / splitk) tiles each, the last
ones fewer or none), with ONE fp32 accumulator per output element and slice.

Bound of the accumulator of slice z (first order), S_z = S over the slice's k range:
  * fp32 kernel: v_mfma_f32_32x32x2_f32 adds two products per step, 16 steps per K-tile; the kernel's header has the result bitwise
    an fmaf chain.  Charged as c_z = 32 t_z sequential fp32 additions (the project's convention: the zero padding counts; also what
    ANY order of that many terms is bounded by) and one more rounding for the products, fused or not:
        e_z = (c_z + 1) U S_z
  * bf16x3 kernel: ec_split3x4 (common.h) splits an fp32 x into p0 = bf16(x), p1 = bf16(x - p0), p2 = bf16(x - p0 - p1) with
    ec_pack2 = v_cvt_pk_bf16_f32, round to nearest even.  The two differences are exact in fp32 and the last residual has at most 8
    significant bits, so x = p0 + p1 + p2 EXACTLY (for |x| below the largest values whose p0 stays finite, and multiples of the
    smallest bf16 subnormal 2^-133: tests/test_gpu_policy_gemm.py::test_split3_planes_sum_exactly), with
        |p0| <= (1 + UB) |x|,  |p1| <= UB |x|,  |p2| <= UB^2 |x|        (weights w = (1 + UB, UB, UB^2); a bf16 operand: w = (1))
    The kernel multiplies the plane pairs with pa + pb <= maxsum (2: all six of fp32 x fp32, or the three of fp32 x bf16;
    EC_GEMM_3PRODUCTS: 1).  Each bf16 x bf16 product is exact in fp32 (16 bits).  What is left out is carried explicitly:
        dropped = sum over pairs with pa + pb > maxsum of wa[pa] wb[pb]         (six products: 2 UB^3 + UB^4 = 2.004 U;
                                                                                 3PRODUCTS: 3 UB^2 + ..., the 2^-16 class)
    The kept products are fed in v_mfma_f32_32x32x16_bf16 steps, 16 products each, two steps per K-tile and plane pair, the
    smallest pairs first; a step is charged as 16 sequential additions, each partial sum bounded by the |a_i b_j|-weighted total
    kept S_z (kept = sum over the P kept pairs of wa[pa] wb[pb]):
        e_z = (32 t_z P U kept + dropped) S_z
Epilogue, both kernels (x the running value, e its error; |x| from the float64 reference):
        + bias: e += U |x|;   + gbias: e += U |x|;   ReLU: Lipschitz 1;   * rowscale: e = |rs| e + U |x|;   mask: exact (e = 0 where
        the mask is off);   store: exact;   C0 + x (ACCUMULATE): e += U |C0 + x|
  * split-K by atomics: the n non-empty slices are added onto C0 in ANY order; every partial sum is at most |C0| + sum_z |x_z|:
        e = sum_z e_z + n U (|C0| + sum_z |x_z|)
  * parts: part z holds x_z (an empty slice: exact zeros) and is judged alone against e_z.
  bound = 1.05 e: 5 % on top, as in _conv_tile_ref.py.  A bound of 0 (masked-off elements of a plain store, empty parts) asks for
  the exact value.

Plane accounting: at these K the accumulation term is most of the x3 bound, which therefore cannot tell six products from five.
Every fp32 x fp32 x3 case without 3PRODUCTS has a second criterion: its relative L2 error against float64 stays under
sqrt(E6 E3), E6 / E3 the relative L2 errors of this module's six- / three-product emulations on the same operands (l2_threshold).

ec_dw_tn_x3 (dw_tn.hip) is the same arithmetic with bf16 X and token splits: dw_reference / dw_emulate / dw_wrong at the end.
"""
import zlib

import torch

from _bounds import F32, F64, U, UB, bf16, randn as _randn, rel_l2, worst_ratio  # noqa: F401  (re-exported for the checks)

GBK = 32
A_BF16, B_BF16, RELU, ACCUMULATE, SPLIT_PARTS, P3 = 1, 2, 4, 8, 16, 32
EC_ERR_ARG, EC_ERR_SHAPE, EC_ERR_UNSUPPORTED = -1, -2, -6

KF = "gemm_f32_kernel<%s>"     # <BM, BN, WM, WN, ABF, BBF>
KX = "gemm_x3_kernel<%s>"      # <BM, BN, WM, WN, ABF, BBF, AKC, BKC>

# The library reads its switches once per process: one recorder / GPU child process per setting.
SETTINGS = {"default": {}, "no_x3": {"EC_GEMM_NO_X3": "1"}}
SWITCHES = ("EC_GEMM_NO_X3",)

# registered gemm instances no case reaches: none.  dw_tn_x3_kernel<2> (dw_tn.hip, the same arithmetic on two planes) is reachable
# only through the learn pass: tests/test_gpu_learn_routes.py covers it; tests/test_gpu_policy_gemm.py covers dw_tn_x3_kernel<3>.
EXEMPT = {}
EXEMPT_RELATED = {"dw_tn_x3_kernel<2>": "tests/test_gpu_learn_routes.py"}

FIELDS = ("M", "N", "K", "sam", "sak", "sbk", "sbn", "ldc", "flags", "bias", "gbias", "gidx", "group", "dmask", "rowscale", "splitk",
          "aoff", "boff")
TILES = {"64": "64, 64, 2, 2", "128": "128, 128, 2, 2", "256x32": "256, 32, 4, 1", "32x256": "32, 256, 1, 4"}


def _cmd(M, N, K, lay, flags=0, ldc=0, bias=0, gbias=0, gidx=0, group=0, dmask=0, rowscale=0, splitk=1, aoff=0, boff=0, ap=0, bp=0):
    """The `f32` command of a call.  lay: two letters, A then B.  A: k = k-contiguous rows of pitch ap or K; r = row-contiguous
    (sam = 1) with pitch ap or M; g = generic (element stride 2, row pitch ap or 2 K).  B: k = W[N][K] (NT) with pitch bp or K;
    n = B[K][N] with pitch bp or N; g = generic (sbn = 2, sbk = bp or 2 N)."""
    sam, sak = {"k": (ap or K, 1), "r": (1, ap or M), "g": (ap or 2 * K, 2)}[lay[0]]
    sbk, sbn = {"k": (1, bp or K), "n": (bp or N, 1), "g": (bp or 2 * N, 2)}[lay[1]]
    return "f32 " + " ".join(str(v) for v in (M, N, K, sam, sak, sbk, sbn, ldc or N, flags, bias, gbias, gidx, group, dmask, rowscale,
                                             splitk, aoff, boff))


def _x(tile, abf, bbf, akc, bkc):
    return KX % ("%s, %s, %s, %s, %s" % (TILES[tile], *(str(bool(v)).lower() for v in (abf, bbf, akc, bkc))))


def _f(tile, abf, bbf):
    return KF % ("%s, %s, %s" % (TILES[tile], str(bool(abf)).lower(), str(bool(bbf)).lower()))


ACC = ACCUMULATE
# (setting, command, instance, input family).  Shapes, read off the dispatch at the end of ec_gemm_f32:
#   * 64 x 64 tiles: fewer than 512 tiles of 128^2 including split-K;
#   * 128 x 128: at least 512 -- split-K + ACCUMULATE (1100 x 600: 9 x 5 tiles x 12 slices = 540; 520 x 520: 25 x 21; 516 x 772: 35 x 15),
#     or parts with ceil(M / 64) ceil(N / 64) splitk > 400 (300 x 330: 5 x 6 x 14 = 420);
#   * x3<256, 32>: N == 32 and ceil(M / 256) splitk >= 512 (130,900 rows = 512 tiles unsplit; 8,300 rows = 33 tiles x 16 slices;
#     16,644 rows = 66 tiles x 8 slices);  f32<256, 32>: N <= 32;  f32<32, 256>: M <= 32 < N.
# K = 148 / 150 are 5 K-tiles: over 4 slices of 2 tiles the last slice is empty.  K = 400 .. 452 over 12 / 14 slices of 2 tiles, 520 over
# 16, 700 over 21, 1000 over 15 (3 tiles each), 300 over 8 leave several trailing slices empty.  group = 49 with M = 150 (3 x 49 + 3).
# The x3 path needs 16-byte (bf16: 8-byte) aligned bases, so its offset bases are 16 / 8 bytes in; a base one ELEMENT in (4 / 2
# bytes), K % 4 != 0, a pitch that is no multiple of 4 or an extent under 32 are what sends a default-setting call to the fp32 kernels.
CASES = [
    # ---- bf16x3, 64 x 64 tiles
    ("default", _cmd(200, 96, 100, "kk", RELU, bias=1, ap=108, aoff=16), _x("64", 0, 0, 1, 1), "zm"),
    ("default", _cmd(200, 96, 100, "kk", RELU | P3, bias=1, ap=108, aoff=16), _x("64", 0, 0, 1, 1), "zm"),
    ("default", _cmd(147, 72, 136, "kn", ACC, ldc=80, dmask=1, rowscale=1, boff=16), _x("64", 0, 0, 1, 0), "pos"),
    ("default", _cmd(132, 100, 68, "rk", 0, gbias=1, group=49, ap=136), _x("64", 0, 0, 0, 1), "zm"),
    ("default", _cmd(100, 200, 148, "rn", ACC, bias=1, gbias=1, gidx=1, group=49, splitk=4), _x("64", 0, 0, 0, 0), "pos"),
    ("default", _cmd(150, 40, 64, "kk", A_BF16 | RELU, gbias=1, gidx=1, group=49, aoff=8, ap=72), _x("64", 1, 0, 1, 1), "pos"),
    ("default", _cmd(70, 64, 96, "kn", A_BF16, bias=1, ldc=72), _x("64", 1, 0, 1, 0), "zm"),
    ("default", _cmd(90, 136, 200, "kn", B_BF16 | RELU, rowscale=1, bp=144, boff=8), _x("64", 0, 1, 1, 0), "zm"),
    ("default", _cmd(36, 260, 1000, "rn", B_BF16 | ACC, splitk=7), _x("64", 0, 1, 0, 0), "pos"),
    ("default", _cmd(70, 96, 148, "kk", SPLIT_PARTS, bias=1, splitk=4), _x("64", 0, 0, 1, 1), "pos"),
    # ---- bf16x3, 128 x 128 tiles
    ("default", _cmd(300, 330, 452, "kk", SPLIT_PARTS, bias=1, splitk=14, ldc=336), _x("128", 0, 0, 1, 1), "zm"),
    ("default", _cmd(1100, 600, 400, "kn", ACC, dmask=1, rowscale=1, splitk=12), _x("128", 0, 0, 1, 0), "pos"),
    ("default", _cmd(520, 520, 700, "rk", ACC, bias=1, gbias=1, group=49, splitk=21), _x("128", 0, 0, 0, 1), "zm"),
    ("default", _cmd(516, 772, 1000, "rn", ACC, splitk=15), _x("128", 0, 0, 0, 0), "zm"),
    ("default", _cmd(330, 300, 452, "kk", A_BF16 | SPLIT_PARTS, bias=1, splitk=14), _x("128", 1, 0, 1, 1), "pos"),
    ("default", _cmd(600, 1100, 400, "kn", A_BF16 | ACC, splitk=12, ldc=1104), _x("128", 1, 0, 1, 0), "zm"),
    ("default", _cmd(1100, 600, 420, "kn", B_BF16 | ACC, rowscale=1, splitk=12), _x("128", 0, 1, 1, 0), "pos"),
    ("default", _cmd(516, 772, 1000, "rn", B_BF16 | ACC, splitk=15, ap=520), _x("128", 0, 1, 0, 0), "pos"),
    # ---- bf16x3, 256 x 32 tiles
    ("default", _cmd(130900, 32, 36, "kk", RELU, bias=1, ldc=40), _x("256x32", 0, 0, 1, 1), "zm"),
    ("default", _cmd(8300, 32, 520, "kn", ACC, dmask=1, rowscale=1, splitk=16), _x("256x32", 0, 0, 1, 0), "pos"),
    ("default", _cmd(8300, 32, 520, "rk", ACC, bias=1, splitk=16), _x("256x32", 0, 0, 0, 1), "zm"),
    ("default", _cmd(16644, 32, 300, "rn", ACC, splitk=8), _x("256x32", 0, 0, 0, 0), "pos"),
    ("default", _cmd(130900, 32, 64, "kk", A_BF16 | RELU, gbias=1, gidx=1, group=49), _x("256x32", 1, 0, 1, 1), "pos"),
    ("default", _cmd(8300, 32, 520, "kn", A_BF16 | ACC, splitk=16), _x("256x32", 1, 0, 1, 0), "zm"),
    ("default", _cmd(8300, 32, 520, "kn", B_BF16 | ACC, splitk=16, ap=524), _x("256x32", 0, 1, 1, 0), "zm"),
    ("default", _cmd(16644, 32, 300, "rn", B_BF16 | ACC, splitk=8), _x("256x32", 0, 1, 0, 0), "pos"),
    # ---- fp32 MFMA, default setting: shapes the x3 path refuses
    ("default", _cmd(300, 96, 70, "kk", RELU, bias=1, ldc=100), _f("64", 0, 0), "zm"),                                # K % 4 != 0
    ("default", _cmd(300, 96, 70, "kk", RELU | P3, bias=1, ldc=100), _f("64", 0, 0), "zm"),                           # ... the flag is inert
    ("default", _cmd(100, 80, 50, "gk", RELU, rowscale=1), _f("64", 0, 0), "zm"),                                     # generic A
    ("default", _cmd(150, 70, 64, "kk", A_BF16 | RELU, gbias=1, gidx=1, group=49, aoff=2), _f("64", 1, 0), "pos"),    # base one element in
    ("default", _cmd(70, 200, 148, "rn", B_BF16 | ACC, bias=1, gbias=1, group=49, splitk=4), _f("64", 0, 1), "pos"),  # M % 4 != 0, row-contiguous A
    ("default", _cmd(70, 96, 150, "kk", SPLIT_PARTS, bias=1, splitk=4), _f("64", 0, 0), "pos"),
    ("default", _cmd(1100, 600, 402, "kn", ACC, dmask=1, rowscale=1, splitk=12, ldc=608), _f("128", 0, 0), "pos"),
    ("default", _cmd(600, 1100, 400, "kk", A_BF16 | ACC, splitk=12, aoff=2, ap=406), _f("128", 1, 0), "zm"),
    ("default", _cmd(518, 772, 1000, "rn", B_BF16 | ACC, splitk=15), _f("128", 0, 1), "zm"),
    ("default", _cmd(700, 32, 200, "kk", RELU, bias=1, ap=203), _f("256x32", 0, 0), "pos"),                           # pitch % 4 != 0
    ("default", _cmd(147, 20, 128, "kk", A_BF16, gbias=1, group=49), _f("256x32", 1, 0), "zm"),                       # N < 32
    ("default", _cmd(300, 24, 100, "rn", B_BF16, bias=1, ldc=32), _f("256x32", 0, 1), "zm"),
    ("default", _cmd(5, 300, 512, "kk", 0, bias=1), _f("32x256", 0, 0), "zm"),                                        # M < 32
    ("default", _cmd(32, 300, 102, "kn", A_BF16 | RELU, bias=1), _f("32x256", 1, 0), "pos"),
    ("default", _cmd(20, 520, 200, "rn", B_BF16, boff=2, bp=522), _f("32x256", 0, 1), "zm"),
    ("default", _cmd(200, 96, 100, "kk", 0, aoff=4, ap=104), _f("64", 0, 0), "pos"),                                  # fp32 base one element in
    ("default", _cmd(90, 100, 44, "kg", 0, bias=1), _f("64", 0, 0), "pos"),                                           # generic B
    # vector loads allowed, the ragged end taken element by element: K % 4 != 0 in a pitch of 72; 70 rows in a pitch of 72
    ("default", _cmd(130, 70, 70, "kk", 0, bias=1, ap=72, bp=72), _f("64", 0, 0), "zm"),
    ("default", _cmd(70, 90, 100, "rn", ACC, ap=72, bp=92), _f("64", 0, 0), "pos"),
    # the operand types the x3 path has no instance for: a k-contiguous bf16 B, a row-contiguous bf16 A (vector branches)
    ("default", _cmd(200, 96, 100, "kk", B_BF16, gbias=1, group=49), _f("64", 0, 1), "zm"),
    ("default", _cmd(200, 96, 100, "rn", A_BF16 | RELU, bias=1), _f("64", 1, 0), "pos"),
    # ---- fp32 MFMA, EC_GEMM_NO_X3=1: aligned shapes, the vector-load branches of the big tiles
    ("no_x3", _cmd(200, 96, 100, "kk", RELU, bias=1, ap=108, aoff=16), _f("64", 0, 0), "zm"),
    ("no_x3", _cmd(1100, 600, 400, "kn", ACC, dmask=1, rowscale=1, splitk=12), _f("128", 0, 0), "pos"),
    ("no_x3", _cmd(600, 1100, 400, "kn", A_BF16 | ACC, splitk=12, ldc=1104), _f("128", 1, 0), "zm"),
    ("no_x3", _cmd(330, 300, 452, "kk", A_BF16 | SPLIT_PARTS, bias=1, splitk=14), _f("64", 1, 0), "pos"),
    ("no_x3", _cmd(516, 772, 1000, "rn", B_BF16 | ACC, splitk=15, ap=520), _f("128", 0, 1), "pos"),
    ("no_x3", _cmd(2100, 32, 64, "kk", A_BF16 | RELU, gbias=1, gidx=1, group=49), _f("256x32", 1, 0), "pos"),
    ("no_x3", _cmd(32, 320, 200, "rn", 0, bias=1), _f("32x256", 0, 0), "zm"),
]
CASES = [dict(setting=s, cmd=c, instance=i, family=f) for s, c, i, f in CASES]

# (setting, command, return code): refused with no launch
REFUSED = [
    ("default", _cmd(70, 96, 148, "kk", SPLIT_PARTS, bias=1, splitk=6), EC_ERR_ARG),           # more parts than K-tiles
    ("default", _cmd(70, 96, 150, "kk", SPLIT_PARTS, bias=1, splitk=6), EC_ERR_ARG),
    ("default", _cmd(70, 96, 148, "kk", SPLIT_PARTS | RELU, bias=1, splitk=4), EC_ERR_ARG),
    ("default", _cmd(70, 96, 148, "kk", SPLIT_PARTS, gbias=1, group=49, splitk=4), EC_ERR_ARG),
    ("default", _cmd(70, 96, 148, "kk", 0, splitk=4), EC_ERR_ARG),                             # atomics without ACCUMULATE
    ("default", _cmd(70, 96, 148, "kk", ACC | RELU, splitk=4), EC_ERR_ARG),
    ("default", _cmd(70, 96, 148, "kk", 0, gbias=1, group=0), EC_ERR_ARG),
    ("default", _cmd(70, 96, 148, "kk", 0, ldc=95), EC_ERR_SHAPE),
    ("default", _cmd(70, 96, 148, "kn", A_BF16 | B_BF16), EC_ERR_UNSUPPORTED),
    ("default", _cmd(70, 96, 150, "kn", A_BF16 | B_BF16), EC_ERR_UNSUPPORTED),
]


def cases_of(setting):
    return [c for c in CASES if c["setting"] == setting]


def short(name):
    return name.replace("(anonymous namespace)::", "").replace("void ", "", 1).replace("(GemmArgs)", "")


def is_gemm(name):
    return name.startswith("gemm_f32_kernel<") or name.startswith("gemm_x3_kernel<")


def shape(case):
    """The command's numbers by name, the flags apart, the tile of the case's instance and the K slices."""
    f = case["cmd"].split()
    assert f[0] == "f32" and len(f) == 19, case["cmd"]
    d = dict(zip(FIELDS, (int(t) for t in f[1:])))
    fl = d["flags"]
    d.update(abf=bool(fl & A_BF16), bbf=bool(fl & B_BF16), relu=bool(fl & RELU), acc=bool(fl & ACCUMULATE), parts=bool(fl & SPLIT_PARTS),
             p3=bool(fl & P3))
    name, args = case["instance"].split("<")
    t = [a.strip() for a in args.rstrip(">").split(",")]
    d["x3"] = name == "gemm_x3_kernel"
    d["BM"], d["BN"] = int(t[0]), int(t[1])
    d["alay"] = "k" if d["sak"] == 1 else "r" if d["sam"] == 1 else "g"
    d["blay"] = "k" if d["sbk"] == 1 else "n" if d["sbn"] == 1 else "g"
    nk = -(-d["K"] // GBK)
    sk = max(1, min(d["splitk"], nk))
    per = -(-nk // sk)
    d["nk"], d["nk_per"], d["nslices"] = nk, per, sk
    d["slices"] = [(min(d["K"], z * per * GBK), min(d["K"], (z + 1) * per * GBK)) for z in range(sk)]     # k ranges; empty: k0 == k1
    d["atomic"] = sk > 1 and not d["parts"]
    d["maxsum"] = 1 if d["p3"] else 2
    d["ngroups"] = -(-d["M"] // d["group"]) if d["group"] else 0
    return d


def reduced(case):
    """The same case with fewer rows: M > 512 becomes 256 + M % 256, the raggedness against every tile kept (the strides stay: a
    row-contiguous A keeps its pitch).  Same generator, same bound formula, a size the CPU checks afford."""
    f = case["cmd"].split()
    M = int(f[1])
    if M > 512:
        f[1] = str(256 + M % 256)
    return dict(case, cmd=" ".join(f))


def twin_cmd(case):
    """the command without EC_GEMM_3PRODUCTS"""
    f = case["cmd"].split()
    f[9] = str(int(f[9]) & ~P3)
    return " ".join(f)


def operands(case):
    """-> dict of the logical operands, seeded by the command: a fp32 [M, K], b fp32 [K, N] (bf16-representable where the flag says
    bf16 storage), bias [N], gbias [rows, N], gidx int32 [ceil(M / group)] (non-monotone, repeated entries), dmask [M, N] (with +0.0,
    -0.0 and negatives), rowscale [M] (negative and zero entries), c0 [M, N] -- or None where the command passes NULL."""
    d = shape(case)
    M, N, K = d["M"], d["N"], d["K"]
    s = zlib.crc32(twin_cmd(case).encode())          # a 3PRODUCTS case has the operands of its unflagged twin
    a = _randn(s, M, K)
    b = _randn(s + 1, K, N) * K ** -0.5
    if case["family"] == "pos":
        a = 0.7 * a.abs()
        b = b + 0.05 * K ** -0.5
    elif case["family"] != "zm":
        raise KeyError(case["family"])
    if d["abf"]:
        a = bf16(a)
    if d["bbf"]:
        b = bf16(b)
    op = dict(a=a, b=b, bias=None, gbias=None, gidx=None, dmask=None, rowscale=None, c0=None)
    if d["bias"]:
        op["bias"] = 0.5 * _randn(s + 2, N)
    if d["gbias"]:
        rows = 7 if d["gidx"] else d["ngroups"]
        op["gbias"] = 0.5 * _randn(s + 3, rows, N)
        if d["gidx"]:
            g = torch.randint(0, 7, (d["ngroups"],), generator=torch.Generator().manual_seed(s + 4), dtype=torch.int32)
            g[:4] = torch.tensor([5, 2, 2, 6], dtype=torch.int32)[:d["ngroups"]]
            op["gidx"] = g
    if d["dmask"]:
        m = _randn(s + 5, M, N)
        m.view(-1)[0::7] = 0.0
        m.view(-1)[3::7] = -0.0
        op["dmask"] = m
    if d["rowscale"]:
        r = _randn(s + 6, M)
        r[2::5] = 0.0
        op["rowscale"] = r
    if d["acc"]:
        op["c0"] = _randn(s + 7, M, N)
    return op


def embed(t, s0, s1, off_elems, dtype, slack=64):
    """t [R, C] laid out at element offset off_elems with strides (s0, s1) in a flat buffer of `dtype` whose every other element is
    NaN (the padding of a pitch, the gaps of a generic stride, the elements before the base and `slack` behind the end)."""
    R, C = t.shape
    buf = torch.full((off_elems + (R - 1) * s0 + (C - 1) * s1 + 1 + slack,), float("nan"), dtype=dtype)
    torch.as_strided(buf, (R, C), (s0, s1), off_elems).copy_(t)
    return buf


def embedded(case, op=None):
    """-> (A buffer, element offset of A(0, 0), B buffer, element offset of B(0, 0)) in the storage types of the case"""
    d = shape(case)
    op = op or operands(case)
    ta, tb = (torch.bfloat16 if d["abf"] else F32), (torch.bfloat16 if d["bbf"] else F32)
    ea, eb = (2 if d["abf"] else 4), (2 if d["bbf"] else 4)
    assert d["aoff"] % ea == 0 and d["boff"] % eb == 0
    return (embed(op["a"], d["sam"], d["sak"], d["aoff"] // ea, ta), d["aoff"] // ea,
            embed(op["b"], d["sbk"], d["sbn"], d["boff"] // eb, tb), d["boff"] // eb)


# ------------------------------------------------------------------------------------------------------------------------------------
def _gb_rows(d, op, dt, shift=0, use_gidx=True):
    """the gbias row of every output row: [M, N]"""
    g = torch.div(torch.arange(d["M"]) + shift, d["group"], rounding_mode="floor").clamp(max=d["ngroups"] - 1)
    if op["gidx"] is not None and use_gidx:
        g = op["gidx"].long()[g]
    return op["gbias"].to(dt)[g.clamp(max=op["gbias"].shape[0] - 1)]


def _slice_value(d, op, z, first, dt, kind=None):
    """The epilogue of one K slice up to the mask, in the dtype of z; `kind`: a wrong version (see wrong())."""
    x = z
    if kind == "relu_before_bias":
        x = torch.relu(x)
    if op["bias"] is not None and (first or kind == "bias_every_slice"):
        x = x + op["bias"].to(dt)[None, :]
    if op["gbias"] is not None and first:
        x = x + _gb_rows(d, op, dt, shift=1 if kind == "gbias_group_off_by_one" else 0, use_gidx=kind != "gidx_ignored")
    if d["relu"] and kind not in ("relu_before_bias", "rowscale_before_relu"):
        x = torch.relu(x)
    if op["rowscale"] is not None:
        x = x * op["rowscale"].to(dt)[:, None]
    if kind == "rowscale_before_relu":
        x = torch.relu(x)
    if op["dmask"] is not None:
        on = (op["dmask"] >= 0) if kind == "mask_ge_zero" else (op["dmask"] > 0)
        x = torch.where(on, x, torch.zeros((), dtype=dt))
    return x


def _combine(d, op, xs, dt, kind=None):
    """slice values -> the output: [M, N], parts: [splitk, M, N]"""
    live = [z for z, (k0, k1) in enumerate(d["slices"]) if k1 > k0]
    if kind == "last_slice_dropped":
        xs = list(xs)
        xs[live[-1]] = torch.zeros_like(xs[live[-1]])
    if d["parts"]:
        out = torch.stack(xs, 0)
        if kind == "empty_slice_not_zeroed":
            out[[z for z in range(d["nslices"]) if z not in live]] = float("nan")
        return out
    c0 = op["c0"].to(dt) if (op["c0"] is not None and kind != "accumulate_ignored") else None
    if d["atomic"]:
        out = c0 if c0 is not None else torch.zeros_like(xs[0])
        for z in live:
            out = out + xs[z]
        return out
    return xs[0] if c0 is None else c0 + xs[0]


def _ldc_as_n(d, out):
    """row r of the result written at flat r N + col into a buffer of pitch ldc (the rest of it: NaN), read back at pitch ldc"""
    def one(o):
        flat = torch.full((d["M"] * d["ldc"],), float("nan"), dtype=o.dtype)
        flat[:o.numel()] = o.reshape(-1)
        return flat.view(d["M"], d["ldc"])[:, :d["N"]]
    return torch.stack([one(o) for o in out], 0) if out.dim() == 3 else one(out)


def _weights(d):
    """plane weights of A and B, the kept plane pairs in the kernel's order (smallest first), sum of their weights, sum of the dropped"""
    wa = (1.0,) if d["abf"] else (1 + UB, UB, UB * UB)
    wb = (1.0,) if d["bbf"] else (1 + UB, UB, UB * UB)
    kept = [(pa, s - pa) for s in (2, 1, 0) for pa in range(len(wa)) if 0 <= s - pa < len(wb) and s <= d["maxsum"]]
    allp = [(pa, pb) for pa in range(len(wa)) for pb in range(len(wb))]
    return wa, wb, kept, sum(wa[i] * wb[j] for i, j in kept), sum(wa[i] * wb[j] for i, j in allp if (i, j) not in kept)


def reference(case, op=None):
    """-> ref, bound: float64 [M, N] (parts: [splitk, M, N])"""
    d = shape(case)
    op = op or operands(case)
    a, b = op["a"].to(F64), op["b"].to(F64)
    aa, ba = a.abs(), b.abs()
    _wa, _wb, kept, kw, dropped = _weights(d)
    xs, es = [], []
    for z, (k0, k1) in enumerate(d["slices"]):
        zz = a[:, k0:k1] @ b[k0:k1]
        S = aa[:, k0:k1] @ ba[k0:k1]
        tiles = -(-(k1 - k0) // GBK)
        e = ((32 * tiles * len(kept) * U * kw + dropped) if d["x3"] else (32 * tiles + 1) * U) * S
        x = zz
        if op["bias"] is not None and z == 0:
            x = x + op["bias"].to(F64)[None, :]
            e = e + U * x.abs()
        if op["gbias"] is not None and z == 0:
            x = x + _gb_rows(d, op, F64)
            e = e + U * x.abs()
        if d["relu"]:
            x = torch.relu(x)
        if op["rowscale"] is not None:
            rs = op["rowscale"].to(F64)[:, None]
            x = x * rs
            e = rs.abs() * e + U * x.abs()
        if op["dmask"] is not None:
            on = op["dmask"] > 0
            x = torch.where(on, x, torch.zeros((), dtype=F64))
            e = torch.where(on, e, torch.zeros((), dtype=F64))
        xs.append(x)
        es.append(e)
    ref = _combine(d, op, xs, F64)
    if d["parts"]:
        e = torch.stack(es, 0)
    elif d["atomic"]:
        live = [z for z, (k0, k1) in enumerate(d["slices"]) if k1 > k0]
        mag = op["c0"].to(F64).abs() + sum(xs[z].abs() for z in live)
        e = sum(es[z] for z in live) + len(live) * U * mag
    elif d["acc"]:
        e = es[0] + U * ref.abs()
    else:
        e = es[0]
    return ref, 1.05 * e


def _planes(t, is_bf16):
    """the planes of ec_split3x4 in fp32 (a bf16 operand: itself)"""
    if is_bf16:
        return [t]
    p0 = bf16(t)
    r = t - p0
    p1 = bf16(r)
    return [p0, p1, bf16(r - p1)]


def _slice_products(d, op, dt=F32, maxsum=None, skip=None):
    """Per K slice the accumulator of the kernel in `dt`: fp32 kernel -- the K-tiles in order, two k per step; x3 kernel -- per K-tile
    and 16-k step the kept plane pairs, smallest first, one product matrix each.  maxsum / skip: another product selection."""
    a, b = op["a"].to(dt), op["b"].to(dt)
    M, N = d["M"], d["N"]
    out = []
    if d["x3"]:
        dd = dict(d, maxsum=d["maxsum"] if maxsum is None else maxsum)
        kept = [p for p in _weights(dd)[2] if p != skip]
        pa, pb = [p.to(dt) for p in _planes(op["a"], d["abf"])], [p.to(dt) for p in _planes(op["b"], d["bbf"])]
    for k0, k1 in d["slices"]:
        acc = torch.zeros(M, N, dtype=dt)
        if d["x3"]:
            for ks in range(k0, k1, 16):
                ke = min(k1, ks + 16)
                for i, j in kept:
                    acc = acc + pa[i][:, ks:ke] @ pb[j][ks:ke]
        else:
            for ks in range(k0, k1, 2):
                acc = acc + a[:, ks:min(k1, ks + 2)] @ b[ks:min(k1, ks + 2)]
        out.append(acc)
    return out


def emulate(case, op=None, maxsum=None):
    """The kernel's arithmetic in fp32 on the CPU: plane split, the products kept, K-tile order, the epilogue's roundings, the split-K
    slices folded in slice order.  maxsum: the product selection of another flag setting (2: six products, 1: three)."""
    d = shape(case)
    op = op or operands(case)
    zs = _slice_products(d, op, F32, maxsum=maxsum)
    return _combine(d, op, [_slice_value(d, op, z, i == 0, F32) for i, z in enumerate(zs)], F32)


def needs_l2(case):
    """fp32 x fp32 on the x3 kernel, all six products: the plane accounting criterion applies"""
    d = shape(case)
    return d["x3"] and not d["abf"] and not d["bbf"] and not d["p3"]


def l2_threshold(case, op=None, ref=None):
    """-> (threshold, E6, E3): relative L2 errors against float64 of the six- and the three-product emulation, their geometric mean"""
    op = op or operands(case)
    ref = reference(case, op)[0] if ref is None else ref
    e6, e3 = rel_l2(emulate(case, op, maxsum=2), ref), rel_l2(emulate(case, op, maxsum=1), ref)
    return (e6 * e3) ** 0.5, e6, e3


def dw_operands(M, NX):
    """dY fp32 [M, 128] (zero-mean, a scale per channel), X bf16 [M, NX] (non-negative features), dW0 fp32 [128, NX]"""
    s = zlib.crc32(b"dw %d %d" % (M, NX))
    dy = _randn(s, M, 128) * torch.rand(1, 128, generator=torch.Generator().manual_seed(s + 1))
    return dict(dy=dy, x=_randn(s + 2, M, NX).abs().to(torch.bfloat16), w0=_randn(s + 3, 128, NX))


def dw_reference(op, nsplit):
    """ec_dw_tn_x3 (dw_tn.hip, dw_tn_x3_kernel<3>): dW = dW0 + dY^T X, dY split as above, X bf16 -- the three products of a k are all
    kept (dropped = 0).  Each of the nsplit token splits walks t = ceil(ceil(M / nsplit) / 32) K-tiles of 32 tokens with one accumulator,
    3 planes x 2 steps of 16 per tile: 96 t additions, weighted total (1 + UB + UB + UB^2) S_split; dw_reduce_kernel adds the splits in
    order (one addition each) and the sum onto dW0 (one more).  With sum_split S_split = S and |part| <= S_split:
        e = (96 t (1 + 2 UB + UB^2) + nsplit) U S + U |dW0 + dY^T X|,   bound = 1.05 e      -> ref, bound: float64 [128, NX]"""
    dy, x = op["dy"].to(F64), op["x"].to(F64)
    M = dy.shape[0]
    t = -(-(-(-M // nsplit)) // 32)
    ref = op["w0"].to(F64) + dy.t() @ x
    S = dy.abs().t() @ x
    return ref, 1.05 * ((96 * t * (1 + 2 * UB + UB * UB) + nsplit) * U * S + U * ref.abs())


def dw_splits(M, NX):
    """-> (token splits, tokens per split) of ec_dw_tn_x3: one workgroup per CU over the NX / 256 column tiles, at most one split per
    32-token K-tile; the tokens of a split rounded up to whole K-tiles"""
    ns = max(1, min(-(-256 // (NX // 256)), -(-M // 32)))
    return ns, -(-(-(-M // ns)) // 32) * 32


def dw_emulate(op, nsplit, tok):
    """The arithmetic of dw_tn_x3_kernel<3> + dw_reduce_kernel in fp32: per split one accumulator over its K-tiles of 32 tokens, two
    16-token steps each, plane 2, 1, 0 of dY per step; the splits added in order from zero, the sum onto dW0."""
    pl = _planes(op["dy"], False)
    x = op["x"].to(F32)
    M = x.shape[0]
    s = torch.zeros_like(op["w0"])
    for k in range(nsplit):
        acc = torch.zeros_like(op["w0"])
        for t0 in range(k * tok, min(M, (k + 1) * tok), 16):
            t1 = min(M, t0 + 16)
            for p in (2, 1, 0):
                acc = acc + pl[p][t0:t1].t() @ x[t0:t1]
        s = s + acc
    return op["w0"] + s


DW_WRONG = ("drop_ktile", "last_split_dropped", "dw0_ignored", "x_next_token")


def dw_wrong(op, nsplit, tok, kind):
    """float64: the ragged last K-tile ignored (M % 32 != 0) | the last non-empty split missing (nsplit > 1) | dW0 overwritten | X read
    one token late"""
    dy, x, w0 = op["dy"].to(F64), op["x"].to(F64), op["w0"].to(F64)
    M = dy.shape[0]
    if kind == "drop_ktile":
        assert M % 32
        return w0 + dy[:M // 32 * 32].t() @ x[:M // 32 * 32]
    if kind == "last_split_dropped":
        assert nsplit > 1
        m = (-(-M // tok) - 1) * tok
        return w0 + dy[:m].t() @ x[:m]
    if kind == "dw0_ignored":
        return dy.t() @ x
    if kind == "x_next_token":
        return w0 + dy.t() @ torch.roll(x, -1, 0)
    raise KeyError(kind)


WRONG = ("drop_ktile", "k_tail_reads_pitch", "operand_transposed", "bias_every_slice", "gbias_group_off_by_one", "gidx_ignored",
         "relu_before_bias", "rowscale_before_relu", "mask_ge_zero", "accumulate_ignored", "empty_slice_not_zeroed",
         "last_slice_dropped", "ldc_as_n", "plane_dropped")


def wrong_kinds(case):
    """The wrong versions that apply to the case."""
    d = shape(case)
    live = sum(k1 > k0 for k0, k1 in d["slices"])
    k = ["operand_transposed"]
    if d["K"] % GBK:
        k.append("drop_ktile")
        if d["alay"] == "k" and d["sam"] > d["K"]:
            k.append("k_tail_reads_pitch")
    if d["bias"] and live > 1:
        k.append("bias_every_slice")
    if d["gbias"]:
        k.append("gbias_group_off_by_one")
        if d["gidx"]:
            k.append("gidx_ignored")
    if d["relu"] and (d["bias"] or d["gbias"]):
        k.append("relu_before_bias")
    if d["relu"] and d["rowscale"]:
        k.append("rowscale_before_relu")
    if d["dmask"]:
        k.append("mask_ge_zero")
    if d["acc"]:
        k.append("accumulate_ignored")
    if d["parts"] and live < d["nslices"]:
        k.append("empty_slice_not_zeroed")
    if live > 1:
        k.append("last_slice_dropped")
    if d["ldc"] > d["N"]:
        k.append("ldc_as_n")
    if needs_l2(case):
        k.append("plane_dropped")
    return k


def wrong(case, kind, op=None):
    """Named wrong versions, in float64 (no rounding: the deviation is the mistake alone).
      drop_ktile              the ragged last K-tile is ignored
      k_tail_reads_pitch      the K padding of the last K-tile of a k-contiguous A is read from the row pitch, not taken as zero,
                              against B's padding read as the following rows (the pitch holds NaN)
      operand_transposed      B read with the other layout: the [K][N] image taken as [N][K]
      bias_every_slice        every K slice adds the bias
      gbias_group_off_by_one  the group of row m is (m + 1) / group
      gidx_ignored            the group index itself in place of gidx[group]
      relu_before_bias        ReLU on the bare product, then the biases
      rowscale_before_relu    the row scale, then the ReLU
      mask_ge_zero            dmask >= 0 in place of > 0 (lets +0.0 and -0.0 through)
      accumulate_ignored      C0 overwritten
      empty_slice_not_zeroed  parts: an empty trailing slice leaves its part as it was (NaN)
      last_slice_dropped      the last non-empty K slice is missing
      ldc_as_n                rows written at pitch N into the pitch-ldc output
      plane_dropped           the a1 b1 product of the six is missing"""
    d = shape(case)
    op = op or operands(case)
    if kind not in wrong_kinds(case):
        raise KeyError((kind, case["cmd"]))
    a, b = op["a"].to(F64), op["b"].to(F64)
    if kind == "operand_transposed":
        b = b.t().contiguous().reshape(d["K"], d["N"])
    if kind == "plane_dropped":
        zs = _slice_products(d, op, F64, skip=(1, 1))
    else:
        zs = [a[:, k0:k1] @ b[k0:k1] for k0, k1 in d["slices"]]
    if kind == "drop_ktile":
        kr = (d["K"] // GBK) * GBK
        z = max(i for i, (k0, k1) in enumerate(d["slices"]) if k1 > k0)
        zs[z] = zs[z] - a[:, kr:] @ b[kr:]
    if kind == "k_tail_reads_pitch":
        abuf, ao, _bbuf, _bo = embedded(case, op)
        kp = min(d["nk"] * GBK, d["sam"])
        tail = torch.as_strided(abuf, (d["M"], kp - d["K"]), (d["sam"], 1), ao + d["K"]).to(F64)
        z = max(i for i, (k0, k1) in enumerate(d["slices"]) if k1 > k0)
        zs[z] = zs[z] + tail @ torch.ones(kp - d["K"], d["N"], dtype=F64)
    out = _combine(d, op, [_slice_value(d, op, z, i == 0, F64, kind) for i, z in enumerate(zs)], F64, kind)
    return _ldc_as_n(d, out) if kind == "ldc_as_n" else out

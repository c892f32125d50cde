"""Records which kernel instance, grid, block and dynamic LDS size a BUILT library launches for a list of conv / GEMM calls and
whole trunk forwards, under every dispatch switch setting (CPU only: tools/launch_log.cpp stands in for the HIP runtime):

    EC_AMD_LIB=/path/to/libec_amd.so python tests/golden/make_conv_routes_golden.py      (from the repository root)

  tests/golden/conv_routes_golden.json   kernel names once (`kernels`; the first `registered_conv_igemm` of them are the
                                         conv_igemm instances the library registers), every distinct launch once (`launches`:
                                         kernel index, LDS bytes, block x, grid x, then grid y z / block y z unless all 1), every
                                         distinct launch sequence once (`seqs`: return code, then launch indices -- or {base, set}:
                                         sequence `base` with the launches at the positions in `set` replaced); per setting the
                                         sequence index of each case -- in full for `default`, only where it differs for the others

The committed table was written by the library of commit d571d96, the commit BEFORE the host side of csrc/rn50.hip (the trunk
executor's plan builder and runner) was rebuilt around block forms, op parts and one route function per op kind; every
(setting, case) pair of the table before it (written by commit 6f7d5da, the commit before the host side of csrc/conv_igemm.hip
was rebuilt) decodes to the same launches in this one.  tests/test_conv_routes.py holds every later build to it, launch for
launch.  The library reads its switches once per process: one recorder process per setting."""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
GOLDEN = os.path.join(HERE, "conv_routes_golden.json")
PARENT_COMMIT = "d571d96"
ENGINE_MIN_TILES = 50          # what clip_preprocessors.py sets on a worker's two encoder handles

SETTINGS = {
    "default": {},
    "big0": {"EC_CONV_BIG": "0"}, "big4": {"EC_CONV_BIG": "4"},
    "bn128_off": {"EC_CONV8_BN128": "-1"}, "big4_bn128": {"EC_CONV_BIG": "4", "EC_CONV8_BN128": "1"},
    "longseg0": {"EC_CONV8_LONGSEG": "0"}, "big4_longseg0": {"EC_CONV_BIG": "4", "EC_CONV8_LONGSEG": "0"},
    "t224_0": {"EC_CONV_T224": "0"}, "t224_1": {"EC_CONV_T224": "1"}, "t224_3": {"EC_CONV_T224": "3"},
    "t64_0": {"EC_CONV_T64": "0"},
    "ring0": {"EC_CONV_RING": "0"}, "ring2": {"EC_CONV_RING": "2"},
    "regw0": {"EC_CONV_REGW": "0"},
    "min_tiles50": {"EC_CONV8_MIN_TILES": "50"},
    "vit_wide0": {"EC_VIT_WIDE": "0"}, "vit_wide2": {"EC_VIT_WIDE": "2"},
    "vit_bm192_0": {"EC_VIT_BM192": "0"},
    # the trunk plan's switches (csrc/rn50.hip): each alone, the fully plain plan, the bottleneck fusion without both of its parts
    "fuse0": {"EC_RN50_FUSE": "0"}, "bneck0": {"EC_RN50_BNECK": "0"}, "bneck2": {"EC_RN50_BNECK": "2"},
    "bneck3_0": {"EC_RN50_BNECK3": "0"}, "img3_0": {"EC_RN50_IMG3": "0"}, "dscat0": {"EC_RN50_DSCAT": "0"},
    "poolout0": {"EC_RN50_POOLOUT": "0"},
    "plain": {"EC_RN50_FUSE": "0", "EC_RN50_DSCAT": "0", "EC_RN50_BNECK": "0"},
    "bneck3_0_img3_0": {"EC_RN50_BNECK3": "0", "EC_RN50_IMG3": "0"},
}

# Instance names as the test writes them: 8-wave kernel c8<BN, KS, POOL, ABL, X3, S2, BM, XP>, 4-wave kernel
# c4<BM, BN, WM, WN, KS, POOL, PF, MV, NS, ILV, S2>.
C8 = "conv_igemm8_kernel<%s>"
C4 = "conv_igemm_kernel<%s>"

# (setting, rule, command, instance the rule must launch).  One line per rule of the route choice and per side of each of its
# tile-count thresholds; `rule` names are those of conv_route() in csrc/conv_igemm.hip.  conv: B H W Cin Cout ks pool act res ldo;
# s2: B H W Cin Cout ks act res; gemm: M N K act res; x3: M N K act.  16 x 16 maps make a frame one 256-row tile.
EXPECT = [
    # ---- stride 1, EC_CONV_BIG = 1: the 8-wave rules (min tiles 150 unless the setting says 50) ----
    ("default", "c8_3x3_wide", "conv 150 16 16 256 256 3 0 1 0 0", C8 % "256, 3, false, 0, false, false, 256, 3"),
    ("default", "c8_3x3_wide", "conv 256 14 14 512 512 3 1 1 0 0", C8 % "256, 3, true, 0, false, false, 256, 3"),
    ("default", "c8_3x3_few_wide", "conv 149 16 16 256 256 3 0 1 0 0", C8 % "128, 3, false, 512, false, false, 256, 3"),
    ("default", "c8_3x3_few_wide", "conv 75 16 16 256 256 3 0 1 0 0", C8 % "128, 3, false, 512, false, false, 256, 3"),
    ("default", "tile128", "conv 74 16 16 256 256 3 0 1 0 0", C4 % "128, 128, 2, 2, 3, false, false, 128, 0, false, false"),
    ("min_tiles50", "c8_3x3_lowfill", "conv 99 16 16 256 256 3 0 1 0 0", C8 % "128, 3, false, 512, false, false, 256, 3"),
    ("min_tiles50", "c8_3x3_lowfill", "conv 50 16 16 256 256 3 0 1 0 0", C8 % "128, 3, false, 512, false, false, 256, 3"),
    ("min_tiles50", "c8_3x3_wide", "conv 100 16 16 256 256 3 0 1 0 0", C8 % "256, 3, false, 0, false, false, 256, 3"),
    ("min_tiles50", "c8_3x3_few_wide", "conv 49 16 16 256 256 3 0 1 0 0", C8 % "128, 3, false, 512, false, false, 256, 3"),
    ("default", "c8_3x3_c128", "conv 300 16 16 128 128 3 0 1 0 0", C8 % "128, 3, false, 512, false, false, 256, 3"),
    ("default", "c8_3x3_c128", "conv 128 28 28 128 128 3 1 1 0 0", C8 % "128, 3, true, 512, false, false, 256, 3"),
    ("longseg0", "c8_3x3_c128", "conv 128 28 28 128 128 3 1 1 0 0", C8 % "128, 3, true, 0, false, false, 256, 3"),
    ("default", "tile128", "conv 299 16 16 128 128 3 0 1 0 0", C4 % "128, 128, 2, 2, 3, false, false, 128, 0, false, false"),
    ("bn128_off", "tile128", "conv 300 16 16 128 128 3 0 1 0 0", C4 % "128, 128, 2, 2, 3, false, false, 128, 0, false, false"),
    ("min_tiles50", "c8_1x1_lowfill", "gemm 6400 768 3072 0 1", C8 % "128, 1, false, 512, false, false, 256, 3"),
    ("default", "tile128", "gemm 6400 768 3072 0 1", C4 % "128, 128, 2, 2, 1, false, false, 128, 0, false, false"),
    ("default", "c8_1x1_res_lowfill", "gemm 6400 768 768 0 1", C8 % "128, 1, false, 512, false, false, 256, 3"),
    ("longseg0", "c8_1x1_res_lowfill", "gemm 6400 768 768 0 1", C8 % "128, 1, false, 0, false, false, 256, 3"),
    ("default", "tile128", "gemm 6144 768 768 0 1", C4 % "128, 128, 2, 2, 1, false, false, 128, 0, false, false"),
    ("default", "tile128", "gemm 25600 256 1024 0 1", C4 % "128, 128, 2, 2, 1, false, false, 128, 0, false, false"),
    ("default", "c8_1x1_wide", "gemm 12800 2304 768 0 0", C8 % "256, 1, false, 0, false, false, 256, 3"),
    ("default", "tile128", "gemm 12800 2304 704 0 0", C4 % "128, 128, 2, 2, 1, false, false, 128, 0, false, false"),
    ("default", "c8_1x1_wide", "gemm 50176 512 2048 1 1", C8 % "256, 1, false, 0, false, false, 256, 3"),
    ("default", "c8_1x1_wide", "gemm 12544 2048 512 1 1", C8 % "256, 1, false, 0, false, false, 256, 3"),
    ("default", "c8_1x1_few_wide", "gemm 12544 512 2048 1 0", C8 % "128, 1, false, 512, false, false, 256, 3"),
    ("big0", "tile128", "conv 150 16 16 256 256 3 0 1 0 0", C4 % "128, 128, 2, 2, 3, false, false, 128, 0, false, false"),
    # ---- stride 1, EC_CONV_BIG = 4 ----
    ("big4", "c8_all_wide", "conv 64 28 28 512 256 1 1 1 0 0", C8 % "256, 1, true, 0, false, false, 256, 3"),
    ("big4", "c8_all_narrow", "conv 64 28 28 512 128 1 1 1 0 0", C8 % "128, 1, true, 512, false, false, 256, 3"),
    ("big4_bn128", "c8_all_narrow", "conv 64 28 28 512 256 1 1 1 0 0", C8 % "128, 1, true, 512, false, false, 256, 3"),
    ("big4_longseg0", "c8_all_narrow", "conv 64 28 28 512 128 1 1 1 0 0", C8 % "128, 1, true, 0, false, false, 256, 3"),
    ("big4", "tile128_ring", "conv 31 16 16 256 512 3 0 1 0 0", C4 % "128, 128, 2, 4, 3, false, false, 128, 3, true, false"),
    ("big4", "c8_all_wide", "conv 32 16 16 256 512 3 0 1 0 0", C8 % "256, 3, false, 0, false, false, 256, 3"),
    # ---- stride 1: the 4-wave kernel's tiles ----
    ("default", "t224", "conv 256 14 14 192 256 3 0 1 0 0", C4 % "224, 128, 1, 4, 3, false, false, 196, 0, false, false"),
    ("big0", "t224", "conv 256 14 14 1024 256 1 0 1 0 0", C4 % "224, 128, 1, 4, 1, false, false, 196, 0, false, false"),
    ("t224_0", "tile128", "conv 256 14 14 192 256 3 0 1 0 0", C4 % "128, 128, 2, 2, 3, false, false, 128, 0, false, false"),
    ("default", "tile128", "conv 128 14 14 192 256 3 0 1 0 0", C4 % "128, 128, 2, 2, 3, false, false, 128, 0, false, false"),
    ("t224_3", "t224", "conv 128 14 14 192 256 3 0 1 0 0", C4 % "224, 128, 1, 4, 3, false, false, 196, 0, false, false"),
    ("t224_1", "t224", "conv 1 14 14 192 256 3 0 1 0 0", C4 % "224, 128, 1, 4, 3, false, false, 196, 0, false, false"),
    ("default", "tile64", "conv 32 7 7 512 512 3 0 1 0 0", C4 % "64, 64, 2, 2, 3, false, false, 64, 4, true, false"),
    ("default", "tile64", "gemm 9472 256 512 0 0", C4 % "64, 64, 2, 2, 1, false, false, 64, 4, true, false"),
    ("ring0", "tile64", "conv 32 7 7 512 512 3 0 1 0 0", C4 % "64, 64, 2, 2, 3, false, false, 64, 0, false, false"),
    ("ring0", "tile64", "gemm 9472 256 512 0 0", C4 % "64, 64, 2, 2, 1, false, false, 64, 0, false, false"),
    ("t64_0", "tile128_ring", "gemm 9472 256 512 0 0", C4 % "128, 128, 2, 4, 1, false, false, 128, 3, true, false"),
    ("default", "tile128_ring", "gemm 9600 256 512 0 0", C4 % "128, 128, 2, 4, 1, false, false, 128, 3, true, false"),
    ("default", "tile128_ring", "gemm 16384 256 512 0 0", C4 % "128, 128, 2, 4, 1, false, false, 128, 3, true, false"),
    ("default", "tile128", "gemm 16512 256 512 0 0", C4 % "128, 128, 2, 2, 1, false, false, 128, 0, false, false"),
    ("ring2", "tile128_ring", "gemm 16512 256 512 0 0", C4 % "128, 128, 2, 4, 1, false, false, 128, 3, true, false"),
    ("ring0", "tile128", "gemm 16384 256 512 0 0", C4 % "128, 128, 2, 2, 1, false, false, 128, 0, false, false"),
    ("default", "tile128_ring", "conv 32 14 14 512 128 1 1 1 0 0", C4 % "128, 128, 2, 4, 1, true, false, 128, 3, true, false"),
    ("default", "tile128_ring", "conv 16 28 28 256 256 3 1 1 0 0", C4 % "128, 128, 2, 4, 3, true, false, 128, 3, true, false"),
    ("default", "tile128_prefetch", "gemm 50176 256 64 1 1", C4 % "128, 128, 2, 2, 1, false, true, 128, 0, false, false"),
    ("default", "tile128", "gemm 50176 256 320 1 1", C4 % "128, 128, 2, 2, 1, false, false, 128, 0, false, false"),
    ("default", "tile128", "conv 32 14 14 256 128 1 1 1 0 0", C4 % "128, 128, 2, 2, 1, true, false, 128, 0, false, false"),
    ("default", "tile128", "conv 64 28 28 64 128 3 1 1 0 0", C4 % "128, 128, 2, 2, 3, true, false, 128, 0, false, false"),
    ("default", "tile256x64", "gemm 50176 64 256 1 0", C4 % "256, 64, 4, 1, 1, false, false, 256, 0, false, false"),
    ("default", "tile256x64", "conv 32 28 28 256 64 1 1 1 0 0", C4 % "256, 64, 4, 1, 1, true, false, 256, 0, false, false"),
    ("default", "tile256x64", "conv 32 28 28 128 64 3 0 1 0 0", C4 % "256, 64, 4, 1, 3, false, false, 256, 0, false, false"),
    ("default", "tile256x64", "conv 32 28 28 128 64 3 1 1 0 0", C4 % "256, 64, 4, 1, 3, true, false, 256, 0, false, false"),
    ("default", "tile256x32", "gemm 50176 32 256 1 0", C4 % "256, 32, 4, 1, 1, false, false, 256, 0, false, false"),
    ("default", "tile256x32", "conv 32 28 28 256 32 1 1 1 0 0", C4 % "256, 32, 4, 1, 1, true, false, 256, 0, false, false"),
    ("default", "tile256x32", "conv 32 28 28 128 32 3 0 1 0 0", C4 % "256, 32, 4, 1, 3, false, false, 256, 0, false, false"),
    ("default", "tile256x32", "conv 32 28 28 128 32 3 1 1 0 0", C4 % "256, 32, 4, 1, 3, true, false, 256, 0, false, false"),
    # ---- stride 2 ----
    ("default", "s2_c8_wide", "s2 150 32 32 256 256 3 1 0", C8 % "256, 3, false, 0, false, true, 256, 3"),
    ("default", "s2_c8_wide", "s2 256 28 28 512 1024 1 0 0", C8 % "256, 1, false, 0, false, true, 256, 3"),
    ("default", "s2_c8_narrow", "s2 149 32 32 256 256 3 1 0", C8 % "128, 3, false, 512, false, true, 256, 3"),
    ("default", "s2_c8_narrow", "s2 75 32 32 256 256 3 1 0", C8 % "128, 3, false, 512, false, true, 256, 3"),
    ("longseg0", "s2_c8_narrow", "s2 75 32 32 256 256 3 1 0", C8 % "128, 3, false, 0, false, true, 256, 3"),
    ("default", "s2_c8_narrow", "s2 256 28 28 512 128 1 0 0", C8 % "128, 1, false, 512, false, true, 256, 3"),
    ("longseg0", "s2_c8_narrow", "s2 256 28 28 512 128 1 0 0", C8 % "128, 1, false, 0, false, true, 256, 3"),
    ("min_tiles50", "s2_tile128", "s2 74 32 32 256 256 3 1 0", C4 % "128, 128, 2, 2, 3, false, false, 128, 0, false, true"),
    ("default", "s2_tile128", "s2 256 28 28 512 128 1 0 1", C4 % "128, 128, 2, 2, 1, false, false, 128, 0, false, true"),
    ("big0", "s2_tile128", "s2 150 32 32 256 256 3 1 0", C4 % "128, 128, 2, 2, 3, false, false, 128, 0, false, true"),
    ("big4", "s2_c8_wide", "s2 150 32 32 256 256 3 1 0", C8 % "256, 3, false, 0, false, true, 256, 3"),
    ("default", "s2_tile64", "s2 32 14 14 256 512 3 1 0", C4 % "64, 64, 2, 2, 3, false, false, 64, 4, false, true"),
    ("default", "s2_tile64", "s2 8 14 14 1024 2048 1 0 0", C4 % "64, 64, 2, 2, 1, false, false, 64, 4, false, true"),
    ("ring0", "s2_tile64", "s2 32 14 14 256 512 3 1 0", C4 % "64, 64, 2, 2, 3, false, false, 64, 4, false, true"),
    ("default", "s2_tile128_ring", "s2 32 56 56 128 128 3 1 0", C4 % "128, 128, 2, 4, 3, false, false, 128, 3, true, true"),
    ("default", "s2_tile128_ring", "s2 32 14 14 1024 2048 1 0 0", C4 % "128, 128, 2, 4, 1, false, false, 128, 3, true, true"),
    ("ring0", "s2_tile128_ring", "s2 32 56 56 128 128 3 1 0", C4 % "128, 128, 2, 4, 3, false, false, 128, 3, true, true"),
    ("default", "s2_tile128", "s2 256 56 56 64 128 1 0 0", C4 % "128, 128, 2, 2, 1, false, false, 128, 0, false, true"),
    ("default", "s2_tile256x64", "s2 64 56 56 64 64 3 1 0", C4 % "256, 64, 4, 1, 3, false, false, 256, 0, false, true"),
    ("default", "s2_tile256x64", "s2 64 56 56 256 64 1 0 0", C4 % "256, 64, 4, 1, 1, false, false, 256, 0, false, true"),
    # ---- the policy's compressor GEMM ----
    ("default", "x3", "x3 12544 128 2048 1", C8 % "128, 1, false, 512, true, false, 256, 3"),
    ("longseg0", "x3", "x3 12544 128 2048 1", C8 % "128, 1, false, 0, true, false, 256, 3"),
]
RULES = ["c8_3x3_lowfill", "c8_3x3_wide", "c8_3x3_few_wide", "c8_3x3_c128", "c8_1x1_lowfill", "c8_1x1_res_lowfill", "c8_1x1_wide",
         "c8_1x1_few_wide", "c8_all_wide", "c8_all_narrow", "t224", "tile64", "tile128_ring", "tile128_prefetch", "tile128",
         "tile256x64", "tile256x32", "s2_c8_wide", "s2_c8_narrow", "s2_tile64", "s2_tile128_ring", "s2_tile128", "s2_tile256x64"]

# Further direct calls (no expectation beyond the table): the kernels in front of the tile dispatch, a column-block output,
# calls the entry points refuse.
EXTRA = ["conv 64 28 28 128 512 1 0 1 1 0", "conv 64 28 28 512 256 1 0 1 0 0", "conv 32 56 56 64 64 3 0 1 0 0",
         "conv 64 14 14 1024 512 1 0 1 0 1536", "conv 256 14 14 256 256 3 0 1 0 0", "conv 256 7 7 512 512 3 0 1 0 0",
         "conv 8 14 14 64 48 1 0 1 0 0", "conv 8 15 14 64 64 3 1 1 0 0", "conv 8 14 14 64 64 1 0 2 1 0", "s2 8 14 14 64 32 1 0 0",
         "s2 8 14 14 64 64 1 2 0", "gemm 100 64 4 0 0", "x3 100 64 64 0"]
FRAMES = [1, 32, 64, 128, 256]
TRUNKS = ["trunk %s %d %d" % (k, f, m) for k in ("clip50", "tv50", "tv18", "vitb32") for f in FRAMES for m in (0, ENGINE_MIN_TILES)]


def tower(kind, layers, frames, width=64, res=224, min_tiles=0, chunk=0, inp="f32"):
    return "tower %s %d %d %d %d %d %d %d %d %d %s" % (kind, width, *layers, res, frames, min_tiles, chunk, inp)


# Both sides of every route decision of the trunk executor (csrc/rn50.hip): an odd frame count (the layer-2 pair launch refuses
# it: two convs), the image-resident 3x3 limits (16 pooled, 32 at 14x14x256, 64 at 7x7x512), the pooled-output conv3 (an even
# count from 42 on), the fused bottleneck's 128 frames, the BasicBlock tail's 32; the engine's min-tiles, a ragged last chunk,
# the u8 and depth stems (a 7x7-stem tower refuses depth frames: the return code is the record), RN50x16, the test-sized towers.
L50, L18, L34, LX16, L1 = (3, 4, 6, 3), (2, 2, 2, 2), (3, 4, 6, 3), (6, 8, 18, 8), (1, 1, 1, 1)
TOWERS = ([tower("clip", L50, f) for f in (3, 16, 17, 32, 33, 40, 42, 64, 65, 127, 128)] +
          [tower("clip", L50, 128, min_tiles=ENGINE_MIN_TILES), tower("clip", L50, 5, chunk=2),
           tower("clip", L50, 3, inp="u8"), tower("clip", L50, 3, inp="depth")] +
          [tower("clip", LX16, f, width=96, res=384) for f in (2, 32)] +
          [tower(k, L1, 2, res=64) for k in ("clip", "tvb", "tvbasic")] +
          [tower("tvb", L50, 3), tower("tvb", L50, 33), tower("tvb", L50, 3, inp="depth")] +
          [tower("tvbasic", l, f) for l in (L18, L34) for f in (3, 32, 33, 128)])
CASES = list(dict.fromkeys([c for _s, _r, c, _k in EXPECT] + EXTRA + TRUNKS + TOWERS))

# conv_igemm instances that only a call the recorder cannot make reaches (library-internal C++ entry points): instance -> that call
UNRECORDED = {
    C8 % "128, 1, false, 512, true, false, 256, 2": "ec_gemm_bf16a_xp(planes = 2): policy.hip's learn pass under EC_POLICY_FAST",
    C8 % "128, 1, false, 0, true, false, 256, 2": "ec_gemm_bf16a_xp(planes = 2) with EC_CONV8_LONGSEG=0",
}


def short(name):
    return name.replace("(anonymous namespace)::", "").replace("void ", "", 1).replace("(ConvArgs)", "")


def build_recorder(outdir, cxx=None):
    exe = os.path.join(outdir, "launch_log")
    subprocess.run([cxx or os.environ.get("CXX", "c++"), "-O1", "-std=c++17", "-rdynamic", "-o", exe,
                    os.path.join(ROOT, "tools", "launch_log.cpp"), "-ldl"], check=True)
    return exe


def record(exe, lib, env_over, extra_args=()):
    """-> (registered kernel names, {case: (rc, [(kernel, gx, gy, gz, bx, by, bz, lds[, args])])})"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("EC_")}
    env.update(env_over)
    r = subprocess.run([exe, lib, *extra_args], input="".join(c + "\n" for c in CASES), capture_output=True, text=True, env=env,
                       timeout=600)
    assert r.returncode == 0, r.stderr
    registered, out, cur = [], {}, None
    for line in r.stdout.splitlines():
        tag, rest = line[0], line[2:]
        if tag == "K":
            registered.append(short(rest))
        elif tag == "C":
            cur = rest
            out[cur] = [None, []]
        elif tag == "L":
            f = rest.split("|")
            out[cur][1].append((short(f[0]), *map(int, f[1].split(",")), *map(int, f[2].split(",")), int(f[3]), *f[4:]))
        elif tag == "R":
            out[cur][0] = int(rest)
    assert list(out) == CASES
    return sorted(registered), {c: (rc, ls) for c, (rc, ls) in out.items()}


def is_conv_igemm(name):
    return name.startswith("conv_igemm")


def decode(table, setting):
    """the table's launches of `setting`: {case: (rc, [launch tuples])}"""
    idx = list(table["settings"]["default"]["seq"])
    for i, s in table["settings"][setting].get("diff", {}).items():
        idx[int(i)] = s

    def seq(i):
        s = table["seqs"][i]
        if isinstance(s, dict):
            s, repl = seq(s["base"]), s["set"]
            for pos, launch in zip(repl[0::2], repl[1::2]):
                s[1 + pos] = launch
        return list(s)

    def launch(j):
        k, lds, bx, gx, *rest = table["launches"][j]
        gy, gz, by, bz = rest or (1, 1, 1, 1)
        return (table["kernels"][k], gx, gy, gz, bx, by, bz, lds)

    return {case: (seq(si)[0], [launch(j) for j in seq(si)[1:]]) for case, si in zip(table["cases"], idx)}


def encode_seq(seq, earlier):
    """`seq` as a list, or as the earlier sequence of the same length that differs in the fewest launches + the replacements"""
    best = None
    for i, e in enumerate(earlier):
        if len(e) == len(seq) and e[0] == seq[0]:
            d = [x for p, (a, b) in enumerate(zip(e[1:], seq[1:])) if a != b for x in (p, b)]
            if best is None or len(d) < len(best[1]):
                best = (i, d)
    return {"base": best[0], "set": best[1]} if best and len(best[1]) + 4 < len(seq) else list(seq)


if __name__ == "__main__":
    import tempfile
    sys.path.insert(0, ROOT)
    from embodied_clip_amd import _lib  # noqa: E402
    kernels, launches, seqs = {}, {}, {}

    def launch_key(l):
        k, gx, gy, gz, bx, by, bz, lds = l
        return (kernels[k], lds, bx, gx) + ((gy, gz, by, bz) if (gy, gz, by, bz) != (1, 1, 1, 1) else ())
    table = {"parent_commit": PARENT_COMMIT, "cases": CASES, "settings": {}}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_recorder(tmp)
        for name, env in SETTINGS.items():
            registered, got = record(exe, _lib.LIB_PATH, env)
            if name == "default":
                table["registered_conv_igemm"] = sum(is_conv_igemm(k) for k in registered)
                kernels.update((k, i) for i, k in enumerate(k for k in registered if is_conv_igemm(k)))
            idx = []
            for c in CASES:
                rc, ls = got[c]
                for l in ls:
                    kernels.setdefault(l[0], len(kernels))
                seq = (rc,) + tuple(launches.setdefault(launch_key(l), len(launches)) for l in ls)
                idx.append(seqs.setdefault(seq, len(seqs)))
            if name == "default":
                table["settings"][name] = {"env": env, "seq": idx}
            else:
                base = table["settings"]["default"]["seq"]
                table["settings"][name] = {"env": env, "diff": {str(i): s for i, s in enumerate(idx) if s != base[i]}}
    table["kernels"], table["launches"], table["seqs"] = list(kernels), [list(l) for l in launches], [encode_seq(s, list(seqs)[:i]) for i, s in enumerate(seqs)]
    json.dump(table, open(GOLDEN, "w"), indent=0, separators=(",", ":"))
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes from", _lib.LIB_PATH, "-", len(CASES), "cases,", len(launches),
          "distinct launches,", len(seqs), "distinct sequences")

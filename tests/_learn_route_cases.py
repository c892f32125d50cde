"""The routes of the learn pass of the policy -- the forward with for_backward=1, then ec_policy_backward* in the same workspace
(make_plan() in csrc/policy.hip) -- as one table of cases that three tests share:

  tests/test_learn_routes.py       (no GPU)  the launch sequence of every case contains the kernel instances its route labels
                                             name and none of the instances of that stage's other labels
  tests/test_learn_route_ref.py    (no GPU)  the bounds of the GPU test admit the fp32 oracle and reject named wrong versions
  tests/test_gpu_learn_routes.py   (GPU)     outputs and every gradient tensor of every case against the float64 oracle

Plain data, no torch.  A case: `cfg` (what differs from the reference config REF of tests/_act_route_cases.py), T, N, `bf16`
(feature dtype), `dhf` (the backward gets a dh_final tensor; else NULL), `route` (one label per stage, ROUTE_STAGES order,
written `c1/tail/wih/step/dw/dw1/bias/heads`), `env` (the name of a SETTINGS entry; the library reads its switches once per
process), `base` (the default-setting case whose shape, inputs and float64 reference this one shares; its own name for a
default case) and `repeat` (two runs must be bit-equal: marked only where the code promises it -- `p.ordered` handles, and the
perm / fused-tail / fused-step reference route the engine's bit-identical rollout test relies on).  Every case is the smallest
shape that still reaches its route: rows = T * N * spatial^2.  GRU handles with goal ids or coordinate goals; LSTM handles,
previous-action embeddings and fusion=1 have suites of their own."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _act_route_cases import REF  # noqa: E402

# stage -> label -> the kernel instances the recorded forward + backward of a case with that label must contain.  A label's
# instances are required; the instances of the stage's other labels that are not also its own are forbidden.  A name without
# template arguments stands for every instance of that template.
#   tail   fused: both directions in one pass;  fwdonly: fused forward, GEMM backward;  gemm: GEMMs both ways;  ...vec: coordinate goals
#   step   f16: the 16-tile kernels of H = 512;  f32: the 32-tile kernels;  ...g: that forward with the gate + GEMM backward;
#          gates: GEMM + gate kernel both ways
#   dw     t: two transposes in front of each of the GRU's two weight-gradient GEMMs -- transpose_f32_kernel also serves W_hh^T
#          (fused backward step) and the re-ordered weight_ih (perm), so its launches are counted: transposes()
ROUTE_STAGES = ("c1", "tail", "wih", "step", "dw", "dw1", "bias", "heads")
PINGPONG = ("conv_igemm8_kernel<128, 1, false, 512, true, false, 256, 2>",      # EC_POLICY_FAST: two planes of W1
            "conv_igemm8_kernel<128, 1, false, 512, true, false, 256, 3>")
ROUTE_KERNELS = {
    "c1": {"pingpong": ["conv_igemm8_kernel"], "plain": []},                    # (the instance: pingpong_instance())
    "tail": {"fused": ["tail_fwd_kernel<false>", "tail_bwd_kernel<false>", "tail_bwd_reduce_kernel", "tail_bwd_fold_kernel"],
             "fwdonly": ["tail_fwd_kernel<false>"], "gemm": [],
             "fusedvec": ["tail_fwd_kernel<true>", "tail_bwd_kernel<true>", "seg_fold_kernel", "tail_bwd_reduce_kernel", "tail_bwd_fold_kernel"],
             "gemmvec": ["frame_sum_kernel"]},
    "wih": {"perm": ["permute_row_kernel"], "plain": ["to_cmajor_kernel", "from_cmajor_kernel"]},
    "step": {"f16": ["gru_step_fwd512_kernel", "gru_step_bwd512_kernel"], "f16g": ["gru_step_fwd512_kernel"],
             "f32": ["gru_step_fwd_kernel", "gru_step_bwd_kernel"], "f32g": ["gru_step_fwd_kernel"], "gates": ["gru_gates_fwd_kernel"]},
    "dw": {"t": [], "n": []},
    "dw1": {"planes": ["dw_tn_x3_kernel", "dw_reduce_kernel"], "gemm": []},               # (ec_dw_tn_xp; <2> / <3>: the planes of W1)
    "bias": {"c4": ["colsum4_kernel"], "c1": []},
    "heads": {"narrow": [], "wide": ["wa_heads_pack_kernel", "wa_heads_unpack_add_kernel"]},
}
FUSED_BWD = ("f16", "f32")            # step labels whose backward is one fused launch per step below T - 1
GATE_BWD = ("f16g", "f32g", "gates")
FUSED_TAIL_BWD = ("fused", "fusedvec")

_FAST0 = {"EC_POLICY_FAST": "0"}
SETTINGS = {
    "default": {},                                      # EC_POLICY_FAST=1: two planes of W1, three of the six bf16x3 products
    "exact": dict(_FAST0),
    "tail_fused0": dict(_FAST0, EC_TAIL_FUSED="0"),
    "gru_fused0": dict(_FAST0, EC_GRU_FUSED="0"),
    "gru_fused1": dict(_FAST0, EC_GRU_FUSED="1"),
    "wih_perm0": dict(_FAST0, EC_WIH_PERM="0"),
    "dw_t0": dict(_FAST0, EC_DW_TRANSPOSED="0"),
    "dw1_tr0": dict(_FAST0, EC_DW1_TR="0"),
}

CASES = {}


def _case(name, route, N, T, bf16=1, dhf=False, repeat=False, env="default", base=None, **cfg):
    assert name not in CASES and set(cfg) <= set(REF) and env in SETTINGS, name
    labels = dict(zip(ROUTE_STAGES, route.split("/")))
    assert len(route.split("/")) == len(ROUTE_STAGES) and all(labels[s] in ROUTE_KERNELS[s] for s in ROUTE_STAGES), (name, route)
    CASES[name] = dict(cfg=cfg, T=T, N=N, bf16=bf16, dhf=dhf, route=labels, env=env, repeat=repeat, base=base or name)


C128 = dict(in_channels=128)
NARROW = "/n/gemm/c1/narrow"                             # few rows, C % 256 != 0 or too few rows for dW1's planes, A + 1 <= 8

# ---- reference widths (C = 2048, S = 7, H = 512) and the dw1 threshold M49 >= 2048 --------------------------------------------
_case("ref_t2_n21", "plain/fused/perm/f16/n/planes/c1/narrow", 21, 2, dhf=True, repeat=True)      # 2058 rows
_case("ref_t1_n41", "plain/fused/perm/f16g" + NARROW, 41, 1)                                      # 2009 rows; T = 1: no fused backward step
_case("ref_f32_t2_n21", "plain/fused/perm/f16" + NARROW, 21, 2, bf16=0)                           # fp32 features: dW1 through the GEMM
# ---- the recurrence step -----------------------------------------------------------------------------------------------------
_case("h256_t3_n33", "plain/fused/perm/f32" + NARROW, 33, 3, dhf=True, hidden=256, **C128)        # a ragged second actor tile
_case("h768_t2_n5", "plain/fused/perm/f32" + NARROW, 5, 2, hidden=768, **C128)                    # 24 column blocks, three K chunks
_case("h256_t1_n33", "plain/fused/perm/f32g" + NARROW, 33, 1, hidden=256, **C128)                 # T = 1 at a width that would fuse
_case("h96_t3_n33", "plain/fused/perm/f32g" + NARROW, 33, 3, hidden=96, **C128)
_case("h32_t3_n5", "plain/fused/perm/f32g" + NARROW, 5, 3, hidden=32, **C128)
_case("h48_t3_n5", "plain/fused/perm/gates" + NARROW, 5, 3, hidden=48, **C128)                    # H % 32 != 0
_case("h512_nohf", "plain/fused/perm/f16" + NARROW, 19, 3, hidden=512, **C128)                    # dh_final NULL == zeros
# ---- the 1024-row thresholds: dw_t (B >= 1024) and colsum4 (M >= 1024, 3H = 288 >= 256 columns) ------------------------------
_case("b1023", "plain/fwdonly/perm/f32g/n/gemm/c1/narrow", 31, 33, spatial=2, hidden=96, **C128)  # S = 4 < 32: 4092 rows through the GEMM tail
_case("b1024", "plain/fwdonly/perm/f32g/t/gemm/c4/narrow", 32, 32, spatial=2, hidden=96, **C128)  # 4096 rows
# ---- ping-pong size: 36,864 rows, nwg == TB_MAX_WG (the tail reducer's scratch in the dm1 area) ------------------------------
_case("pp_c128", "pingpong/fused/perm/f16/t/gemm/c4/narrow", 32, 32, spatial=6, hidden=512, **C128)
_case("pp_c256", "pingpong/fused/perm/f16/t/planes/c4/narrow", 32, 32, spatial=6, hidden=512, in_channels=256)
# ---- tail variants -----------------------------------------------------------------------------------------------------------
_case("goals16", "plain/fused/perm/f16" + NARROW, 21, 2, num_goals=16, **C128)                    # the dE1 register table is full
_case("goals17", "plain/fwdonly/perm/f16" + NARROW, 21, 2, num_goals=17, **C128)                  # ... and past it, at S = 49
_case("goals1", "plain/fused/perm/f16" + NARROW, 21, 2, num_goals=1, **C128)
_case("hid64", "plain/gemm/perm/f16" + NARROW, 8, 2, compress_hid=64, **C128)                     # not the fused tail's widths
_case("s5", "plain/fwdonly/perm/f16" + NARROW, 8, 2, spatial=5, **C128)                           # 25 pixels: frames straddle the 32-row tiles
# ---- other handle shapes -----------------------------------------------------------------------------------------------------
_case("dual_c256", "plain/fused/plain/f16/n/planes/c1/narrow", 21, 2, in_channels=256, dual=1)    # two streams, from_cmajor with a column offset
_case("vec_t2_n21", "plain/fusedvec/perm/f16" + NARROW, 21, 2, repeat=True, goal_in=2, **C128)
_case("vec_s3", "plain/gemmvec/perm/f16" + NARROW, 33, 2, repeat=True, spatial=3, goal_in=2, **C128)
_case("wide_a9", "plain/fused/perm/f16/n/gemm/c1/wide", 21, 2, repeat=True, num_actions=9, **C128)
_case("wide_a9_s3", "plain/fwdonly/perm/f16/n/gemm/c1/wide", 21, 2, repeat=True, spatial=3, num_actions=9, **C128)   # the ordered goal group sum

DEFAULT_CASES = list(CASES)

# ---- EC_POLICY_FAST=0: route predicates do not read it, so every default case again, same labels ------------------------------
for _n in DEFAULT_CASES:
    _c = CASES[_n]
    _case("exact_" + _n, "/".join(_c["route"][s] for s in ROUTE_STAGES), _c["N"], _c["T"], bf16=_c["bf16"], dhf=_c["dhf"],
          repeat=_c["repeat"], env="exact", base=_n, **_c["cfg"])

# ---- the switches (each with EC_POLICY_FAST=0): the fallbacks a user flips when a fast route misbehaves, on the bases whose
# route the switch changes.  `repeat` only on the ordered handle: the fallbacks of the others split K with float atomics ---------
_SWITCH_ROUTES = {   # setting -> base -> route
    "tail_fused0": {"ref_t2_n21": "plain/gemm/perm/f16/n/gemm/c1/narrow", "vec_t2_n21": "plain/gemmvec/perm/f16/n/gemm/c1/narrow",
                    "pp_c256": "pingpong/gemm/perm/f16/t/gemm/c4/narrow"},
    "gru_fused0": {"ref_t2_n21": "plain/fused/perm/gates/n/planes/c1/narrow", "h256_t3_n33": "plain/fused/perm/gates/n/gemm/c1/narrow"},
    "gru_fused1": {"ref_t2_n21": "plain/fused/perm/f32/n/planes/c1/narrow", "pp_c256": "pingpong/fused/perm/f32/t/planes/c4/narrow"},
    "wih_perm0": {"ref_t2_n21": "plain/fused/plain/f16/n/planes/c1/narrow", "b1024": "plain/fwdonly/plain/f32g/t/gemm/c4/narrow",
                  "vec_t2_n21": "plain/fusedvec/plain/f16/n/gemm/c1/narrow"},
    "dw_t0": {"b1024": "plain/fwdonly/perm/f32g/n/gemm/c4/narrow", "pp_c256": "pingpong/fused/perm/f16/n/planes/c4/narrow"},
    "dw1_tr0": {"ref_t2_n21": "plain/fused/perm/f16/n/gemm/c1/narrow", "pp_c256": "pingpong/fused/perm/f16/t/gemm/c4/narrow"},
}
for _s, _routes in _SWITCH_ROUTES.items():
    for _b, _r in _routes.items():
        _c = CASES[_b]
        _case("%s_%s" % (_s, _b), _r, _c["N"], _c["T"], bf16=_c["bf16"], dhf=_c["dhf"], repeat=_c["repeat"] and _b.startswith("vec"),
              env=_s, base=_b, **_c["cfg"])


def cfg_of(case):
    return dict(REF, **case["cfg"])


def rows_of(case):
    return case["T"] * case["N"] * cfg_of(case)["spatial"] ** 2


def cases_of(setting):
    return [n for n, c in CASES.items() if c["env"] == setting]


def streams_of(case):
    return 1 + cfg_of(case)["dual"]


def pingpong_instance(case):
    """the compressor conv's instance on the ping-pong route: two planes of W1 under EC_POLICY_FAST (the default), else three"""
    return PINGPONG[SETTINGS[case["env"]].get("EC_POLICY_FAST", "1") == "0"]


def transposes(case):
    """transpose_f32_kernel launches of the backward: W_hh^T for a fused backward step, the re-ordered weight_ih in front of
    dx4 = dgi @ W_ih, and two in front of each of the GRU's two weight-gradient GEMMs on the `t` route"""
    r = case["route"]
    return (r["step"] in FUSED_BWD) + (r["wih"] == "perm") + 4 * (r["dw"] == "t")


def check_boundary_cases():
    """the row / actor counts of the boundary cases against the plan's literal thresholds (make_plan() and Bwd::colsum in
    csrc/policy.hip): dw_t B >= 1024; colsum4 M >= 1024 and Ncol >= 256; dw1_planes M49 >= 2048 and C % 256 == 0; tail_bwd
    S >= 32 and num_goals <= TB_MAXG = 16; nwg = min(TB_MAX_WG = 256, ceil(ceil(M49 / 32) / 4)) == TB_MAX_WG"""
    rows = {n: rows_of(CASES[n]) for n in DEFAULT_CASES}
    acts = {n: CASES[n]["T"] * CASES[n]["N"] for n in DEFAULT_CASES}
    assert (acts["b1023"], acts["b1024"]) == (1023, 1024) and (rows["b1023"], rows["b1024"]) == (4092, 4096)
    assert all(3 * cfg_of(CASES[n])["hidden"] >= 256 for n in ("b1023", "b1024"))
    assert (rows["ref_t1_n41"], rows["ref_t2_n21"], rows["ref_f32_t2_n21"]) == (2009, 2058, 2058) and rows["ref_t1_n41"] < 2048 <= rows["ref_t2_n21"]
    assert cfg_of(CASES["ref_t2_n21"])["in_channels"] % 256 == 0 and cfg_of(CASES["pp_c256"])["in_channels"] % 256 == 0
    assert cfg_of(CASES["pp_c128"])["in_channels"] % 256 != 0
    px = {n: cfg_of(CASES[n])["spatial"] ** 2 for n in DEFAULT_CASES}
    assert px["s5"] == 25 and px["b1024"] == 4 and px["vec_s3"] == px["wide_a9_s3"] == 9 and max(px["s5"], px["b1024"], px["vec_s3"]) < 32
    assert px["pp_c128"] == px["pp_c256"] == 36 and 36 >= 32 and px["goals17"] == 49
    assert (cfg_of(CASES["goals16"])["num_goals"], cfg_of(CASES["goals17"])["num_goals"]) == (16, 17)
    assert rows["pp_c128"] == rows["pp_c256"] == 36864 and 32 * 4 * 255 < 36864 and acts["pp_c128"] >= 1024
    assert rows["pp_c128"] >= 256 * 128 > rows_of(dict(CASES["pp_c128"], N=28))      # (the ping-pong conv: M49 >= 256 * 128)
    assert max(rows.values()) == 36864
    assert CASES["h256_t3_n33"]["N"] % 32 == 1 and CASES["h768_t2_n5"]["N"] < 32       # ragged actor tiles of the 32-tile step

"""The inference routes of the policy (make_plan() in csrc/policy.hip), as one table of cases that two tests share:

  tests/test_policy_routes.py      (no GPU)  the launch sequence of every case contains the kernel instance its route label
                                             names and none of the instances of that stage's other routes
  tests/test_gpu_act_routes.py     (GPU)     the numbers of every case against the float64 oracle

Plain data, no torch.  A case: `cfg` (what differs from the reference config REF), T, N, `bf16` (feature dtype), `mode`
("infer": one EC_POLICY_INFER call; "reuse": an EC_POLICY_INFER call that builds the weight-derived tables, then an
EC_POLICY_INFER_REUSE call in the same workspace on new inputs), `route` (one label per stage, ROUTE_STAGES order, written
`c1/tail/wih/gi/step/heads`) and `env` (the name of a SETTINGS entry; the library reads its switches once per process).
Every case is the smallest shape that still reaches its route: rows = T * N * spatial^2."""

REF = dict(in_channels=2048, spatial=7, hidden=512, goal_dims=32, num_goals=12, num_actions=6, compress_hid=128, compress_out=32,
           comb_hid=128, comb_out=32, fusion=0, dual=0, goal_in=0)

# stage -> label -> (what the launch sequence of the recorded call must contain, as kernel-name prefixes).  A label's instances
# are required, the instances of the stage's other labels forbidden.  "z4": a GEMM launch whose grid is 4 deep (the act step's
# split-K partial matrices, EC_GEMM_SPLIT_PARTS) -- the GEMM kernels carry no route in their name, so those are counted.
ROUTE_STAGES = ("c1", "tail", "wih", "gi", "step", "heads")
ROUTE_KERNELS = {
    "c1": {"act18": ["c1_act_kernel<1, 8>"], "act24": ["c1_act_kernel<2, 4>"], "act44": ["c1_act_kernel<4, 4>"],
           "pingpong": ["conv_igemm8_kernel<128, 1, false, 512, true, false, 256, 3>"], "parts": [], "plain": []},
    "tail": {"fused": ["tail_fwd_kernel<false>"], "fusedvec": ["tail_fwd_kernel<true>"], "gemm": []},
    "wih": {"perm": [], "cmajor": ["to_cmajor_kernel"]},          # (perm: permute_row_kernel, in the table-building call only)
    "gi": {"act7": ["gi_act_kernel<7>"], "act8": ["gi_act_kernel<8>"], "parts": [], "plain": []},
    "step": {"fused32": ["gru_step_fwd_kernel"], "gates": ["gru_gates_fwd_kernel"]},
    "heads": {"wave": ["heads_fwd_kernel<8>"], "gemm": []},
}

SETTINGS = {
    "default": {},
    "act_split0": {"EC_ACT_SPLIT": "0"},
    "tail_fused0": {"EC_TAIL_FUSED": "0"},
    "gru_fused0": {"EC_GRU_FUSED": "0"},
    "gru_fused1": {"EC_GRU_FUSED": "1"},
    "wih_perm0": {"EC_WIH_PERM": "0"},
    "c1_pingpong0": {"EC_C1_PINGPONG": "0"},
    "gemm_no_x3": {"EC_GEMM_NO_X3": "1"},
}

CASES = {}


def _case(name, route, N, T=1, bf16=1, mode="infer", env="default", **cfg):
    assert name not in CASES and set(cfg) <= set(REF) and env in SETTINGS and mode in ("infer", "reuse"), name
    labels = dict(zip(ROUTE_STAGES, route.split("/")))
    assert len(labels) == len(ROUTE_STAGES) and all(labels[s] in ROUTE_KERNELS[s] for s in ROUTE_STAGES), (name, route)
    CASES[name] = dict(cfg=cfg, T=T, N=N, bf16=bf16, mode=mode, route=labels, env=env)


ACT = "/fused/perm/act7/fused32/wave"          # the act step at the reference widths, behind the compressor conv
C128 = dict(in_channels=128)

# ---- c1_act_kernel<MBLK, U>, reference widths, bf16, T = 1: 49 N rows; <1,8> up to 2048, <2,4> up to 4096, <4,4> above --------
_case("c1_n1", "act18" + ACT, 1)
_case("c1_n41", "act18" + ACT, 41)                      # 2009 rows
_case("c1_n42", "act24" + ACT, 42)                      # 2058
_case("c1_n83", "act24" + ACT, 83)                      # 4067
_case("c1_n84", "act44" + ACT, 84)                      # 4116
_case("c1_n127", "act44" + ACT, 127)                    # the last workgroup's 3rd / 4th 32-row blocks partly / wholly past M
_case("c1_n128", "act44" + ACT, 128)                    # the production slice
# ---- its K tail: kw = K / 8 per wave, rounds of 16 U ------------------------------------------------------------------------
for _k in (128, 384, 512, 640, 768, 3072):
    _case("c1_k%d_n5" % _k, "act18" + ACT, 5, in_channels=_k)
for _k in (384, 640):                                   # U = 4 meets kw = 48 / 80
    _case("c1_k%d_n90" % _k, "act44" + ACT, 90, in_channels=_k)
# ---- gi_act_kernel<8> (flat % 64 == 0) / <7> ----------------------------------------------------------------------------------
_case("gi8_s2", "act18/fused/perm/act8/fused32/wave", 33, spatial=2, **C128)       # flat 128
_case("gi8_s4", "act18/fused/perm/act8/fused32/wave", 33, spatial=4, **C128)       # flat 512
_case("gi8_s8", "act24/fused/perm/act8/fused32/wave", 33, spatial=8, **C128)       # flat 2048, 2112 rows
_case("gi7_h96", "act18" + ACT, 33, hidden=96, **C128)
_case("gi7_h768", "act18" + ACT, 33, hidden=768, **C128)
_case("gi7_n256", "act44" + ACT, 256, **C128)                                      # B <= 256 ...
_case("gi_parts_n257", "act44/fused/perm/parts/fused32/wave", 257, **C128)         # ... and past it (gi_fold = 4)
# ---- the other compressor routes ---------------------------------------------------------------------------------------------
_case("c1_parts_f32", "parts" + ACT, 8, bf16=0)
_case("c1_parts_k160", "parts" + ACT, 8, in_channels=160)
_case("c1_parts_dual", "parts/fused/cmajor/parts/fused32/wave", 8, in_channels=256, dual=1)
_case("c1_plain_k64", "plain" + ACT, 8, in_channels=64)
_case("rows_n334", "act44/fused/perm/parts/fused32/wave", 334, **C128)             # 16366 rows <= ACT_MAX_ROWS ...
_case("rows_n335", "plain/fused/perm/plain/fused32/wave", 335, **C128)             # ... 16415: c1 plain, weight_ih through the GEMM
_case("c1_pingpong_n669", "pingpong/fused/perm/plain/fused32/wave", 669, **C128)   # 32781 rows >= 256 * 128: 3 planes
# ---- the recurrence step ---------------------------------------------------------------------------------------------------
for _h in (32, 256, 512):                               # (96 and 768: gi7_h96 / gi7_h768 above)
    _case("gru_h%d" % _h, "act18" + ACT, 33, hidden=_h, **C128)
_case("gru_h48", "act18/fused/perm/plain/gates/wave", 33, hidden=48, **C128)       # H % 32 != 0: GEMM + gate kernel, plain gi
_case("gru_n31", "act18" + ACT, 31, **C128)
_case("gru_n32", "act18" + ACT, 32, **C128)
# ---- wider coverage --------------------------------------------------------------------------------------------------------
_case("t3_n37", "act44/fused/perm/parts/fused32/wave", 37, T=3)                    # hs_direct off, h_final copied
_case("heads_a3", "act18" + ACT, 33, num_actions=3, **C128)
_case("heads_a9", "act18/fused/perm/act7/fused32/gemm", 33, num_actions=9, **C128)
_case("vec_c1_n84", "act44/fusedvec/perm/act7/fused32/wave", 84, goal_in=2)
_case("vec_parts_f32", "parts/fusedvec/perm/act7/fused32/wave", 8, bf16=0, goal_in=2)
_case("vec_s3", "plain/gemm/cmajor/parts/fused32/wave", 33, spatial=3, goal_in=2, **C128)   # S < 32: the GEMM tail
_case("tail_gemm_hid64", "plain/gemm/cmajor/parts/fused32/wave", 8, compress_hid=64, **C128)   # not the fused tail's widths: int32 goal ids
# ---- a reuse pair per table-building route -----------------------------------------------------------------------------------
_case("reuse_n37", "act18" + ACT, 37, mode="reuse")
_case("reuse_gi8_s4", "act18/fused/perm/act8/fused32/wave", 33, mode="reuse", spatial=4, **C128)
_case("reuse_parts_f32", "parts" + ACT, 8, bf16=0, mode="reuse")
_case("reuse_n335", "plain/fused/perm/plain/fused32/wave", 335, mode="reuse", **C128)
_case("reuse_dual", "parts/fused/cmajor/parts/fused32/wave", 8, mode="reuse", in_channels=256, dual=1)
_case("reuse_vec_n84", "act44/fusedvec/perm/act7/fused32/wave", 84, mode="reuse", goal_in=2)

# ---- the switches: what each fast route is supposed to equal -------------------------------------------------------------------
SWITCH_BASES = {
    "n37": dict(N=37), "n127": dict(N=127), "s4": dict(N=33, spatial=4, **C128), "dual": dict(N=8, in_channels=256, dual=1),
    "t3": dict(N=37, T=3),
}
_SWITCH_ROUTES = {   # setting -> base -> route
    "act_split0": {"n37": "plain/fused/perm/plain/fused32/wave", "n127": "plain/fused/perm/plain/fused32/wave",
                   "s4": "plain/fused/perm/plain/fused32/wave", "dual": "plain/fused/cmajor/plain/fused32/wave",
                   "t3": "plain/fused/perm/plain/fused32/wave"},
    "tail_fused0": {"n37": "plain/gemm/cmajor/parts/fused32/wave", "n127": "plain/gemm/cmajor/parts/fused32/wave",
                    "s4": "plain/gemm/cmajor/parts/fused32/wave", "dual": "plain/gemm/cmajor/parts/fused32/wave",
                    "t3": "plain/gemm/cmajor/parts/fused32/wave"},
    "gru_fused0": {"n37": "act18/fused/perm/act7/gates/wave", "n127": "act44/fused/perm/act7/gates/wave",
                   "s4": "act18/fused/perm/act8/gates/wave", "dual": "parts/fused/cmajor/plain/gates/wave",
                   "t3": "act44/fused/perm/plain/gates/wave"},
    "gru_fused1": {"n37": "act18" + ACT, "n127": "act44" + ACT, "s4": "act18/fused/perm/act8/fused32/wave",
                   "dual": "parts/fused/cmajor/parts/fused32/wave", "t3": "act44/fused/perm/parts/fused32/wave"},
    "wih_perm0": {"n37": "act18/fused/cmajor/parts/fused32/wave", "n127": "act44/fused/cmajor/parts/fused32/wave",
                  "s4": "act18/fused/cmajor/parts/fused32/wave", "dual": "parts/fused/cmajor/parts/fused32/wave",
                  "t3": "act44/fused/cmajor/parts/fused32/wave"},
    "gemm_no_x3": {"n37": "act18" + ACT, "n127": "act44" + ACT, "s4": "act18/fused/perm/act8/fused32/wave",
                   "dual": "parts/fused/cmajor/parts/fused32/wave", "t3": "act44/fused/perm/parts/fused32/wave"},
}
for _s, _routes in _SWITCH_ROUTES.items():
    for _b, _r in _routes.items():
        _case("%s_%s" % (_s, _b), _r, env=_s, **SWITCH_BASES[_b])
_case("c1_pingpong0_n669", "plain/fused/perm/plain/fused32/wave", 669, env="c1_pingpong0", **C128)


def cfg_of(case):
    return dict(REF, **case["cfg"])


def rows_of(case):
    return case["T"] * case["N"] * cfg_of(case)["spatial"] ** 2


def cases_of(setting):
    return [n for n, c in CASES.items() if c["env"] == setting]


def z4_launches(case):
    """GEMM launches 4 deep in the recorded call: the compressor conv's partial matrices (one launch per encoder stream) and
    the input projection's."""
    r = case["route"]
    return (1 + cfg_of(case)["dual"]) * (r["c1"] == "parts") + (r["gi"] == "parts")

"""CPU: the case list of tests/_policy_gemm_ref.py reaches every registered gemm_f32_kernel / gemm_x3_kernel instance and each case
launches exactly the instance it names (tools/launch_log.cpp's `f32` command against the built library, one recorder process per
setting); the refused combinations return their codes without a launch; the list holds the edges each kernel family must see; the
element-wise bounds bite on the reduced cases: the fp32 emulation of the kernel's arithmetic stays at ratio <= 1 on every element and
every applicable wrong version exceeds the bound at least 4 x somewhere (plane_dropped: fails the relative-L2 plane accounting).
tests/test_gpu_policy_gemm.py holds the kernels to the same bounds."""
import importlib.util
import os
import shutil

import pytest
import torch

import _policy_gemm_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX", "c++")
BITE = 4.0


def _recorder_module():
    spec = importlib.util.spec_from_file_location("make_conv_routes_golden_for_policy_gemm",
                                                  os.path.join(ROOT, "tests", "golden", "make_conv_routes_golden.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    return g


@pytest.fixture(scope="module")
def recorded(tmp_path_factory):
    """{setting: (registered gemm instances, {command: (rc, launches)})}: this module's own copy of the recorder module, its command
    list replaced by the setting's cases and the refused calls."""
    if shutil.which(CXX) is None:
        pytest.skip("host C++ compiler not found")
    from embodied_clip_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), _lib.LIB_PATH
    g = _recorder_module()
    exe = g.build_recorder(str(tmp_path_factory.mktemp("launch_log_policy_gemm")), CXX)
    out = {}
    for setting, env in R.SETTINGS.items():
        g.CASES = list(dict.fromkeys([c["cmd"] for c in R.cases_of(setting)] + [c for s, c, _rc in R.REFUSED if s == setting]))
        registered, got = g.record(exe, _lib.LIB_PATH, env)
        got = {c: (rc, [(R.short(l[0]),) + tuple(l[1:]) for l in ls]) for c, (rc, ls) in got.items()}
        out[setting] = ({R.short(k) for k in registered if R.is_gemm(R.short(k))}, got)
    return out


def test_every_case_launches_the_instance_it_names(recorded):
    for c in R.CASES:
        rc, launches = recorded[c["setting"]][1][c["cmd"]]
        assert rc == 0 and [l[0] for l in launches] == [c["instance"]], (c, rc, launches)
        d = R.shape(c)
        gx, gy, gz = launches[0][1:4]
        assert (gx, gy, gz) == (-(-d["M"] // d["BM"]) * -(-d["N"] // d["BN"]), 1, d["nslices"]), (c, launches)


def test_every_registered_instance_has_a_case(recorded):
    registered = recorded["default"][0]
    assert all(reg == registered for reg, _ in recorded.values())
    named = {c["instance"] for c in R.CASES}
    nf = sum(k.startswith("gemm_f32_kernel<") for k in registered)
    print(f"{len(registered)} gemm instances registered ({nf} fp32 MFMA, {len(registered) - nf} bf16x3), {len(named)} named by cases")
    assert not R.EXEMPT
    assert named == registered, (sorted(named - registered), sorted(registered - named))
    # 4 tiles x 3 operand types on the fp32 MFMA; the 3 tiles launch_x3 is instantiated for x 8 type / layout combinations
    assert (nf, len(registered) - nf) == (12, 24)


def test_refused_combinations_return_their_codes_without_a_launch(recorded):
    for setting, cmd, want in R.REFUSED:
        rc, launches = recorded[setting][1][cmd]
        assert rc == want and launches == [], (cmd, rc, launches)
    d = [R.shape(dict(cmd=c, instance=R.KF % "64, 64, 2, 2, false, false")) for _s, c, _rc in R.REFUSED]
    assert any(x["parts"] and x["splitk"] > x["nk"] for x in d)          # more parts than K-tiles, on either kernel's shapes
    assert {x["K"] % 4 for x in d if x["parts"] and x["splitk"] > x["nk"]} == {0, 2}


def test_settings_are_disjoint_in_commands_and_cover_the_edges():
    """The edges the list must cover, per kernel family (gemm_f32_kernel, gemm_x3_kernel)."""
    assert len({(c["setting"], c["cmd"]) for c in R.CASES}) == len(R.CASES)
    assert set(R.SETTINGS) == {"default", "no_x3"} and R.SETTINGS["default"] == {}
    fam = {"gemm_f32_kernel": [], "gemm_x3_kernel": []}
    for c in R.CASES:
        fam[c["instance"].split("<")[0]].append((c, R.shape(c)))
    assert all(c["setting"] == "default" for c, _d in fam["gemm_x3_kernel"])
    assert {c["setting"] for c, _d in fam["gemm_f32_kernel"]} == {"default", "no_x3"}
    for name, cs in fam.items():
        ds = [d for _c, d in cs]
        live = lambda d: sum(k1 > k0 for k0, k1 in d["slices"])
        assert any(d["M"] % d["BM"] for d in ds) and any(d["N"] % d["BN"] for d in ds) and any(d["K"] % 32 for d in ds), name
        assert {(d["alay"], d["blay"]) for d in ds} >= {("k", "k"), ("k", "n"), ("r", "n")}, name      # NT, NN, TN
        assert any(d["alay"] == "k" and d["sam"] > d["K"] for d in ds), name                           # padded pitch (NaN in it: embed)
        assert any(d["abf"] for d in ds) and any(d["bbf"] for d in ds), name
        assert any(d["ldc"] > d["N"] for d in ds), name
        assert any(d["bias"] and d["relu"] for d in ds), name
        assert any(d["gbias"] and d["gidx"] and d["group"] == 49 for d in ds), name
        assert any(d["gbias"] and not d["gidx"] for d in ds), name
        assert any(d["gbias"] and d["M"] % d["group"] for d in ds), name
        assert any(d["rowscale"] and d["dmask"] and d["acc"] for d in ds), name
        assert any(d["relu"] and d["rowscale"] for d in ds), name
        assert any(d["atomic"] and d["bias"] and d["gbias"] and live(d) < d["nslices"] for d in ds), name
        assert any(d["atomic"] and (d["nk"], d["nslices"]) == (5, 4) for d in ds), name
        assert any(d["parts"] and live(d) < d["nslices"] for d in ds), name
        assert any(d["p3"] for d in ds), name
        assert {c["family"] for c, _d in cs} == {"zm", "pos"}, name
        # the 3PRODUCTS case has an unflagged twin
        for c, d in cs:
            if d["p3"]:
                assert any(o["cmd"] == R.twin_cmd(c) and o["instance"] == c["instance"] for o, _ in cs), c
    x3 = [d for _c, d in fam["gemm_x3_kernel"]]
    f32 = [d for _c, d in fam["gemm_f32_kernel"]]
    # an offset base: the x3 path wants it 16-byte (bf16: 8-byte) aligned, the fp32 kernels take one ELEMENT
    assert any(d["aoff"] == 16 and not d["abf"] for d in x3) and any(d["aoff"] == 8 and d["abf"] for d in x3)
    assert any(d["aoff"] == 4 and not d["abf"] for d in f32) and any(d["aoff"] == 2 and d["abf"] for d in f32)
    assert any(d["boff"] == 2 and d["bbf"] for d in f32)
    assert any(d["K"] % 4 for d in f32) and any(d["alay"] == "g" for d in f32)
    assert any(d["alay"] == "k" and d["sam"] % 4 for d in f32)
    assert any(min(d["M"], d["N"]) < 32 for d in f32)
    assert any(d["p3"] and not d["abf"] and not d["bbf"] for d in x3)
    # the operands hold what the edges are about
    for c in R.CASES:
        d = R.shape(c)
        if d["dmask"] or d["rowscale"] or d["gidx"]:
            op = R.operands(R.reduced(c))
            if d["dmask"]:
                m = op["dmask"]
                assert bool(((m == 0) & ~torch.signbit(m)).any() and ((m == 0) & torch.signbit(m)).any() and (m < 0).any())
            if d["rowscale"]:
                assert bool((op["rowscale"] < 0).any() and (op["rowscale"] == 0).any())
            if d["gidx"]:
                g = op["gidx"].tolist()
                assert g != sorted(g) and len(set(g)) < len(g)
    assert set(R.WRONG) == {k for c in R.CASES for k in R.wrong_kinds(R.reduced(c))}


def test_embedding_keeps_the_operand_and_fills_the_rest_with_nan():
    for c in R.CASES:
        d = R.shape(R.reduced(c))
        if not (d["alay"] == "g" or d["sam"] > d["K"] or d["aoff"] or d["boff"]):
            continue
        op = R.operands(R.reduced(c))
        abuf, ao, bbuf, bo = R.embedded(R.reduced(c), op)
        av = torch.as_strided(abuf, (d["M"], d["K"]), (d["sam"], d["sak"]), ao)
        bv = torch.as_strided(bbuf, (d["K"], d["N"]), (d["sbk"], d["sbn"]), bo)
        assert torch.equal(av.float(), op["a"]) and torch.equal(bv.float(), op["b"])
        assert int(torch.isnan(abuf.float()).sum()) == abuf.numel() - d["M"] * d["K"]
        assert int(torch.isnan(bbuf.float()).sum()) == bbuf.numel() - d["K"] * d["N"]


@pytest.mark.parametrize("i", range(len(R.CASES)), ids=lambda i: "%s-%s" % (R.CASES[i]["setting"], R.CASES[i]["cmd"].replace(" ", "_")))
def test_bound_bites_on_the_reduced_case(i):
    case = R.reduced(R.CASES[i])
    op = R.operands(case)
    ref, bound = R.reference(case, op)
    d = R.shape(case)
    assert ref.shape == bound.shape == ((d["nslices"], d["M"], d["N"]) if d["parts"] else (d["M"], d["N"])) and bool((bound >= 0).all())
    emu = R.emulate(case, op)
    r, at = R.worst_ratio(emu, ref, bound)
    print(f"{case['cmd']}: emulation {r:.3f}")
    assert r <= 1.0, (case["cmd"], r, at)
    kinds = R.wrong_kinds(case)
    assert "operand_transposed" in kinds
    thr = None
    if R.needs_l2(case):
        thr, e6, e3 = R.l2_threshold(case, op, ref)
        print(f"{case['cmd']}: relative L2 of the six-product emulation {e6:.3e}, of the three-product one {e3:.3e}, threshold {thr:.3e}")
        assert e6 < thr < e3 and e3 > 10 * e6           # at least half a decade of room on either side of the threshold
        assert R.rel_l2(emu, ref) < thr
    if d["p3"] and d["x3"]:
        twin = dict(case, cmd=R.twin_cmd(case))
        assert torch.equal(R.operands(twin)["a"], op["a"])
        assert not torch.equal(R.emulate(twin, op), emu)       # the flag is taken: the twin's products differ
    for kind in kinds:
        w = R.wrong(case, kind, op)
        if kind == "plane_dropped":
            e = R.rel_l2(w, ref)
            print(f"{case['cmd']}: {kind} relative L2 {e:.3e} against {thr:.3e}")
            assert e > thr, (case["cmd"], kind, e, thr)
            continue
        r, at = R.worst_ratio(w, ref, bound)
        print(f"{case['cmd']}: {kind} {r:.1f}")
        assert r >= BITE, (case["cmd"], kind, r, at)


@pytest.mark.parametrize("M,NX", [(31, 256), (64, 768), (1017, 256)])
def test_dw_bound_bites(M, NX):
    """dw_reference (ec_dw_tn_x3): the fp32 emulation stays under the bound, every wrong version exceeds it 4 x somewhere.  (At the
    49,017 tokens of the GPU test a single dropped K-tile is of the size of the worst-case accumulation term: the small cases are where
    this bound tells, the existing empirical bound of tests/test_gpu_policy.py holds the large ones.)"""
    op = R.dw_operands(M, NX)
    ns, tok = R.dw_splits(M, NX)
    ref, bound = R.dw_reference(op, ns)
    r, at = R.worst_ratio(R.dw_emulate(op, ns, tok), ref, bound)
    print(f"dw {M} {NX}: {ns} splits of {tok} tokens, emulation {r:.3f}")
    assert r <= 1.0, (M, NX, r, at)
    kinds = [k for k in R.DW_WRONG if (k != "drop_ktile" or M % 32) and (k != "last_split_dropped" or ns > 1)]
    for kind in kinds:
        r, at = R.worst_ratio(R.dw_wrong(op, ns, tok, kind), ref, bound)
        print(f"dw {M} {NX}: {kind} {r:.1f}")
        assert r >= BITE, (M, NX, kind, r, at)


def test_dw_splits_mirror_the_library():
    """dw_splits against ec_dw_tn_x3_splits (a host function), at the sizes the CPU and GPU tests use; every wrong version applies"""
    from embodied_clip_amd import _lib
    lib = _lib.load()
    sizes = [(M, NX) for M in (31, 64, 1017, 1000 * 49 + 17) for NX in (256, 768)]
    for M, NX in sizes:
        assert R.dw_splits(M, NX)[0] == lib.ec_dw_tn_x3_splits(M, NX), (M, NX)
    assert R.dw_splits(31, 256) == (1, 32) and R.dw_splits(1000 * 49 + 17, 768) == (86, 576) and R.dw_splits(1000 * 49 + 17, 256) == (256, 192)
    assert any(M % 32 for M, _ in sizes) and any(R.dw_splits(M, NX)[0] > 1 for M, NX in sizes)

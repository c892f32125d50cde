"""CPU: the case list of tests/_trunk_fused_ref.py reaches every registered instance of the nine fused-kernel templates of
conv3x3_narrow.hip, conv_pair.hip, conv_bneck.hip and conv_basic.hip (but the exempt one), each case launches exactly the
launch sequence it names (tools/launch_log.cpp against the built library, one recorder process per setting), the list has the
edges each kernel needs, and the element-wise bounds bite on the reduced cases: the fp32 / bf16 emulation of the kernel's
arithmetic stays at ratio <= 1 on every element of every output and every applicable wrong version exceeds the bound at least
4 x somewhere.  tests/test_gpu_trunk_fused.py holds the kernels to the same bounds."""
import importlib.util
import os
import shutil

import pytest

import _trunk_fused_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX", "c++")
BITE = 4.0


def _recorder_module():
    spec = importlib.util.spec_from_file_location("make_conv_routes_golden_for_trunk_fused",
                                                  os.path.join(ROOT, "tests", "golden", "make_conv_routes_golden.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    return g


@pytest.fixture(scope="module")
def recorded(tmp_path_factory):
    """{setting: (registered instances of the nine templates, {command: (rc, launched kernels)})}: this module's own copy of the
    recorder module, its command list replaced by the setting's cases (and the line test_gpu_encoder.py's comment is about)."""
    if shutil.which(CXX) is None:
        pytest.skip("host C++ compiler not found")
    from embodied_clip_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), _lib.LIB_PATH
    g = _recorder_module()
    exe = g.build_recorder(str(tmp_path_factory.mktemp("launch_log_trunk_fused")), CXX)
    out = {}
    for setting, env in R.SETTINGS.items():
        g.CASES = list(dict.fromkeys([c["cmd"] for c in R.cases_of(setting)] + ["conv 96 14 14 256 1024 1 0 1 1 0"]))
        registered, got = g.record(exe, _lib.LIB_PATH, env)
        mine = {R.strip_args(k) for k in registered if k.split("<")[0].split("(")[0] in R.TEMPLATES}
        out[setting] = (mine, {c: (rc, [R.strip_args(l[0]) for l in ls]) for c, (rc, ls) in got.items()})
    return out


def test_every_case_launches_the_sequence_it_names(recorded):
    for c in R.CASES:
        rc, launches = recorded[c["setting"]][1][c["cmd"]]
        launches = [l.split("(")[0] if l.startswith(R.PACK) else l for l in launches]
        assert rc == 0 and launches == R.launches_of(c), (c, rc, launches)


def test_every_registered_instance_has_a_case_or_an_exemption(recorded):
    registered = recorded["default"][0]
    assert all(reg == registered for reg, _ in recorded.values())
    named = {c["instance"] for c in R.CASES}
    per = {t: sorted(k for k in registered if k.split("<")[0] == t) for t in R.TEMPLATES}
    print({t: len(v) for t, v in per.items()})
    print(f"{len(registered)} instances registered, {len(named)} mapped to cases, {len(R.EXEMPT)} exempt")
    assert not (named & set(R.EXEMPT))
    assert set(R.EXEMPT) <= registered, sorted(set(R.EXEMPT) - registered)
    assert named <= registered, sorted(named - registered)
    assert registered - named == set(R.EXEMPT), sorted(registered - named - set(R.EXEMPT))
    assert [len(per[t]) for t in R.TEMPLATES] == [5, 5, 4, 7, 1, 4, 3, 2, 2]
    assert (len(named), len(R.EXEMPT)) == (32, 1)
    assert not any("true>" in k for k in per["bneck23_kernel"])        # the tools-only WEMU instance is not in the product library


def test_the_1024_channel_line_of_the_encoder_test_is_not_a_regw_launch(recorded):
    """test_conv_bf16_matches_oracle's (96, 14, 14, 256, 1024) line: 588 tiles and a (K, N) the register-weight kernel has no
    instance for -- it runs on conv_igemm's 128 x 128 residual-prefetch tile (held by tests/test_gpu_conv_tiles.py)."""
    rc, launches = recorded["default"][1]["conv 96 14 14 256 1024 1 0 1 1 0"]
    assert rc == 0 and launches == ["conv_igemm_kernel<128, 128, 2, 2, 1, false, true, 128, 0, false, false>"]


def test_the_case_list_covers_the_edges():
    assert len({(c["setting"], c["cmd"]) for c in R.CASES}) == len(R.CASES)
    assert set(R.SETTINGS) == {c["setting"] for c in R.CASES} and len(R.SETTINGS) == 5
    by = {}
    for c in R.CASES:
        by.setdefault(c["instance"], []).append(R.shape(c))
    for inst, ds in by.items():
        tpl = inst.split("<")[0]
        if tpl in ("conv3x3_rows_kernel", "conv3x3_rowsN_kernel"):
            for d in ds:
                assert d["B"] >= 2 and d["W"] == 56 and d["W"] // d["SEG"] >= 2, inst          # frame borders and segment seams
            if tpl == "conv3x3_rowsN_kernel":
                assert all(d["H"] % d["RT"] == 0 and d["H"] // d["RT"] >= 2 for d in ds), inst
        if tpl == "conv3x3_narrow_kernel":
            for d in ds:
                assert d["W"] % (14 if d["pool"] else 28) and d["M"] % 32 == 0 and d["H"] != d["W"], inst
                assert d["W"] % 32 and (d["H"] * d["W"]) % 32 and d["B"] >= 2, inst            # tiles straddle rows and frames
        if tpl == "conv1x1_regw_kernel":
            assert all(d["nt"] >= 1024 and d["nt"] % 256 for d in ds), inst
        if tpl == "conv3x3_img_kernel":
            assert {d["B"] for d in ds} == {1, 3, 33}, inst
            assert all(d["B"] * d["Cin"] // (32 * d["FN"]) > 256 for d in ds if d["B"] == 33), inst
        if tpl == "bneck23_kernel":
            assert {d["B"] for d in ds} == {1, 3}, inst
    # the row-tile kernel's own fallback: H no multiple of the multi-row tile's RT, under the default setting
    assert any(c["setting"] == "default" and R.shape(c)["H"] % 2 for c in R.CASES if c["instance"] == R.ROWS % "64, 64, false, 6")
    assert any(c["setting"] == "default" and R.shape(c)["H"] % 4 for c in R.CASES if c["instance"] == R.ROWS % "32, 32, false, 16")
    # persistent loops: one case per kernel with more tiles than a sweep of the grid takes, and a ragged rest
    loops = {R.shape(c)["tpl"] for c in R.CASES if R.shape(c)["loops"] and R.shape(c)["nt"] % R.shape(c)["GW"]}
    assert loops == set(R.TEMPLATES[:6]), loops
    assert all(R.shape(c)["K"] <= 576 for c in R.CASES if R.shape(c)["loops"])
    # pair: every (TWO, RES, N2) the entry point takes, the pooled form with >= 2 tile rows / columns / frames, once with y = NULL
    pairs = [R.shape(c) for c in R.CASES if c["instance"].startswith("conv1x1_pair_kernel")]
    assert {(d["two"], d["res"], d["N2"]) for d in pairs if d["kind"] == "pair"} == {(1, 1, 64), (1, 0, 64), (0, 1, 64), (0, 0, 64),
                                                                                    (0, 1, 128), (0, 0, 128)}
    pooled = [d for d in pairs if d["kind"] == "pairpool"]
    assert {d["ystored"] for d in pooled} == {0, 1} and all(d["B"] >= 2 and d["H"] // 4 >= 2 and d["W"] // 8 >= 2 for d in pooled)
    p512 = [R.shape(c) for c in R.CASES if c["instance"] == R.PAIR512]
    assert all((d["K"], d["N"], d["N2"], d["res"]) == (128, 512, 128, 1) for d in p512) and p512
    # img: the pooled geometry also into a column block
    assert any(d["ldo"] > d["N"] for c in R.CASES for d in [R.shape(c)] if d["kind"] == "img" and d["pool"])
    # tail: both tile configurations on either side of the dispatch threshold, a ragged last tile, planes != inplanes
    tails = {R.shape(c)["BM"]: R.shape(c) for c in R.CASES if c["instance"].startswith("basic_tail")}
    assert set(tails) == {128, 64} and tails[128]["B"] == tails[64]["B"] + 1
    assert all(d["M"] % d["BM"] and d["P"] != d["I"] for d in tails.values())
    assert -(-tails[128]["M"] // 128) * (tails[128]["N"] // 128) == 512 and -(-tails[64]["M"] // 128) * (tails[64]["N"] // 128) < 512
    assert {c["family"] for c in R.CASES} == {"zm", "pos", "sum"}
    assert set(R.WRONG) == {k for c in R.CASES for k in R.wrong_kinds(R.reduced(c))}


@pytest.mark.parametrize("i", range(len(R.CASES)), ids=lambda i: "%s-%s" % (R.CASES[i]["setting"], R.CASES[i]["cmd"].replace(" ", "_")))
def test_bound_bites_on_the_reduced_case(i):
    case = R.reduced(R.CASES[i])
    op = R.operands(case)
    emu = R.emulate(case, op)
    refs = R.reference(case, op, emu)
    d = R.shape(case)
    assert set(R.outputs(case)) == set(emu) == set(refs) - {"risk"}
    for o in R.outputs(case):
        ref, bound = refs[o]
        assert ref.shape == bound.shape == emu[o].shape and ref.shape[0] in (d["rows"], d["M"] // 4) and bool((bound >= 0).all())
        r, at = R.worst_ratio(emu[o], ref, bound)
        print(f"{case['cmd']}: emulation {o} {r:.3f}")
        assert r <= 1.0, (case["cmd"], o, r, at)
    if "risk" in refs:
        print(f"{case['cmd']}: share of intermediate elements at risk {refs['risk']:.4f}")
        assert refs["risk"] <= R.RISK_CAP
    kinds = R.wrong_kinds(case)
    assert {"drop_kstep", "bias_n4"} <= set(kinds)
    for kind in kinds:
        w, _ = R.worst_of(case, R.wrong(case, kind, op), op)
        r = max(v for v, _at in w.values())
        print(f"{case['cmd']}: {kind} {r:.3g}")
        assert r >= BITE, (case["cmd"], kind, w)

"""CPU: the case list of tests/_conv_tile_ref.py reaches every registered conv_igemm instance (but the exempt ones) and each case
launches exactly the instance it names (tools/launch_log.cpp against the built library, one recorder process per setting); the
element-wise bounds bite on the reduced cases: the fp32 / bf16 emulation of the kernel's arithmetic stays at ratio <= 1 on every
element and every applicable wrong version exceeds the bound at least 4 x somewhere (the convention of test_vit_stage_ref.py).
tests/test_gpu_conv_tiles.py holds the kernels to the same bounds."""
import importlib.util
import os
import shutil

import pytest

import _conv_tile_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX", "c++")
BITE = 4.0


def _recorder_module():
    spec = importlib.util.spec_from_file_location("make_conv_routes_golden_for_tiles",
                                                  os.path.join(ROOT, "tests", "golden", "make_conv_routes_golden.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    return g


@pytest.fixture(scope="module")
def recorded(tmp_path_factory):
    """{setting: (registered conv_igemm instances, {command: (rc, launches)})}: this module's own copy of the recorder module, its
    command list replaced by the setting's cases."""
    if shutil.which(CXX) is None:
        pytest.skip("host C++ compiler not found")
    from embodied_clip_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), _lib.LIB_PATH
    g = _recorder_module()
    exe = g.build_recorder(str(tmp_path_factory.mktemp("launch_log_tiles")), CXX)
    out = {}
    for setting, env in R.SETTINGS.items():
        g.CASES = list(dict.fromkeys(c["cmd"] for c in R.cases_of(setting)))
        registered, got = g.record(exe, _lib.LIB_PATH, env)
        out[setting] = ({k for k in registered if g.is_conv_igemm(k)}, got)
    return out


def test_every_case_launches_the_instance_it_names(recorded):
    for c in R.CASES:
        rc, launches = recorded[c["setting"]][1][c["cmd"]]
        assert rc == 0 and [l[0] for l in launches] == [c["instance"]], (c, rc, launches)


def test_every_registered_instance_has_a_case_or_an_exemption(recorded):
    registered = recorded["a"][0]
    assert all(reg == registered for reg, _ in recorded.values())
    named = {c["instance"] for c in R.CASES}
    print(f"{len(registered)} conv_igemm instances registered, {len(named)} mapped to cases, {len(R.EXEMPT)} exempt")
    assert not (named & set(R.EXEMPT))
    assert set(R.EXEMPT) <= registered, sorted(set(R.EXEMPT) - registered)
    assert named <= registered, sorted(named - registered)
    assert registered - named == set(R.EXEMPT), sorted(registered - named - set(R.EXEMPT))
    assert (len(named), len(R.EXEMPT)) == (51, 4)


def test_settings_are_disjoint_in_commands_and_cover_the_edges():
    """The edges the list must cover, per kernel family (4-wave conv_igemm_kernel, 8-wave conv_igemm8_kernel)."""
    assert len({(c["setting"], c["cmd"]) for c in R.CASES}) == len(R.CASES)
    fam = {"conv_igemm_kernel": [], "conv_igemm8_kernel": []}
    for c in R.CASES:
        fam[c["instance"].split("<")[0]].append((c, R.shape(c)))
    for name, cs in fam.items():
        plain = [d for _c, d in cs if not d["pool"] and not d["x3"]]
        assert {d["act"] for d in plain} == {0, 1, 2}, name
        assert {(d["act"], bool(d["res"])) for d in plain} >= {(0, True), (1, True), (0, False), (1, False), (2, False)}, name
        assert any(d["pool"] for _c, d in cs), name
        assert any(d["M"] % d["MV"] for _c, d in cs), name
        assert any(d["ldo"] > d["Cout"] for _c, d in cs), name
        assert {c["family"] for c, _d in cs} == {"zm", "pos"}, name
        assert {(d["ks"], d["res"], d["act"]) for _c, d in cs if d["s2"]} >= {(1, 0, 0), (1, 1, 0), (3, 0, 1), (3, 1, 1)}, name
    c4 = [d for _c, d in fam["conv_igemm_kernel"]]
    c8 = [d for _c, d in fam["conv_igemm8_kernel"]]
    assert any(d["M"] % 256 and d["H"] * d["W"] % 256 and d["kind"] == "conv" for d in c8)      # ragged, tiles straddle frames
    assert all(d["M"] % 196 == 0 for d in c4 if d["MV"] == 196) and any(d["MV"] == 196 for d in c4)
    assert any(d["ks"] == 3 and d["Cin"] == 32 for d in c4) and any(d["ks"] == 3 and d["Cin"] == 192 for d in c4)
    assert any(d["kind"] == "gemm" and d["K"] % 64 for d in c4)
    assert any(d["H"] != d["W"] and d["ks"] == 3 for d in c4)
    assert not any(d["res"] and d["act"] == 2 for d in c4 + c8)
    assert set(R.WRONG) == {k for c in R.CASES for k in R.wrong_kinds(R.reduced(c))}


@pytest.mark.parametrize("i", range(len(R.CASES)), ids=lambda i: "%s-%s" % (R.CASES[i]["setting"], R.CASES[i]["cmd"].replace(" ", "_")))
def test_bound_bites_on_the_reduced_case(i):
    case = R.reduced(R.CASES[i])
    op = R.operands(case)
    ref, bound = R.reference(case, op)
    d = R.shape(case)
    assert ref.shape == bound.shape == (d["rows"], d["Cout"]) and bool((bound > 0).all())
    r, at = R.worst_ratio(R.emulate(case, op), ref, bound)
    print(f"{case['cmd']}: emulation {r:.3f}")
    assert r <= 1.0, (case["cmd"], r, at)
    kinds = R.wrong_kinds(case)
    assert {"drop_ktile", "bias_n4"} <= set(kinds)
    for kind in kinds:
        r, at = R.worst_ratio(R.wrong(case, kind, op), ref, bound)
        print(f"{case['cmd']}: {kind} {r:.1f}")
        assert r >= BITE, (case["cmd"], kind, r, at)

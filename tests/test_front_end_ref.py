"""CPU: the case list of tests/_front_end_ref.py reaches every registered instance of the front-end kernels (the stems, the 2 x 2
average pool, the layout kernels, the spatial means, the resize: every __global__ function of _front_end_ref.SOURCES) but the
exempt ones, each case launches exactly the instance it names (tools/launch_log.cpp against the built library), every stem
instance has a vector-staged and a scalar-staged case by the kernels' own rule, the list has the edges each kernel needs, the
rounding conditions the tight references rest on hold, and the element-wise bounds bite: the fp32 / bf16 emulation of each
kernel's arithmetic stays at ratio <= 1 on every element and every applicable wrong version exceeds the bound at least 4 x
somewhere.  tests/test_gpu_front_end.py holds the kernels to the same bounds.  Also here, with never-dereferenced pointers: the
shapes the entry points refuse before any HIP call."""
import importlib.util
import os
import shutil

import pytest
import torch

import _front_end_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX", "c++")
BITE = 4.0
EC_ERR_SHAPE = -2
P = 0x1000          # a non-NULL, 16-byte aligned pointer that is never dereferenced: every call below is refused first


def _recorder_module():
    spec = importlib.util.spec_from_file_location("make_conv_routes_golden_for_front_end",
                                                  os.path.join(ROOT, "tests", "golden", "make_conv_routes_golden.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    return g


@pytest.fixture(scope="module")
def recorded(tmp_path_factory):
    """(registered front-end instances, {command: (rc, launched kernels)}): this module's own copy of the recorder module, its
    command list replaced by the cases."""
    if shutil.which(CXX) is None:
        pytest.skip("host C++ compiler not found")
    from embodied_clip_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), _lib.LIB_PATH
    g = _recorder_module()
    exe = g.build_recorder(str(tmp_path_factory.mktemp("launch_log_front_end")), CXX)
    g.CASES = list(dict.fromkeys(c["cmd"] for c in R.CASES))
    registered, got = g.record(exe, _lib.LIB_PATH, {})
    mine = {R.strip_args(k) for k in registered if k.split("<")[0].split("(")[0] in R.TEMPLATES}
    return mine, {c: (rc, [R.strip_args(l[0]) for l in ls]) for c, (rc, ls) in got.items()}


def test_templates_are_the_kernels_of_the_front_end_sources():
    """A kernel added to one of the four files joins the set the next test accounts for."""
    assert sorted(R.kernels_in_sources(ROOT)) == sorted(R.TEMPLATES)


def test_every_case_launches_the_instance_it_names(recorded):
    for c in R.CASES:
        rc, launches = recorded[1][c["cmd"]]
        assert rc == 0 and launches == [c["instance"]], (c, rc, launches)


def test_every_registered_instance_has_a_case_or_an_exemption(recorded):
    registered = recorded[0]
    named = {c["instance"] for c in R.CASES}
    print(f"{len(registered)} front-end instances registered, {len(named)} mapped to cases, {len(R.EXEMPT)} exempt")
    assert not (named & set(R.EXEMPT))
    assert set(R.EXEMPT) <= registered, sorted(set(R.EXEMPT) - registered)
    assert named <= registered, sorted(named - registered)
    assert registered - named == set(R.EXEMPT), sorted(registered - named - set(R.EXEMPT))
    assert (len(named), len(R.EXEMPT)) == (15, 3)


def test_exemptions_name_tests_that_exist():
    for inst, where in R.EXEMPT.items():
        path, _, name = where.split(" ")[0].partition("::")
        with open(os.path.join(ROOT, path)) as fh:
            assert not name or "def %s(" % name in fh.read(), (inst, where)


def test_every_stem_instance_has_a_vector_and_a_scalar_case():
    by = {}
    for c in R.CASES:
        br = R.staging_branch(c)
        if br is not None:
            by.setdefault(c["instance"], set()).add(br)
    assert len(by) == 9 and all(v == {"vector", "scalar"} for v in by.values()), by        # (`float4`: unreachable, see the module)
    # the depth stem's alignment fallback: a vector shape that stages scalar only because of its pointer
    off = [c for c in R.CASES if c["variant"] == "off1"]
    assert {c["instance"] for c in off} == {R.DSTEM % n for n in (32, 48, 64)}
    assert all(R.staging_branch(c) == "scalar" and R.staging_branch(dict(c, variant="")) == "vector" for c in off)
    # no RGB stem / stem7 case leaves the pointer alignment those kernels need
    assert all(R.shape(c)["off"] == 0 for c in R.CASES if R.shape(c)["kind"] != "dstem")


def test_the_case_list_covers_the_edges():
    assert len({(c["cmd"], c["variant"]) for c in R.CASES}) == len(R.CASES)
    sh = [(c, R.shape(c)) for c in R.CASES]
    for inst in {c["instance"] for c, d in sh if d["kind"] in ("stem", "dstem")}:
        ds = [d for c, d in sh if c["instance"] == inst]
        assert any(d["H"] % 2 and d["W"] % 2 for d in ds) and any(d["H"] % 2 == 0 and d["W"] % 4 == 0 for d in ds), inst
        assert any(d["Ho"] > 16 and d["Wo"] > 16 and d["Ho"] % 16 and d["Wo"] % 16 for d in ds), inst       # 2 x 2 tiles, both ragged
        assert all(d["B"] >= 2 for d in ds), inst
    stems = [(c, d) for c, d in sh if d["kind"] == "stem"]
    for mfma in (True, False):
        assert any((d["H"], d["W"]) == (2, 4) for c, d in stems if d["mfma"] == mfma)                        # one output row, minimal vector row
        assert any(d["W"] % 4 == 2 and R.staging_branch(c) == "scalar" for c, d in stems if d["mfma"] == mfma)
    assert {(d["u8"], c["family"]) for c, d in stems} == {(0, "zm"), (0, "pos"), (1, "zm"), (1, "pos")}
    assert {c["consts"] for c, d in sh if d["u8"]} == set(R.CONSTS)
    assert all(R.shape(c)["mfma"] for c in R.CASES if "trunc" in R.wrong_kinds(c))
    assert any(not d["u8"] and c["family"] == "zm" and d["mfma"] for c, d in stems)                          # trunc on a zero-mean case
    for c, d in sh:
        if d["u8"]:
            x = R.operands(c)["x"]
            assert int(x.min()) == 0 and int(x.max()) == 255, c["cmd"]
    for u8 in (0, 1):
        s7 = [d for c, d in sh if d["kind"] == "stem7" and d["u8"] == u8]
        assert any((d["H"], d["W"]) == (8, 8) for d in s7)
        assert any(d["H"] != d["W"] and d["tiles_x"] > 1 and d["tiles_y"] > 1 and d["Ho"] % R.TPH7 and d["Wo"] % R.TPW7 for d in s7)
        assert any(R.GRID7 < d["ntiles"] < 2 * R.GRID7 for d in s7)                                          # some workgroups run a second tile
    assert all(bool((R.operands(c)["bias"] > 0).any()) for c, d in sh if d["kind"] == "stem7")
    dst = [(c, d) for c, d in sh if d["kind"] == "dstem"]
    assert all(any(c["affine"] == (4.0, -2.0) for c, d in dst if c["instance"] == i) for i in {c["instance"] for c, d in dst})
    avg = [d for c, d in sh if d["kind"] == "avgpool"]
    assert any(d["vectors"] > R.AVG_SWEEP and d["vectors"] % R.AVG_SWEEP for d in avg)                       # the grid-stride loop, ragged
    assert any(d["ldo"] > d["Cout"] + R.COL0 for d in avg) and any(d["ldo"] == d["Cout"] for d in avg)
    for k in ("tonchw", "tonhwc"):
        hw = {d["HW"] for c, d in sh if d["kind"] == k}
        assert {1, 49, 252} <= hw and 252 * 65 * 4 <= R.LDS_LIMIT < 253 * 65 * 4, k
        assert any(d["C"] > 64 and d["B"] > 1 for c, d in sh if d["kind"] == k)                              # more than one slab and frame
    mean = [d for c, d in sh if d["kind"] == "mean"]
    assert any(d["HW"] == 1 for d in mean) and any(d["C"] % 8 for d in mean) and any(d["B"] * d["C"] > 256 for d in mean)
    assert set(R.WRONG) == {k for c in R.CASES for k in R.wrong_kinds(R.reduced(c))}
    assert [c["cmd"] for c in R.CASES if "stale_patch" in R.wrong_kinds(c)] == ["stem7 65 128 8 0", "stem7 65 128 8 1"]


@pytest.mark.parametrize("name", list(R.CONSTS))
def test_uint8_affine_rounds_to_one_bf16_fused_or_not(name):
    """The tight reference of the uint8 cases needs it: all 768 (channel, byte value) pairs but the excluded ones."""
    bad = R.u8_rounding_condition(name)
    excluded = R.U8_EXCLUDED.get(name, [])
    assert len(excluded) <= 4 and set(bad) <= set(excluded), (name, bad)
    for c in R.CASES:
        if c["consts"] == name:
            x = R.operands(c)["x"]
            assert not any(bool((x[..., ch] == u).any()) for ch, u in excluded), c["cmd"]


def test_uint8_condition_fails_for_a_set_that_needs_it():
    """The check can fail: the ad-hoc set mean (0.1, 0.5, 0.9), std (0.2, 0.5, 1.0) has one byte value that rounds two ways."""
    R.CONSTS["adhoc"] = ((0.1, 0.5, 0.9), (0.2, 0.5, 1.0))
    try:
        assert R.u8_rounding_condition("adhoc") == [(1, 127)]
    finally:
        del R.CONSTS["adhoc"]


def test_depth_affines_are_exact():
    ds = [c for c in R.CASES if R.shape(c)["kind"] == "dstem"]
    assert len(ds) == 9 and all(R.depth_affine_exact(c) for c in ds)
    assert not R.depth_affine_exact(dict(ds[0], affine=(0.3, -2.0)))


def test_entry_points_refuse_what_they_cannot_launch():
    """Before any HIP call: HW = 253 is past the layout kernels' 64 KiB of LDS (252 is the last that fits); a stem grid past
    2^31 - 1 workgroups."""
    from embodied_clip_amd import _lib
    lib = _lib.load()
    assert lib.ec_nhwc_bf16_to_nchw_f32(P, P, 1, 253, 192, 0) == EC_ERR_SHAPE
    assert lib.ec_nchw_f32_to_nhwc_bf16(P, P, 1, 253, 192, P, 0) == EC_ERR_SHAPE
    assert lib.ec_nhwc_bf16_to_nchw_f32(P, P, 1, 252, 100, 0) == EC_ERR_SHAPE
    # 2^31 - 1 frames of 32 x 64: 1 x 2 tiles each
    big = 2 ** 31 - 1
    mean3 = (_lib.c_float * 3)(0.5, 0.5, 0.5)
    assert lib.ec_stem_conv1(P, P, P, P, big, 32, 64, 32, 0) == EC_ERR_SHAPE
    assert lib.ec_stem_conv1_u8(P, mean3, mean3, P, P, P, big, 32, 64, 32, 0) == EC_ERR_SHAPE
    assert lib.ec_stem_conv1_depth(P, 1.0, 0.0, P, P, P, big, 32, 64, 32, 0) == EC_ERR_SHAPE


def _ratios(case, got, refs):
    return {k: R.worst_ratio(got, *refs[k]) for k in R.shape(case)["kinds"]}


@pytest.mark.parametrize("i", range(len(R.CASES)), ids=lambda i: R.case_id(R.CASES[i]))
def test_bound_bites_on_the_reduced_case(i):
    case = R.reduced(R.CASES[i])
    d = R.shape(case)
    op = R.operands(case)
    refs = R.reference(case, op)
    assert set(refs) == set(d["kinds"])
    emus = {"emulation": R.emulate(case, op)}
    if d["u8"]:
        emus["emulation, unfused affine"] = R.emulate(case, op, unfused=True)
    if d["exact"]:
        ref, bound = refs["tight"]
        assert bound is None and ref.shape == (d["rows"], d["N"]) and torch.equal(emus["emulation"], ref)
        assert not R.wrong_kinds(case)
        return
    for k, (ref, bound) in refs.items():
        assert ref.shape == bound.shape == (d["rows"], d["N"]) and bool((bound >= 0).all()), k
    for name, emu in emus.items():
        for k, (r, at) in _ratios(case, emu, refs).items():
            print(f"{R.case_id(case)}: {name} {k} {r:.3f}")
            assert r <= 1.0, (case["cmd"], name, k, r, at)
    kinds = R.wrong_kinds(case)
    assert kinds
    for kind in kinds:
        w = _ratios(case, R.wrong(case, kind, op), refs)
        print(f"{R.case_id(case)}: {kind} " + " ".join(f"{k} {r:.3g}" for k, (r, _at) in w.items()))
        assert w["tight"][0] >= BITE, (case["cmd"], kind, w)
        if kind in R.TIGHT_ONLY:
            assert w["loose"][0] < BITE, (case["cmd"], kind, w)      # why the loose bound alone would not do
        elif "loose" in w:
            assert w["loose"][0] >= BITE, (case["cmd"], kind, w)

"""Which kernel a conv / GEMM shape runs on is pinned: kernel instance, grid, block and dynamic LDS size of every launch of the
recorded calls and trunk forwards equal tests/golden/conv_routes_golden.json (tests/golden/make_conv_routes_golden.py), under
every dispatch switch -- exactly, there is no tolerance.  Every route computes the same numbers, so the GPU suite cannot see a
rule that stops matching; this can, on a box without a GPU (tools/launch_log.cpp stands in for the HIP runtime)."""
import importlib.util
import json
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_conv_routes_golden",
                                               os.path.join(ROOT, "tests", "golden", "make_conv_routes_golden.py"))
g = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(g)

CXX = os.environ.get("CXX", "c++")
pytestmark = pytest.mark.skipif(shutil.which(CXX) is None, reason="host C++ compiler not found")


@pytest.fixture(scope="module")
def table():
    return json.load(open(g.GOLDEN))


@pytest.fixture(scope="module")
def recorder(tmp_path_factory):
    return g.build_recorder(str(tmp_path_factory.mktemp("launch_log")), CXX)


@pytest.fixture(scope="module")
def lib_path():
    from embodied_clip_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), _lib.LIB_PATH
    return _lib.LIB_PATH


def test_table_matches_the_generator(table):
    assert table["cases"] == g.CASES
    assert {k: v["env"] for k, v in table["settings"].items()} == g.SETTINGS
    assert table["parent_commit"] == g.PARENT_COMMIT


def test_every_rule_decides_a_recorded_case(table):
    """Each rule of the route choice has recorded cases, on both sides of its thresholds (make_conv_routes_golden.EXPECT), and
    the recorded launch of each is the instance that rule stands for."""
    assert {r for _s, r, _c, _k in g.EXPECT} == set(g.RULES) | {"x3"}
    decoded = {s: g.decode(table, s) for s in g.SETTINGS}
    for setting, rule, case, kernel in g.EXPECT:
        rc, launches = decoded[setting][case]
        assert rc == 0 and [l[0] for l in launches] == [kernel], (setting, rule, case, launches)


@pytest.mark.parametrize("setting", list(g.SETTINGS))
def test_launches_equal_the_recorded_table(table, recorder, lib_path, setting):
    _registered, got = g.record(recorder, lib_path, g.SETTINGS[setting])
    want = g.decode(table, setting)
    for case in g.CASES:
        assert got[case] == want[case], (setting, case)


def test_registered_instances_are_recorded_and_none_is_new(table, recorder, lib_path):
    registered, _ = g.record(recorder, lib_path, {})
    mine = {k for k in registered if g.is_conv_igemm(k)}
    parents = set(table["kernels"][:table["registered_conv_igemm"]])
    assert mine <= parents, sorted(mine - parents)
    hit, default_trunk = set(), set()
    for s in g.SETTINGS:
        for case, (_rc, launches) in g.decode(table, s).items():
            hit |= {l[0] for l in launches}
            if s == "default" and case.startswith("trunk"):
                default_trunk |= {l[0] for l in launches}
    assert not (set(g.UNRECORDED) & (hit | default_trunk))
    assert mine - hit <= set(g.UNRECORDED), sorted(mine - hit - set(g.UNRECORDED))

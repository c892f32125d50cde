"""What the act entry points, the `_pa` pair and the two-view net's entry points launch, and what their heads launch is told
(outputs, greedy flag, seed, step, first actor, forcing pointers), is pinned on a box without a GPU: the recorder's output for
every command of tests/golden/make_policy_entry_routes_golden.py equals tests/golden/policy_entry_routes_golden.json byte
for byte.  The table was recorded before the entry points were rebuilt around one call record; a swapped or dropped argument
between an exported function and the heads launch shows here."""
import importlib.util
import json
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_policy_entry_routes_golden",
                                               os.path.join(ROOT, "tests", "golden", "make_policy_entry_routes_golden.py"))
g = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(g)

CXX = os.environ.get("CXX", "c++")
pytestmark = pytest.mark.skipif(shutil.which(CXX) is None, reason="host C++ compiler not found")


@pytest.fixture(scope="module")
def table():
    return json.load(open(g.GOLDEN))


@pytest.fixture(scope="module")
def got(tmp_path_factory):
    from embodied_clip_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), _lib.LIB_PATH
    return g.record(g.build_recorder(str(tmp_path_factory.mktemp("launch_log")), CXX), _lib.LIB_PATH)


def test_table_covers_the_commands(table):
    assert list(table["cases"]) == g.commands() and table["parent_commit"] == g.PARENT_COMMIT
    for cmd, lines in table["cases"].items():
        assert lines[0].startswith("W ") and lines[-1] == "R 0", cmd
    names = " ".join(table["kernels"])
    for k in ("heads_fwd_kernel<8>", "wa_heads_kernel", "il_teacher_force_kernel", "tv_fwd_kernel", "pa_gi_act_kernel"):
        assert k in names, k
    # a selecting heads launch carries its dumped arguments
    dumped = [l for lines in table["cases"].values() for l in lines if l.count("|") == 4]
    assert len(dumped) >= len(table["cases"]) // 2


def test_launches_and_arguments_equal_the_recorded_table(table, got):
    kernels, cases = got
    assert list(cases) == list(table["cases"])
    for cmd, lines in cases.items():
        want = table["cases"][cmd]
        name = lambda l, ks: l if l[0] in "WBFRDS" else ks[int(l.split("|")[0])] + l[l.index("|"):]   # noqa: E731
        assert [name(l, kernels) for l in lines] == [name(l, table["kernels"]) for l in want], cmd

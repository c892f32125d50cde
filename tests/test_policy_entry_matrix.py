"""Which calls the policy entry points accept, and the code of every refusal, is pinned on a box without a GPU: the library
reproduces tests/golden/policy_entry_matrix.json (tests/golden/make_policy_entry_matrix.py) -- every forward, act and backward
entry point against every kind of handle and a list of argument patterns, two-fault rows included, which fix the precedence of
the rules -- and every handle's flat tensor table.  Every row passes ws_bytes = 0: an accepted call ends in EC_ERR_WORKSPACE in
front of its first HIP call."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_policy_entry_matrix", os.path.join(ROOT, "tests", "golden", "make_policy_entry_matrix.py"))
g = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(g)


@pytest.fixture(scope="module")
def table():
    return json.load(open(g.GOLDEN))


@pytest.fixture(scope="module")
def got():
    from embodied_clip_amd import _lib
    return g.record(_lib.load(), _lib)


def test_table_is_sound(table):
    """no row succeeds or launches; the all-valid row of an entry point is EC_ERR_WORKSPACE exactly on the handles it serves"""
    assert table["parent_commit"] == g.PARENT_COMMIT
    assert list(table["codes"]) == list(g.ENTRIES) and all(list(v) == list(g.HANDLES) for v in table["codes"].values())
    g.check(table)
    # the pinned oddities
    first = lambda e: table["codes"][e]["null"][0]     # noqa: E731
    assert (first("ec_policy_act"), first("ec_policy_act_ex")) == (g.UNSUPPORTED, g.ARG)
    assert table["layout"]["null"]["count"] != 0
    # precedence: a bad shape behind a short workspace is still a shape error; an act-only rule beats a forward rule
    names = [n for n, _ in g.patterns("ec_policy_act_ex")]
    row = table["codes"]["ec_policy_act_ex"]["ids"]
    assert row[names.index("N0")] == g.SHAPE and row[names.index("first_actor_m1+no_params")] == g.SHAPE
    assert row[names.index("first_actor_m1+expert_without_mask")] == g.ARG


def test_every_code_equals_the_recorded_table(table, got):
    for entry in g.ENTRIES:
        names = [n for n, _ in g.patterns(entry)]
        for hn in g.HANDLES:
            want, have = table["codes"][entry][hn], got["codes"][entry][hn]
            assert have == want, (entry, hn, [(n, w, h) for n, w, h in zip(names, want, have) if w != h])


def test_every_tensor_table_equals_the_recorded_one(table, got):
    for hn in g.HANDLES:
        assert got["layout"][hn] == table["layout"][hn], hn

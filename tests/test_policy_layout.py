"""The policy handle's buffer layout is pinned: flat parameter offsets and workspace sizes equal the table recorded in
tests/golden/policy_layout_golden.json (tests/golden/make_policy_layout_golden.py) -- byte for byte, not within a tolerance.
The workspace size is the end of the launch plan's layout, so a plan change that moves or resizes an area shows here, on a
box without a GPU (none of these entry points makes a HIP call)."""
import json
import os

import pytest

ACT_MAX_ROWS = 16384


def _table(repo_root):
    return json.load(open(os.path.join(repo_root, "tests", "golden", "policy_layout_golden.json")))


def test_layout_table_covers_the_cases(repo_root):
    t = _table(repo_root)
    assert {"reference", "small", "dual", "fusion"} <= set(t)
    ref = t["reference"]["cfg"]
    assert (ref["in_channels"], ref["spatial"], ref["hidden"]) == (2048, 7, 512)
    assert t["dual"]["cfg"]["dual"] == 1 and t["fusion"]["cfg"]["fusion"] == 1
    for name in ("reference", "small", "dual"):                      # both sides of the act step's row limit, both modes
        rows = {T * N * t[name]["cfg"]["spatial"] ** 2 for T, N, _b, _n in t[name]["workspace_bytes"]}
        assert any(ACT_MAX_ROWS - 64 < r <= ACT_MAX_ROWS for r in rows) and any(ACT_MAX_ROWS < r < ACT_MAX_ROWS + 64 for r in rows), name
        assert min(rows) < ACT_MAX_ROWS // 4, name
        assert {b for _T, _N, b, _n in t[name]["workspace_bytes"]} == {0, 1}


@pytest.mark.parametrize("name", ["reference", "small", "small7", "dual", "dual_small", "fusion", "fusion_small"])
def test_policy_layout_equals_the_recorded_table(repo_root, name):
    import ctypes as C

    from embodied_clip_amd import _lib
    lib = _lib.load()
    want = _table(repo_root)[name]
    h = C.c_void_p()
    _lib.check(lib.ec_policy_create(C.byref(h), C.byref(_lib.PolicyCfg(**want["cfg"]))), "ec_policy_create")
    try:
        assert lib.ec_policy_flat_size(h) == want["flat_size"]
        assert lib.ec_policy_num_param_tensors(h) == len(want["param_offsets"])
        for i, (o, n) in enumerate(want["param_offsets"]):
            off, num = C.c_size_t(), C.c_size_t()
            _lib.check(lib.ec_policy_param_offset(h, i, C.byref(off), C.byref(num)), "ec_policy_param_offset")
            assert (off.value, num.value) == (o, n), (name, i)
        assert len(want["workspace_bytes"]) >= 6
        for T, N, bwd, nbytes in want["workspace_bytes"]:
            assert nbytes > 0
            assert lib.ec_policy_workspace_bytes(h, T, N, bwd) == nbytes, (name, T, N, bwd)
    finally:
        lib.ec_policy_destroy(h)

"""Records the policy handle's buffer layout from a BUILT library (CPU only: none of these entry points makes a HIP call):

    EC_AMD_LIB=/path/to/libec_amd.so python tests/golden/make_policy_layout_golden.py      (from the repository root)

  tests/golden/policy_layout_golden.json    per configuration: ec_policy_flat_size, every ec_policy_param_offset, and
                                            ec_policy_workspace_bytes for a few (T, N) on both sides of the act step's row
                                            limit (ACT_MAX_ROWS = 16384 rows of T * N * spatial^2), for_backward 0 and 1

The committed table was written by the library of the commit BEFORE the host dispatch of csrc/policy.hip was rebuilt around
one launch plan; tests/test_policy_layout.py holds every later build to it."""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from embodied_clip_amd import _lib  # noqa: E402

REFERENCE = dict(in_channels=2048, spatial=7, hidden=512, goal_dims=32, num_goals=12, num_actions=6,
                 compress_hid=128, compress_out=32, comb_hid=128, comb_out=32, fusion=0, dual=0)
# (name, overrides of REFERENCE, [(T, N)]): 334 / 335 actors x 49 pixels and 1820 / 1821 x 9 straddle the 16384-row limit
CASES = [
    ("reference", {}, [(1, 8), (1, 128), (1, 334), (1, 335), (16, 64), (128, 32), (128, 128)]),
    ("small", dict(in_channels=64, spatial=3, hidden=32), [(1, 5), (6, 4), (4, 37), (1, 1820), (1, 1821), (16, 128)]),
    ("small7", dict(in_channels=64, spatial=7, hidden=512), [(1, 37), (16, 64), (1, 334), (1, 335)]),
    ("dual", dict(dual=1), [(1, 8), (1, 334), (1, 335), (128, 32)]),
    ("dual_small", dict(in_channels=64, spatial=3, hidden=32, dual=1), [(1, 5), (4, 37), (1, 1820), (1, 1821)]),
    ("fusion", dict(in_channels=1024, spatial=1, fusion=1), [(1, 8), (1, 128), (128, 128), (1, 20000)]),
    ("fusion_small", dict(in_channels=64, spatial=1, hidden=32, fusion=1), [(1, 5), (6, 4), (1, 20000)]),
]


def record(lib, cfg, shapes):
    h = C.c_void_p()
    _lib.check(lib.ec_policy_create(C.byref(h), C.byref(_lib.PolicyCfg(**cfg))), "ec_policy_create")
    offsets = []
    for i in range(lib.ec_policy_num_param_tensors(h)):
        off, num = C.c_size_t(), C.c_size_t()
        _lib.check(lib.ec_policy_param_offset(h, i, C.byref(off), C.byref(num)), "ec_policy_param_offset")
        offsets.append([off.value, num.value])
    out = {"cfg": cfg, "flat_size": lib.ec_policy_flat_size(h), "param_offsets": offsets,
           "workspace_bytes": [[T, N, b, lib.ec_policy_workspace_bytes(h, T, N, b)] for T, N in shapes for b in (0, 1)]}
    lib.ec_policy_destroy(h)
    return out


if __name__ == "__main__":
    lib = _lib.load()
    table = {name: record(lib, dict(REFERENCE, **over), shapes) for name, over, shapes in CASES}
    path = os.path.join(HERE, "policy_layout_golden.json")
    json.dump(table, open(path, "w"), indent=0, separators=(",", ":"))
    print("wrote", path, os.path.getsize(path), "bytes from", _lib.LIB_PATH)

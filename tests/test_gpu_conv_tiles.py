"""GPU: every registered instance of conv_igemm_kernel / conv_igemm8_kernel that the public entry points reach (51 of 55; the other
four: _conv_tile_ref.EXEMPT) against the float64 references and element-wise bounds of tests/_conv_tile_ref.py -- no margin on top of
the derived bounds (the CPU suite checks that those bounds bite and that each case launches the instance it names:
tests/test_conv_tile_ref.py).  One child process per switch setting (tests/_conv_tile_check.py), one at a time; a child that ends by
signal or at its time limit stops every later child of the whole run before it starts a process (tests/_child.py).

Measured worst |error| / bound per instance on an MI355X (every case under 1: the pass threshold is 1.0, not these figures).
c8<BN, KS, POOL, long segments, X3, S2> = conv_igemm8_kernel, c4<BM, BN, WM, WN, KS, POOL, PF, MV, NS, ILV, S2> = conv_igemm_kernel:
  c8<256, 3, -, -, -, -> 0.919   c8<256, 3, pool> 0.885        c8<256, 1> 0.893              c8<256, 1, pool> 0.907
  c8<128, 3, long> 0.916         c8<128, 3, pool, long> 0.906  c8<128, 1, long> 0.926        c8<128, 1, pool, long> 0.879
  c8<128, 3> 0.922               c8<128, 3, pool> 0.854        c8<128, 1> 0.902              c8<128, 1, pool> 0.909
  c8<256, 3, S2> 0.917           c8<256, 1, S2> 0.922          c8<128, 3, long, S2> 0.922    c8<128, 1, long, S2> 0.917
  c8<128, 3, S2> 0.924           c8<128, 1, S2> 0.913          c8<128, 1, long, X3> 0.003    c8<128, 1, X3> 0.003  (fp32 output: the
                                                                                              accumulation term is the whole bound)
  c4<224, 128, 1, 4, 3> 0.815    c4<224, 128, 1, 4, 1> 0.907
  c4<64, 64, 3, ring> 0.861      c4<64, 64, 1, ring> 0.865     c4<64, 64, 3> 0.856           c4<64, 64, 1> 0.894
  c4<64, 64, 3, ring, S2> 0.899  c4<64, 64, 1, ring, S2> 0.907
  c4<128, 128, 2, 2, 3> 0.921    ... pool 0.914                c4<128, 128, 2, 2, 1> 0.904   ... pool 0.944    ... prefetch 0.936
  c4<128, 128, 2, 2, 3, S2> 0.915                              c4<128, 128, 2, 2, 1, S2> 0.942
  c4<128, 128, 2, 4, 3, ring> 0.915   ... pool 0.863           c4<128, 128, 2, 4, 1, ring> 0.913   ... pool 0.898
  c4<128, 128, 2, 4, 3, ring, S2> 0.913                        c4<128, 128, 2, 4, 1, ring, S2> 0.911
  c4<256, 64, 3> 0.858  pool 0.770  S2 0.888                   c4<256, 64, 1> 0.930  pool 0.938  S2 0.946
  c4<256, 32, 3> 0.858  pool 0.831                             c4<256, 32, 1> 0.916  pool 0.931
The one bf16 rounding of the result is nearly the whole budget (2^-8 |ref| against a worst observed 0.95 of the bound); every guard
element intact.  The file takes 10 s in all (setting a 5.2 s, setting b 3.2 s; launch to synchronize 7 ms: the rest is the float64
references and the start of the two child processes)."""
import json
import os
import sys

import pytest

import _conv_tile_ref as R
from _child import GPU, last_json

pytestmark = pytest.mark.gpu

CHILD_LIMIT = 300


@pytest.mark.parametrize("setting", list(R.SETTINGS))
def test_conv_tiles_in_a_child_process(setting):
    """Every case of the setting once: worst |error| / bound <= 1 and every guard element (a tile of rows before and after the
    output, the columns around a column-block output) bitwise untouched."""
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_conv_tile_check.py")
    p = GPU.run([sys.executable, script, setting], drop=R.SWITCHES, env=R.SETTINGS[setting], limit=CHILD_LIMIT)
    print("\n".join(p.stdout.splitlines()[:-1])[-20000:])
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    res = last_json(p)
    cases = R.cases_of(setting)
    assert res["setting"] == setting and [c["cmd"] for c in res["cases"]] == [c["cmd"] for c in cases]
    worst = {}
    for c, want in zip(res["cases"], cases):
        assert c["instance"] == want["instance"]
        worst[c["instance"]] = max(worst.get(c["instance"], 0.0), c["ratio"])
    print("worst per instance", setting, json.dumps(worst, indent=0))
    print("GPU seconds (launch to synchronize)", setting, sum(c["gpu_s"] for c in res["cases"]))
    for c in res["cases"]:
        assert c["guards_ok"], c
        assert c["ratio"] <= 1.0, c

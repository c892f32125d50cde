"""GPU: every registered instance of the nine fused-kernel templates of conv3x3_narrow.hip, conv_pair.hip, conv_bneck.hip and
conv_basic.hip that a public entry point reaches (32 of 33; the other one: _trunk_fused_ref.EXEMPT) against the float64 references
and element-wise bounds of tests/_trunk_fused_ref.py -- no margin on top of the derived bounds (the CPU suite checks that those
bounds bite and that each case launches the instance it names: tests/test_trunk_fused_ref.py).  One child process per switch
setting (tests/_trunk_fused_check.py), one at a time, each with its own time limit; a child that ends by signal, abort code or at
its time limit stops every later child of the whole run before it starts a process (tests/_child.py).

Measured worst |error| / bound per instance on an MI355X (every output of every case under 1: the pass threshold is 1.0, not these
figures; two-stage kernels: the worst of their outputs):
  conv3x3_rowsN_kernel   <64, 64, 2, 4, 2> 0.891    <64, 64, 2, 4, 3> 0.870    <32, 32, 4, 8, 1> 0.939    <32, 32, 4, 4, 2> 0.931
  conv3x3_rows_kernel    <32, 32, false, 16> 0.929  <32, 64, false, 16> 0.914  <32, 64, true, 16> 0.905
                         <64, 64, false, 6> 0.912   <64, 64, true, 8> 0.837
  conv3x3_narrow_kernel  <32, 32, false, 16> 0.933  <32, 64, false, 16> 0.925  <32, 64, true, 16> 0.899
                         <64, 64, false, 16> 0.903  <64, 64, true, 16> 0.836
  conv1x1_pair_kernel <TWO, RES, N2, PL>  <true, true, 64> 0.944 (y 0.944, z 0.938)  <true, false, 64> 0.942  <false, true, 64> 0.946
                         <false, false, 64> 0.941   <false, true, 128> 0.940   <false, false, 128> 0.942
                         <false, true, 128, pooled> 0.949 (y 0.944, pooled y 0.949, z 0.933; y = NULL: z and pooled y bit-identical)
  conv1x1_pair512_kernel 0.944 (y 0.944, z 0.921)
  conv1x1_regw_kernel    <256, 512> 0.938           <512, 256, relu> 0.914     <128, 512, res, relu> 0.944
  conv3x3_img_kernel     <256, 14, 1> 0.924         <512, 7, 2> 0.870          <512, 14, 1, 2, pooled> 0.881 (column block 0.799)
  bneck23_kernel         conv2 + conv3 0.920        conv1 + conv2 + conv3 0.905   (6.0 % / 6.1 % of the intermediate elements at risk:
                                                                                   the cap is 12.5 %)
  basic_tail_s2_kernel   <128, 128> 0.898           <64, 64> 0.916
The one bf16 rounding of each stored tensor is nearly the whole budget, as for the conv_igemm tiles; every guard element intact; no
kernel exceeded its bound.  The file takes 20 s in all (the default setting's 40 cases 7.8 s, each of the four other settings
under 3.1 s; launch to synchronize 0.13 s in all: the rest is the float64 references, the copies and the start of the five child
processes).
"""
import json
import os
import sys

import pytest

import _trunk_fused_ref as R
from _child import GPU, last_json

pytestmark = pytest.mark.gpu

CHILD_LIMIT = 300


@pytest.mark.parametrize("setting", list(R.SETTINGS))
def test_trunk_fused_kernels_in_a_child_process(setting):
    """Every case of the setting once: worst |error| / bound <= 1 on every output, every guard element (a tile of rows before and
    after each output, the columns around a column-block output) bitwise untouched, the share of bneck intermediates at risk under
    its cap, and the pooled pair kernel's outputs with y = NULL bit for bit those with y stored."""
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_trunk_fused_check.py")
    p = GPU.run([sys.executable, script, setting], drop=R.SWITCHES, env=R.SETTINGS[setting], limit=CHILD_LIMIT)
    print("\n".join(p.stdout.splitlines()[:-1])[-20000:])
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    res = last_json(p)
    cases = R.cases_of(setting)
    assert res["setting"] == setting and [c["cmd"] for c in res["cases"]] == [c["cmd"] for c in cases]
    worst = {}
    for c, want in zip(res["cases"], cases):
        assert c["instance"] == want["instance"] and set(c["outputs"]) == set(R.outputs(want))
        worst[c["instance"]] = max(worst.get(c["instance"], 0.0), c["ratio"])
    print("worst per instance", setting, json.dumps(worst, indent=0))
    print("GPU seconds (launch to synchronize)", setting, sum(c["gpu_s"] for c in res["cases"]))
    for c in res["cases"]:
        assert c["guards_ok"], c
        assert c["ratio"] <= 1.0, c
        assert c.get("risk", 0.0) <= R.RISK_CAP, c
        assert c.get("identical", True), c

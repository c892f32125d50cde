"""GPU: every registered instance of the front-end kernels that a public entry point reaches (15 of 18; the other three:
_front_end_ref.EXEMPT) -- the RGB, depth and 7 x 7 stems, the 2 x 2 average pool, the two layout kernels, the spatial mean --
against the float64 references and element-wise bounds of tests/_front_end_ref.py, no margin on top of the derived bounds (the CPU
suite checks that those bounds bite and that each case launches the instance it names: tests/test_front_end_ref.py).  The MFMA
stems are held to two references each: the tight one, of the operands rounded as the kernel rounds them, and the loose one, of the
unrounded frame and fp32 weights.  One child process (tests/_front_end_check.py) with its own time limit: a child that ends by signal, abort
code or at its limit fails the test and stops every later child of the whole run before it starts a process (tests/_child.py).

Measured worst |error| / bound per instance on an MI355X (every case under 1: the pass threshold is 1.0, not these figures):
  stem_conv1_kernel        <32, false> tight 0.941 loose 0.392   <32, true> 0.942 / 0.436   <64, false> 0.947 / 0.422
                           <64, true> 0.944 / 0.416              <48, false> 0.942          <48, true> 0.947  (fp32 route: one reference)
  stem_conv1_depth_kernel  <32> tight 0.946 loose 0.575          <64> 0.948 / 0.653         <48> 0.947
  stem7_pool_kernel        <false> tight 0.943 loose 0.380       <true> 0.943 / 0.428  (520 tiles on 512 workgroups: 0.943 both)
  avgpool2_kernel          0.949 (dense 0.941, column block 0.948, grid-stride case 0.949)
  spatial_mean_kernel      0.019 (fp32 output: the accumulation term is the whole bound)
  nhwc_to_nchw_kernel, nchw_to_nhwc_bf16_kernel   bit-exact, the flag as stated in every variant
Every figure equals the CPU emulation's to the three digits shown: the one bf16 rounding of the stored tensor is nearly the whole
tight budget, the operand roundings about 0.4 of the loose one.  Every guard element intact; no kernel exceeded a bound.  The
file takes 5.3 s in all (the child's 44 cases 3.1 s, 0.6 s of it the 68 MB average-pool case; launch to synchronize 4 ms in all:
the rest is the float64 references, the copies and the start of the child process).
"""
import json
import os
import sys

import pytest

import _front_end_ref as R
from _child import GPU, last_json

pytestmark = pytest.mark.gpu

CHILD_LIMIT = 300


def test_front_end_kernels_in_a_child_process():
    """Every case once: the instance it names, worst |error| / bound <= 1 against the tight and (MFMA stems) the loose reference,
    every guard element (a tile of rows before and after the output, the columns around the column-block output, the words around
    the flag) bitwise untouched, the layout kernels and the flag exact."""
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_front_end_check.py")
    p = GPU.run([sys.executable, script], limit=CHILD_LIMIT)
    print("\n".join(p.stdout.splitlines()[:-1])[-20000:])
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    res = last_json(p)
    assert [(c["cmd"], c["variant"]) for c in res["cases"]] == [(c["cmd"], c["variant"]) for c in R.CASES]
    worst = {}
    for c, want in zip(res["cases"], R.CASES):
        d = R.shape(want)
        assert c["instance"] == want["instance"] and c["branch"] == R.staging_branch(want)
        assert set(c["outputs"]) == {"out"} and set(c["outputs"]["out"]) == set(d["kinds"])
        for kind, r in c["outputs"]["out"].items():
            key = c["instance"] + " " + kind
            worst[key] = max(worst.get(key, 0.0), r)
    print("worst per instance", json.dumps(worst, indent=0))
    print("GPU seconds (launch to synchronize)", sum(c["gpu_s"] for c in res["cases"]))
    for c, want in zip(res["cases"], R.CASES):
        assert c["guards_ok"], c
        assert all(r <= 1.0 for r in c["outputs"]["out"].values()), c
        if R.shape(want)["exact"]:
            assert c["exact"] is True, c
        if "flags" in c or R.shape(want)["kind"] == "tonhwc":
            assert set(c["flags"]) == set(R.FLAG_VARIANTS) and all(got == exp for got, exp in c["flags"].values()), c

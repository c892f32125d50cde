"""Run as a subprocess by tests/test_gpu_conv_tiles.py (the library reads its dispatch switches once per process): every case of
_conv_tile_ref.cases_of(setting) once, through the public entry point its command names, into an output that has one guard tile
of sentinel rows before and after it (and sentinel columns around a column-block output), against _conv_tile_ref.reference.
Prints one line per case (instance, worst |error| / bound, the index of that element) and, last, the results as JSON."""
import json
import os
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from _guard import Guarded  # noqa: E402

COL0 = 24                  # first column of a column-block output (16-byte aligned)


def run_case(R, _lib, lib, dev, case):
    d = R.shape(case)
    op = R.operands(case)
    st = _lib.stream_ptr()
    x, w, bias = op["x"].to(dev), op["w"].to(dev), op["bias"].to(dev)
    res = op["res"].to(dev) if op["res"] is not None else None
    rp = res.data_ptr() if res is not None else None
    rows, N, ldo = d["rows"], d["Cout"], d["ldo"]
    o = Guarded(dev, rows, N, ldo, COL0 if ldo > N else 0, f32=d["x3"])
    out_ptr = o.ptr
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if d["kind"] == "conv":
        rc = lib.ec_conv_bf16_ld(x.data_ptr(), w.data_ptr(), bias.data_ptr(), rp, out_ptr, d["B"], d["H"], d["W"], d["Cin"], N, d["ks"],
                                 d["pool"], d["act"], ldo, st)
    elif d["kind"] == "s2":
        rc = lib.ec_conv_bf16_s2(x.data_ptr(), w.data_ptr(), bias.data_ptr(), rp, out_ptr, d["B"], d["H"], d["W"], d["Cin"], N, d["ks"],
                                 d["act"], st)
    elif d["kind"] == "gemm":
        rc = lib.ec_gemm_bf16(x.data_ptr(), w.data_ptr(), bias.data_ptr(), rp, out_ptr, d["M"], N, d["K"], d["act"], st)
    else:
        rc = lib.ec_gemm_bf16a_x3(x.data_ptr(), w.data_ptr(), bias.data_ptr(), out_ptr, d["M"], N, d["K"], d["act"], st)
    _lib.check(rc, case["cmd"])
    torch.cuda.synchronize()
    gpu_s = time.perf_counter() - t0
    body, guards_ok = o.read()
    got = body.view(torch.float32) if d["x3"] else body.view(torch.bfloat16)
    ref, bound = R.reference(case, op)
    ratio, at = R.worst_ratio(got, ref, bound)
    return dict(cmd=case["cmd"], instance=case["instance"], ratio=ratio, at=[at // N, at % N], guards_ok=guards_ok, gpu_s=gpu_s)


def main():
    import _conv_tile_ref as R
    from embodied_clip_amd import _lib
    setting = sys.argv[1]
    want = R.SETTINGS[setting]
    assert all(os.environ.get(k) == want.get(k) for k in R.SWITCHES), "switches of the setting not in force"
    lib = _lib.load()
    dev = torch.device("cuda:0")
    results = []
    for case in R.cases_of(setting):
        r = run_case(R, _lib, lib, dev, case)
        print(f"{r['instance']}  ratio {r['ratio']:.3f} at row {r['at'][0]} col {r['at'][1]}  guards {'ok' if r['guards_ok'] else 'WRITTEN'}"
              f"  [{r['cmd']}]", flush=True)
        results.append(r)
    print(json.dumps({"setting": setting, "cases": results}))


if __name__ == "__main__":
    main()

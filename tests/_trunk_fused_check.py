"""Run as a subprocess by tests/test_gpu_trunk_fused.py (the library reads its dispatch switches once per process): every case of
_trunk_fused_ref.cases_of(setting) once, through the public entry point its command names, every output between one guard tile of
sentinel rows before and after it (and sentinel columns around a column-block output), against _trunk_fused_ref.reference.  The
pooled pair case with y = NULL runs twice -- y stored, then not -- and its z and pooled y must be equal bit for bit.
Prints one line per case (instance, worst |error| / bound per output, the index of that element) and, last, the results as JSON."""
import json
import os
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from _guard import SENT16, Guarded  # noqa: E402

COL0 = 24                  # first column of a column-block output (16-byte aligned)


def run_case(R, _lib, lib, dev, case):
    d = R.shape(case)
    op = R.operands(case)
    st = _lib.stream_ptr()
    g = {k: (v.to(dev) if v is not None else None) for k, v in op.items()}
    p = {k: (v.data_ptr() if v is not None else None) for k, v in g.items()}
    k, M, N = d["kind"], d["M"], d["N"]
    outs, identical = {}, None
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if k in ("conv", "regw"):
        outs["out"] = o = Guarded(dev, d["rows"], N)
        rc = lib.ec_conv_bf16_ld(p["x"], p["w"], p["bias"], p.get("res"), o.ptr, d["B"], d["H"], d["W"], d["Cin"], N, d["ks"], d["pool"],
                                 d["act"], N, st)
    elif k == "pair":
        outs["y"], outs["z"] = y, z = Guarded(dev, M, N), Guarded(dev, M, d["N2"])
        rc = lib.ec_conv1x1_pair_bf16(p["a0"], p["w0"], p["b0"], p["a1"], p["w1"], p["b1"], p["res"], y.ptr, p["w2"], p["b2"], z.ptr, M, d["K"],
                                      N, d["N2"], st)
    elif k == "pairpool":
        def once(with_y):
            y, yp, z = Guarded(dev, M, N), Guarded(dev, M // 4, N), Guarded(dev, M, d["N2"])
            r = lib.ec_conv1x1_pair_pool_bf16(p["a0"], p["w0"], p["b0"], p["res"], y.ptr if with_y else None, yp.ptr, p["w2"], p["b2"], z.ptr,
                                              d["B"], d["H"], d["W"], d["K"], N, d["N2"], st)
            return r, dict(y=y, yp=yp, z=z)
        rc, outs = once(True)
        if not d["ystored"] and rc == 0:
            rc, second = once(False)
            torch.cuda.synchronize()
            identical = all(torch.equal(second[o].buf, outs[o].buf) for o in ("yp", "z"))
            untouched = bool((second["y"].buf == SENT16).all())
            outs = dict(y=outs["y"], yp=second["yp"], z=second["z"])     # y of the first run; the outputs under test of the second
            identical = identical and untouched
    elif k == "img":
        packed = torch.empty_like(g["w"])
        rc = lib.ec_conv3x3_img_pack(p["w"], packed.data_ptr(), d["Cin"], st)
        outs["out"] = o = Guarded(dev, d["rows"], N, d["ldo"], COL0 if d["ldo"] > N else 0)
        if rc == 0:
            rc = lib.ec_conv3x3_img_bf16_ld(p["x"], packed.data_ptr(), p["bias"], o.ptr, d["B"], d["H"], d["W"], d["Cin"], d["pool"], d["ldo"], st)
    elif k in ("bneck23", "bneck123"):
        C = d["C"]
        f1 = k == "bneck123"
        packed = torch.empty(int(lib.ec_bneck3_packed_elems(C) if f1 else lib.ec_bneck_packed_elems(C)), dtype=torch.bfloat16, device=dev)
        outs["out"] = o = Guarded(dev, M, N)
        if f1:
            rc = lib.ec_bneck3_pack_weights(p["w1"], p["w2"], p["w3"], packed.data_ptr(), C, st)
            if rc == 0:
                rc = lib.ec_bneck_conv123_bf16(p["x"], packed.data_ptr(), p["b1"], p["b2"], p["b3"], o.ptr, d["B"], d["H"], d["W"], C, st)
        else:
            rc = lib.ec_bneck_pack_weights(p["w2"], p["w3"], packed.data_ptr(), C, st)
            if rc == 0:
                rc = lib.ec_bneck_conv23_bf16(p["c1"], packed.data_ptr(), p["b2"], p["b3"], p["x"], o.ptr, d["B"], d["H"], d["W"], C, st)
    elif k == "tail":
        outs["out"] = o = Guarded(dev, M, N)
        rc = lib.ec_basic_tail_s2_bf16(p["c1"], p["x"], p["w"], p["bias"], o.ptr, d["B"], d["H"], d["W"], d["P"], d["I"], N, st)
    else:
        raise KeyError(k)
    _lib.check(rc, case["cmd"])
    torch.cuda.synchronize()
    gpu_s = time.perf_counter() - t0
    got, guards_ok = {}, True
    for name, o in outs.items():
        body, ok = o.read()
        got[name] = body.view(torch.bfloat16)
        guards_ok = guards_ok and ok
    worst, risk = R.worst_of(case, got, op)
    res = dict(cmd=case["cmd"], instance=case["instance"], ratio=max(r for r, _ in worst.values()), guards_ok=guards_ok, gpu_s=gpu_s,
               outputs={o: dict(ratio=r, at=[at // got[o].shape[1], at % got[o].shape[1]]) for o, (r, at) in worst.items()})
    if risk is not None:
        res["risk"] = risk
    if identical is not None:
        res["identical"] = identical
    return res


def main():
    import _trunk_fused_ref as R
    from embodied_clip_amd import _lib
    setting = sys.argv[1]
    want = R.SETTINGS[setting]
    assert all(os.environ.get(k) == want.get(k) for k in R.SWITCHES), "switches of the setting not in force"
    lib = _lib.load()
    dev = torch.device("cuda:0")
    results = []
    for case in R.cases_of(setting):
        t0 = time.perf_counter()
        r = run_case(R, _lib, lib, dev, case)
        r["wall_s"] = time.perf_counter() - t0
        outs = "  ".join(f"{o} {v['ratio']:.3f} at row {v['at'][0]} col {v['at'][1]}" for o, v in r["outputs"].items())
        extra = ("  at risk %.4f" % r["risk"] if "risk" in r else "") + ("  y = NULL %s" % ("identical" if r["identical"] else "DIFFERS")
                                                                         if "identical" in r else "")
        print(f"{r['instance']}  {outs}{extra}  guards {'ok' if r['guards_ok'] else 'WRITTEN'}  [{r['cmd']}] {r['wall_s']:.1f} s", flush=True)
        results.append(r)
    print(json.dumps({"setting": setting, "cases": results}))


if __name__ == "__main__":
    main()

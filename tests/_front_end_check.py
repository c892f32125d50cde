"""Run as a subprocess by tests/test_gpu_front_end.py: every case of _front_end_ref.CASES once, through the public entry point its
command names, into an output that has one guard tile of sentinel rows before and after it (and sentinel columns around the
column-block output), against _front_end_ref.reference -- the tight and, for the MFMA stems, the loose one.  The layout kernels
are compared bit for bit; nchw_to_nhwc_bf16 runs once per flag variant (_front_end_ref.FLAG_VARIANTS), its flag word between two
sentinel words.  Prints one line per case and, last, the results as JSON."""
import ctypes
import json
import os
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from _guard import SENT32, Guarded  # noqa: E402


def _f3(values):
    return (ctypes.c_float * 3)(*values)


def run_case(R, _lib, lib, dev, case):
    d = R.shape(case)
    op = R.operands(case)
    st = _lib.stream_ptr()
    k = d["kind"]
    res = dict(cmd=case["cmd"], variant=case["variant"], instance=case["instance"], branch=R.staging_branch(case))
    if k == "tonhwc":
        return dict(res, **run_tonhwc(R, _lib, lib, dev, case, d, op, st))
    x = op["x"].to(dev)
    xp = x.data_ptr()
    if d["off"]:                                           # the frame starts one float into its allocation
        hold = torch.zeros(x.numel() + 8, dtype=torch.float32, device=dev)
        hold[d["off"]:d["off"] + x.numel()] = x.reshape(-1)
        xp = hold.data_ptr() + 4 * d["off"]
    if k in ("stem", "dstem", "stem7"):
        assert (xp % 16 == 0) == (d["off"] == 0), "frame pointer alignment is not what staging_branch assumed"
        w = (R.pack_stem7(op["w"]) if k == "stem7" else op["w"]).to(dev)
        bias = op["bias"].to(dev)
        mean3, std3 = (_f3(t) for t in R.CONSTS[case["consts"]]) if d["u8"] else (None, None)
    o = Guarded(dev, d["rows"], d["N"], d["ldo"], R.COL0 if d["ldo"] > d["N"] else 0, f32=d["out_dtype"] == "f32")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if k == "stem" and d["u8"]:
        rc = lib.ec_stem_conv1_u8(xp, mean3, std3, w.data_ptr(), bias.data_ptr(), o.ptr, d["B"], d["H"], d["W"], d["Cout"], st)
    elif k == "stem":
        rc = lib.ec_stem_conv1(xp, w.data_ptr(), bias.data_ptr(), o.ptr, d["B"], d["H"], d["W"], d["Cout"], st)
    elif k == "stem7":
        rc = lib.ec_stem7_pool(xp, d["u8"], mean3, std3, w.data_ptr(), bias.data_ptr(), o.ptr, d["B"], d["H"], d["W"], st)
    elif k == "dstem":
        rc = lib.ec_stem_conv1_depth(xp, case["affine"][0], case["affine"][1], w.data_ptr(), bias.data_ptr(), o.ptr, d["B"], d["H"], d["W"],
                                     d["Cout"], st)
    elif k == "avgpool" and d["ldo"] == d["N"]:
        rc = lib.ec_avgpool2_bf16(xp, o.ptr, d["B"], d["H"], d["W"], d["Cout"], st)
    elif k == "avgpool":
        rc = lib.ec_avgpool2_bf16_ld(xp, o.ptr, d["B"], d["H"], d["W"], d["Cout"], d["ldo"], st)
    elif k == "tonchw":
        rc = lib.ec_nhwc_bf16_to_nchw_f32(xp, o.ptr, d["B"], d["HW"], d["C"], st)
    elif k == "mean":
        rc = lib.ec_spatial_mean_bf16(xp, o.ptr, d["B"], d["HW"], d["C"], st)
    else:
        raise KeyError(k)
    _lib.check(rc, case["cmd"])
    torch.cuda.synchronize()
    res["gpu_s"] = time.perf_counter() - t0
    body, res["guards_ok"] = o.read()
    got = body.view(torch.float32) if o.f32 else body.view(torch.bfloat16)
    refs = R.reference(case, op)
    out = {}
    for kind, (ref, bound) in refs.items():
        if bound is None:
            res["exact"] = bool(torch.equal(got.view(torch.int32), ref.view(torch.int32)))
            out[kind] = 0.0 if res["exact"] else float("inf")
        else:
            out[kind], at = R.worst_ratio(got, ref, bound)
            res["at_" + kind] = [at // d["N"], at % d["N"]]
    res["outputs"] = {"out": out}
    return res


def run_tonhwc(R, _lib, lib, dev, case, d, op, st):
    """One run per flag variant: the output bit for bit ec_f2bf of the permuted input, the flag word as the variant says."""
    out = dict(guards_ok=True, exact=True, flags={}, gpu_s=0.0)
    for name, (preset, planted, want) in R.FLAG_VARIANTS.items():
        x = op["x"].clone()
        if planted is not None:
            x[-1, -1, -1] = planted
        xd = x.to(dev)
        o = Guarded(dev, d["rows"], d["N"])
        flag = torch.tensor([SENT32, preset, SENT32], dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = lib.ec_nchw_f32_to_nhwc_bf16(xd.data_ptr(), o.ptr, d["B"], d["HW"], d["C"], flag.data_ptr() + 4, st)
        _lib.check(rc, case["cmd"])
        torch.cuda.synchronize()
        out["gpu_s"] += time.perf_counter() - t0
        body, ok = o.read()
        f = flag.cpu().tolist()
        out["guards_ok"] = out["guards_ok"] and ok and f[0] == SENT32 and f[2] == SENT32
        out["exact"] = out["exact"] and bool(torch.equal(body, R.f2bf_bits(x.permute(0, 2, 1).contiguous()).reshape(d["rows"], d["N"])))
        out["flags"][name] = [f[1], want]
    out["outputs"] = {"out": {"tight": 0.0 if out["exact"] else float("inf")}}
    return out


def main():
    import _front_end_ref as R
    from embodied_clip_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    results = []
    for case in R.CASES:
        t0 = time.perf_counter()
        r = run_case(R, _lib, lib, dev, case)
        r["wall_s"] = time.perf_counter() - t0
        ratios = " ".join(f"{k} {v:.3f}" for k, v in r["outputs"]["out"].items())
        extra = (" exact" if r.get("exact") else " DIFFERS") if "exact" in r else ""
        extra += " flags %s" % r["flags"] if "flags" in r else ""
        print(f"{r['instance']}  {ratios}{extra}  guards {'ok' if r['guards_ok'] else 'WRITTEN'}  [{R.case_id(case)}"
              f"{' ' + r['branch'] if r['branch'] else ''}] {r['wall_s']:.2f} s", flush=True)
        results.append(r)
    print(json.dumps({"cases": results}))


if __name__ == "__main__":
    main()

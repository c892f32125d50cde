"""Run as a subprocess by tests/test_gpu_policy_gemm.py (the library reads its dispatch switches once per process): every case of
_policy_gemm_ref.cases_of(setting) once through ec_gemm_f32, its operands embedded in larger tensors (offset bases, padded pitches,
generic strides: NaN everywhere else), its output in a buffer with one guard tile of sentinel rows before and after it and sentinel
columns from N up to ldc (parts: the whole splitk x M x ldc buffer), prefilled with NaN where the kernel must write every element and
with C0 under ACCUMULATE, against _policy_gemm_ref.reference.  Prints one line per case and, last, the results as JSON."""
import json
import os
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from _guard import Guarded  # noqa: E402


def run_case(R, _lib, lib, dev, case, done):
    d = R.shape(case)
    op = R.operands(case)
    st = _lib.stream_ptr()
    M, N, K, ldc = d["M"], d["N"], d["K"], d["ldc"]
    abuf, _ao, bbuf, _bo = R.embedded(case, op)
    A, B = abuf.to(dev), bbuf.to(dev)
    nparts = d["nslices"] if d["parts"] else 1
    assert not d["parts"] or d["splitk"] == d["nslices"]
    dm = None
    if op["dmask"] is not None:             # indexed like C: pitch ldc (NaN in the columns from N on)
        dm = torch.full((M, ldc), float("nan"))
        dm[:, :N] = op["dmask"]
        dm = dm.to(dev)
    dv = {k: (op[k].to(dev) if op[k] is not None else None) for k in ("bias", "gbias", "gidx", "rowscale")}
    p = lambda t: None if t is None else t.data_ptr()

    def launch():
        o = Guarded(dev, nparts * M, N, ldc, f32=True, fill=op["c0"] if d["acc"] else float("nan"))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = lib.ec_gemm_f32(A.data_ptr() + d["aoff"], B.data_ptr() + d["boff"], o.ptr, M, N, K, d["sam"], d["sak"], d["sbk"], d["sbn"], ldc,
                             d["flags"], p(dv["bias"]), p(dv["gbias"]), p(dv["gidx"]), d["group"], p(dm), p(dv["rowscale"]), d["splitk"], st)
        _lib.check(rc, case["cmd"])
        torch.cuda.synchronize()
        return o, time.perf_counter() - t0

    o, gpu_s = launch()
    res = dict(cmd=case["cmd"], instance=case["instance"], gpu_s=gpu_s)
    if d["parts"]:
        res["twice_same"] = bool(torch.equal(launch()[0].buf.cpu(), o.buf.cpu()))
    body, res["guards_ok"] = o.read()
    got = body.view(torch.float32)
    got = got.view(nparts, M, N) if d["parts"] else got
    res["nan_free"] = not bool(torch.isnan(got).any())
    ref, bound = R.reference(case, op)
    res["ratio"], at = R.worst_ratio(got, ref, bound)
    res["at"] = [at // N, at % N]
    if R.needs_l2(case):
        thr, e6, e3 = R.l2_threshold(case, op, ref)
        res.update(l2=R.rel_l2(got, ref), l2_threshold=thr, l2_six=e6, l2_three=e3)
    if d["p3"]:
        res["twin_equal"] = bool(torch.equal(done[R.twin_cmd(case)], got))
    done[case["cmd"]] = got
    return res


def main():
    import _policy_gemm_ref as R
    from embodied_clip_amd import _lib
    setting = sys.argv[1]
    want = R.SETTINGS[setting]
    assert all(os.environ.get(k) == want.get(k) for k in R.SWITCHES), "switches of the setting not in force"
    lib = _lib.load()
    dev = torch.device("cuda:0")
    results, done = [], {}
    for case in R.cases_of(setting):
        r = run_case(R, _lib, lib, dev, case, done)
        extra = ""
        if "l2" in r:
            extra += f"  L2 {r['l2']:.2e} < {r['l2_threshold']:.2e} (six {r['l2_six']:.2e}, three {r['l2_three']:.2e})"
        if "twin_equal" in r:
            extra += f"  twin {'equal' if r['twin_equal'] else 'differs'}"
        if "twice_same" in r:
            extra += f"  twice {'same' if r['twice_same'] else 'DIFFERENT'}"
        print(f"{r['instance']}  ratio {r['ratio']:.3f} at {r['at']}  guards {'ok' if r['guards_ok'] else 'WRITTEN'}"
              f"  {'' if r['nan_free'] else 'NaN LEFT  '}{extra.strip()}  [{r['cmd']}]", flush=True)
        results.append(r)
    print(json.dumps({"setting": setting, "cases": results}))


if __name__ == "__main__":
    main()

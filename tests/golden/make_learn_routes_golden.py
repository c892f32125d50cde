"""Records what a BUILT library launches for the learn pass of every case of tests/_learn_route_cases.py, each under its switch
setting (CPU only: tools/launch_log.cpp stands in for the HIP runtime; mode 2 of its `policy` command runs the EC_POLICY_LEARN
forward and then ec_policy_backward2 in the same workspace):

    EC_AMD_LIB=/path/to/libec_amd.so python tests/golden/make_learn_routes_golden.py      (from the repository root)

  tests/golden/learn_routes_golden.json    `kernels`: the kernel names once; `policy_kernels`: every instance the library
                                           registers of a kernel that csrc/policy.hip defines; per case the command, the
                                           workspace size, the return code and the events of the forward (`fwd`) and of the
                                           backward (`bwd`): a launch is [kernel index, grid x, y, z, block x, dynamic LDS
                                           bytes], a device-to-device copy is ["D", bytes]

The committed table is what the library of commit b12b1a8 launches, the commit before tests/test_learn_routes.py existed, but
for ONE launch: in h48_t3_n5 and exact_h48_t3_n5 (H = 48, 3H = 144 no multiple of 32) the transpose of the re-ordered weight_ih
in front of dx4 = dgi @ W_ih has a grid 5 row blocks deep where that library launched 4 (144 / 32 rounded down: the last 16
rows of the weight never reached the GEMM, and every gradient in front of the GRU was wrong -- found by
tests/test_gpu_learn_routes.py, fixed in the commit that added it).  No route changed, and no other entry differs.
tests/test_learn_routes.py holds every later build to the table, launch for launch, so a change of a learn-pass route has to
re-record it on purpose.
The library reads its switches once per process: one recorder process per setting."""
import importlib.util
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
GOLDEN = os.path.join(HERE, "learn_routes_golden.json")
PARENT_COMMIT = "b12b1a8"


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


act = _load("make_policy_routes_golden", os.path.join(HERE, "make_policy_routes_golden.py"))
cases = _load("_learn_route_cases", os.path.join(ROOT, "tests", "_learn_route_cases.py"))
build_recorder = act.build_recorder
policy_kernel_names = act.policy_kernel_names
short = act.short


def command(case):
    cfg = cases.cfg_of(case)
    return "policy %s %d %d 2 %d 0 %d" % (" ".join(str(cfg[k]) for k in cases.REF), case["T"], case["N"], case["bf16"], int(case["dhf"]))


def record(exe, lib, setting):
    """-> (registered kernel names, {case name: dict(cmd, ws, rc, fwd, bwd)}) for the cases of `setting`; `fwd` / `bwd` are
    event lists: (kernel, gx, gy, gz, bx, lds) or ("D", bytes)"""
    names = cases.cases_of(setting)
    env = {k: v for k, v in os.environ.items() if not k.startswith("EC_")}
    env.update(cases.SETTINGS[setting])
    r = subprocess.run([exe, lib], input="".join(command(cases.CASES[n]) + "\n" for n in names), capture_output=True, text=True,
                       env=env, timeout=600)
    assert r.returncode == 0, r.stderr
    registered, out, cur = [], [], None
    for line in r.stdout.splitlines():
        tag, rest = line[0], line[2:]
        if tag == "K":
            registered.append(short(rest))
        elif tag == "C":
            cur = dict(cmd=rest, ws=None, rc=None, fwd=None, bwd=[])
            out.append(cur)
        elif tag == "W":
            cur["ws"] = int(rest)
        elif tag == "L":
            f = rest.split("|")
            g, b = [int(x) for x in f[1].split(",")], [int(x) for x in f[2].split(",")]
            assert b[1:] == [1, 1], rest
            cur["bwd"].append((short(f[0]), g[0], g[1], g[2], b[0], int(f[3])))
        elif tag == "D":
            cur["bwd"].append(("D", int(rest)))
        elif tag == "F":                                     # the forward ends here
            assert int(rest) == 0 and cur["fwd"] is None, (cur["cmd"], rest)
            cur["fwd"], cur["bwd"] = cur["bwd"], []
        elif tag == "R":
            cur["rc"] = int(rest)
    assert [o["cmd"] for o in out] == [command(cases.CASES[n]) for n in names]
    assert all(o["fwd"] is not None for o in out)
    return sorted(registered), dict(zip(names, out))


def decode(table):
    """{case name: dict(cmd, ws, rc, fwd, bwd)} of the committed table, events as record() returns them"""
    def events(ev):
        return [("D", e[1]) if e[0] == "D" else (table["kernels"][e[0]], *e[1:]) for e in ev]
    return {n: dict(c, fwd=events(c["fwd"]), bwd=events(c["bwd"])) for n, c in table["cases"].items()}


if __name__ == "__main__":
    import tempfile
    sys.path.insert(0, ROOT)
    from embodied_clip_amd import _lib  # noqa: E402
    kernels, table = {}, {"parent_commit": PARENT_COMMIT, "cases": {}}

    def enc(ev):
        return [list(e) if e[0] == "D" else [kernels.setdefault(e[0], len(kernels)), *e[1:]] for e in ev]
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_recorder(tmp)
        for setting in cases.SETTINGS:
            registered, got = record(exe, _lib.LIB_PATH, setting)
            for n, c in got.items():
                table["cases"][n] = dict(c, fwd=enc(c["fwd"]), bwd=enc(c["bwd"]))
        mine = policy_kernel_names()
        table["policy_kernels"] = [k for k in registered if k.split("<")[0] in mine]
    table["cases"] = {n: table["cases"][n] for n in cases.CASES}
    table["kernels"] = list(kernels)
    with open(GOLDEN, "w") as f:
        f.write(json.dumps(table, separators=(",", ":")).replace('},"', '},\n"').replace('"cases":{', '"cases":{\n'))
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes from", _lib.LIB_PATH, "-", len(table["cases"]), "cases,", len(kernels), "kernels")

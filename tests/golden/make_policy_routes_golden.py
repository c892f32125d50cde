"""Records what a BUILT library launches for every inference case of tests/_act_route_cases.py, each under its switch setting
(CPU only: tools/launch_log.cpp stands in for the HIP runtime and its `policy` command drives the policy entry points):

    EC_AMD_LIB=/path/to/libec_amd.so python tests/golden/make_policy_routes_golden.py      (from the repository root)

  tests/golden/policy_routes_golden.json   `kernels`: the kernel names once; `policy_kernels`: every instance the library
                                           registers of a kernel that csrc/policy.hip defines; per case the command, the
                                           workspace size, the return code and the events of the recorded call (and, for a
                                           reuse case, of the table-building call in front of it): a launch is
                                           [kernel index, grid x, y, z, block x, dynamic LDS bytes], a device-to-device
                                           copy is ["D", bytes]

The committed table was written by the library of commit fdfd74d, the commit before tests/test_policy_routes.py existed:
that test holds every later build to it, launch for launch, so a change of an inference route has to re-record it on purpose.
The library reads its switches once per process: one recorder process per setting."""
import importlib.util
import json
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
GOLDEN = os.path.join(HERE, "policy_routes_golden.json")
PARENT_COMMIT = "fdfd74d"


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


conv = _load("make_conv_routes_golden", os.path.join(HERE, "make_conv_routes_golden.py"))
cases = _load("_act_route_cases", os.path.join(ROOT, "tests", "_act_route_cases.py"))
build_recorder = conv.build_recorder


def short(name):
    """`void (anonymous namespace)::k<1, 8>(args)` -> `k<1, 8>`"""
    name = conv.short(name)
    depth = 0
    for i, ch in enumerate(name):
        depth += (ch == "<") - (ch == ">")
        if ch == "(" and depth == 0:
            return name[:i]
    return name


def command(case):
    cfg = cases.cfg_of(case)
    return "policy %s %d %d 0 %d %d" % (" ".join(str(cfg[k]) for k in cases.REF), case["T"], case["N"], case["bf16"],
                                        int(case["mode"] == "reuse"))


def policy_kernel_names():
    """the kernels csrc/policy.hip defines"""
    src = open(os.path.join(ROOT, "embodied_clip_amd", "csrc", "policy.hip")).read()
    return set(re.findall(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", src))


def record(exe, lib, setting):
    """-> (registered kernel names, {case name: dict(cmd, ws, rc, build, call)}) for the cases of `setting`; `build` is None
    unless the case is a reuse pair, `call` / `build` are event lists: (kernel, gx, gy, gz, bx, lds) or ("D", bytes)"""
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
            cur = dict(cmd=rest, ws=None, rc=None, build=None, call=[])
            out.append(cur)
        elif tag == "W":
            cur["ws"] = int(rest)
        elif tag == "L":
            f = rest.split("|")
            g, b = [int(x) for x in f[1].split(",")], [int(x) for x in f[2].split(",")]
            assert b[1:] == [1, 1], rest
            cur["call"].append((short(f[0]), g[0], g[1], g[2], b[0], int(f[3])))
        elif tag == "D":
            cur["call"].append(("D", int(rest)))
        elif tag == "B":
            assert int(rest) == 0, (cur["cmd"], rest)
            cur["build"], cur["call"] = cur["call"], []
        elif tag == "R":
            cur["rc"] = int(rest)
    assert [o["cmd"] for o in out] == [command(cases.CASES[n]) for n in names]
    return sorted(registered), dict(zip(names, out))


def decode(table):
    """{case name: dict(cmd, ws, rc, build, call)} of the committed table, events as record() returns them"""
    def events(ev):
        return None if ev is None else [("D", e[1]) if e[0] == "D" else (table["kernels"][e[0]], *e[1:]) for e in ev]
    return {n: dict(c, build=events(c["build"]), call=events(c["call"])) for n, c in table["cases"].items()}


if __name__ == "__main__":
    import tempfile
    sys.path.insert(0, ROOT)
    from embodied_clip_amd import _lib  # noqa: E402
    kernels, table = {}, {"parent_commit": PARENT_COMMIT, "cases": {}}

    def enc(ev):
        return None if ev is None else [list(e) if e[0] == "D" else [kernels.setdefault(e[0], len(kernels)), *e[1:]] for e in ev]
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_recorder(tmp)
        for setting in cases.SETTINGS:
            registered, got = record(exe, _lib.LIB_PATH, setting)
            for n, c in got.items():
                table["cases"][n] = dict(c, build=enc(c["build"]), call=enc(c["call"]))
        mine = policy_kernel_names()
        table["policy_kernels"] = [k for k in registered if k.split("<")[0] in mine]
    table["cases"] = {n: table["cases"][n] for n in cases.CASES}
    table["kernels"] = list(kernels)
    with open(GOLDEN, "w") as f:
        f.write(json.dumps(table, separators=(",", ":")).replace('},"', '},\n"').replace('"cases":{', '"cases":{\n'))
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes from", _lib.LIB_PATH, "-", len(table["cases"]), "cases,", len(kernels), "kernels")

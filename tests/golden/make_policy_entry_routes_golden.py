"""Records what a BUILT library launches through the policy entry points that tests/golden/policy_routes_golden.json and
learn_routes_golden.json do not drive: the act entry points (`face` of tools/launch_log.cpp's `policy` command), the `_pa` pair
and the two-view net's (`twoview`), with the selection and forcing arguments of the heads launch dumped (CPU only):

    EC_AMD_LIB=/path/to/libec_amd.so python tests/golden/make_policy_entry_routes_golden.py      (from the repository root)

  tests/golden/policy_entry_routes_golden.json   `kernels`: the kernel names once; `cases`: command -> the recorder's lines for
                                                 it, a launch as `<kernel index>|grid|block|lds[|argument bytes]`

The committed table was written by the library of commit 2f47d9e, the last one whose entry points passed their arguments on
positionally; tests/test_policy_entry_routes.py holds every later build to it byte for byte.  What the dumped bytes are:
heads_fwd_kernel's SampleArgs, wa_heads_kernel's WaSelect (without its tail padding) and il_teacher_force_kernel's expert
pointer and probability -- outputs, greedy flag, seed, step, first actor, forcing pointers present or not."""
import importlib.util
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
GOLDEN = os.path.join(HERE, "policy_entry_routes_golden.json")
PARENT_COMMIT = "2f47d9e"

_spec = importlib.util.spec_from_file_location("make_policy_routes_golden", os.path.join(HERE, "make_policy_routes_golden.py"))
routes = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(routes)
build_recorder, short = routes.build_recorder, routes.short

# (kernel name part, bytes, argument index)
DUMPS = (("heads_fwd_kernel", 48, 9), ("wa_heads_kernel", 68, 9), ("il_teacher_force_kernel", 8, 1), ("il_teacher_force_kernel", 4, 3))

# the first 13 ec_policy_cfg fields: hidden = 64, spatial = 7, in_channels = 64
NARROW = "64 7 64 32 12 6 128 32 128 32 0 0 0"
VEC = "64 7 64 32 12 6 128 32 128 32 0 0 2"
WIDE = "64 7 64 32 12 20 128 32 128 32 0 0 0"
# ec_two_view_cfg: spatial = 2, in_channels = 64, hidden = 64, attn_hidden = 32; 20 actions; with / without previous actions; LSTM
TV_PA, TV = "64 2 64 32 20 8 1 1 1", "64 2 64 32 20 0 0 1 1"


def _policy(cfg, T, mode, reuse, face, pad=0, pnull=0, N=4):
    return "policy %s %d %d %d 1 %d 0 0 %d %d %d" % (cfg, T, N, mode, reuse, pad, pnull, face)


def commands():
    out = []
    for cfg, faces in ((NARROW, (1, 2, 3, 4)), (VEC, (1, 2, 3)), (WIDE, (3, 4))):          # the act entry points: infer, reuse
        out += [_policy(cfg, 1, 0, reuse, face) for face in faces for reuse in (0, 1)]
    for T in (1, 2):                                                                       # the 20-action handle's forward
        out += [_policy(WIDE, T, 0, 0, 0), _policy(WIDE, T, 0, 1, 0), _policy(WIDE, T, 2, 0, 0)]
    for T in (1, 2):                                                                       # previous actions: the _pa pair
        out += [_policy(NARROW, T, 0, 0, 5, 8, 1), _policy(NARROW, T, 0, 1, 5, 8, 1), _policy(NARROW, T, 2, 0, 5, 8, 1)]
    out += [_policy(NARROW, 1, 0, reuse, face, 8, 1) for face in (6, 7) for reuse in (0, 1)]
    out += [_policy(WIDE, 1, 0, 0, 7, 8, 0)]
    for cfg in (TV_PA, TV):                                                                # twoview: T N mode reuse inplace act
        for T in (1, 2):
            out += ["twoview %s %d 4 %d %d 0 0" % (cfg, T, mode, reuse) for mode, reuse in ((0, 0), (0, 1), (2, 0))]
        out += ["twoview %s 1 4 0 %d %d %d" % (cfg, reuse, inplace, act) for act in (1, 2) for reuse, inplace in ((0, 0), (1, 0), (0, 1))]
    assert len(set(out)) == len(out)
    return out


def record(exe, lib):
    """-> (kernel names in order of first use, {command: lines}) of commands()"""
    cmds = commands()
    args = [exe, lib]
    for of, n, idx in DUMPS:
        args += ["--args-of", of, str(n), str(idx)]
    env = {k: v for k, v in os.environ.items() if not k.startswith("EC_")}
    r = subprocess.run(args, input="".join(c + "\n" for c in cmds), capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr
    kernels, cases, cur = {}, {}, None
    for line in r.stdout.splitlines():
        tag, rest = line[0], line[2:]
        if tag == "K":
            continue
        if tag == "C":
            cur = cases.setdefault(rest, [])
        elif tag == "L":
            f = rest.split("|")
            cur.append("|".join([str(kernels.setdefault(short(f[0]), len(kernels)))] + f[1:]))
        else:
            cur.append(line)
    assert list(cases) == cmds
    return list(kernels), cases


if __name__ == "__main__":
    import tempfile
    sys.path.insert(0, ROOT)
    from embodied_clip_amd import _lib  # noqa: E402
    with tempfile.TemporaryDirectory() as tmp:
        kernels, cases = record(build_recorder(tmp), _lib.LIB_PATH)
    for cmd, lines in cases.items():
        assert lines[-1] == "R 0" and lines[0].startswith("W "), (cmd, lines[-1])
    with open(GOLDEN, "w") as f:
        json.dump({"parent_commit": PARENT_COMMIT, "kernels": kernels, "cases": cases}, f, indent=0, separators=(",", ":"))
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes from", _lib.LIB_PATH, "-", len(cases), "cases,", len(kernels), "kernels")

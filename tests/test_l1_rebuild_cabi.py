"""Layer 1's rebuilt identity on a box without a GPU: ``ec_rn50_set_l1_rebuild`` and ``ec_conv1x1_pair_rebuild_bf16`` declared, bound
and exported; their refusals in front of the first HIP call; and, through tools/launch_log.cpp standing in for the HIP runtime, the
launch list of a 128-frame CLIP RN50 forward: with the option off exactly the recorded table's (tests/golden/conv_routes_golden.json),
with it on the same 37 launches but for the layer1.1 boundary's kernel and the layer1.0 boundary's NULL y."""
import importlib.util
import json
import os
import re
import shutil
import subprocess

import pytest

NEW = ("ec_rn50_set_l1_rebuild", "ec_conv1x1_pair_rebuild_bf16")
ARG, SHAPE, UNSUPPORTED = -1, -2, -6
P = 0x1000          # a non-NULL, 16-byte aligned pointer that is never dereferenced
L50 = (3, 4, 6, 3)
PAIR0, PAIR1 = "conv1x1_pair_kernel<true, false, 64, false>(PairArgs)", "conv1x1_pair_kernel<false, true, 64, false>(PairArgs)"
REBUILD = "conv1x1_pair_rebuild_kernel(RebuildArgs)"
LDS_REBUILD = 4 * 32768 + (256 + 256 + 64) * 4 + 4 * 32 * 144      # four weight images, three bias vectors, a quarter-row staging per wave
Y_AT = 9 * 8        # PairArgs: six operand pointers, three bias pointers, then y
CXX = os.environ.get("CXX", "c++")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from embodied_clip_amd import _lib
    return _lib.load()


def test_symbols_are_declared_exported_and_bound(lib, repo_root):
    from embodied_clip_amd import _lib
    text = open(os.path.join(repo_root, "include", "ec_amd.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, header) and n in _lib.SIGNATURES and hasattr(lib, n), n


def test_refusals_need_no_hip(lib):
    names = ("a", "w3", "b3", "i0", "wi0", "bi0", "i1", "wi1", "bi1", "y", "w2", "b2", "z")

    def f(M=64, K0=64, N=256, N2=64, **null):
        return lib.ec_conv1x1_pair_rebuild_bf16(*[None if n in null else P for n in names], M, K0, N, N2, None)
    for n in names:
        assert f(**{n: None}) == ARG, n
    for M in (0, -32, 33, 48):
        assert f(M=M) == SHAPE, M
    assert f(K0=128) == SHAPE and f(N=512) == SHAPE and f(N2=128) == SHAPE and f(N2=32) == SHAPE
    assert f(a=None, M=33) == ARG           # pointers first
    assert lib.ec_rn50_set_l1_rebuild(None, 1) == ARG
    # the pair launch takes a NULL y at the layer-1 widths only: the layer-2 kernel always stores it
    pair = lambda y, K0, N, N2: lib.ec_conv1x1_pair_bf16(P, P, P, None, None, None, P, y, P, P, P, 64, K0, N, N2, None)  # noqa: E731
    assert pair(None, 128, 512, 128) == ARG and pair(None, 64, 256, 32) == SHAPE


# ---- the recorder stands in for the HIP runtime ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def conv():
    spec = importlib.util.spec_from_file_location("make_conv_routes_golden", os.path.join(ROOT, "tests", "golden", "make_conv_routes_golden.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    return g


@pytest.fixture(scope="module")
def recorder(conv, tmp_path_factory):
    if shutil.which(CXX) is None:
        pytest.skip("host C++ compiler not found")
    return conv.build_recorder(str(tmp_path_factory.mktemp("launch_log_l1")), CXX)


def _run(conv, recorder, cmds):
    """-> per command: rc, the setter's return codes, the `P` line, the launches of the handle's creation and of the forward as
    [(kernel, gx, gy, gz, bx, by, bz, lds)], and per launch of the forward the y pointer of a pair kernel's argument block (None for
    the other kernels)"""
    from embodied_clip_amd import _lib
    env = {k: v for k, v in os.environ.items() if not k.startswith("EC_")}
    r = subprocess.run([recorder, _lib.LIB_PATH, "--args-of", "conv1x1_pair_kernel", str(Y_AT + 8)], input="".join(c + "\n" for c in cmds),
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr
    out = []
    for line in r.stdout.splitlines():
        tag, rest = line[0], line[2:]
        if tag == "C":
            out.append(dict(rc=None, set=[], plan=None, create=[], launches=[], y=[]))
        elif tag == "S":
            out[-1]["set"].append(int(rest))
        elif tag == "P":
            out[-1]["plan"] = rest.split()
            out[-1]["create"] = list(out[-1]["launches"])      # the weight packing of the handle's creation
            out[-1]["launches"].clear()
            out[-1]["y"].clear()
        elif tag == "L":
            f = rest.split("|")
            out[-1]["launches"].append((conv.short(f[0]), *map(int, f[1].split(",")), *map(int, f[2].split(",")), int(f[3])))
            out[-1]["y"].append(int.from_bytes(bytes.fromhex(f[4])[Y_AT:Y_AT + 8], "little") if len(f) > 4 else None)
        elif tag == "R":
            out[-1]["rc"] = int(rest)
    assert len(out) == len(cmds)
    return out


@pytest.mark.parametrize("min_tiles", [0, 50])
def test_option_off_is_the_recorded_plan_and_on_changes_two_launches(conv, recorder, min_tiles):
    case = conv.tower("clip", L50, 128, min_tiles=min_tiles)
    off, on, back = _run(conv, recorder, [case, case + "+l1", case + "+l1off"])
    assert off["rc"] == on["rc"] == back["rc"] == 0 and on["set"] == [0] and back["set"] == [0, 0]
    # off: launch by launch what the parent's table records for this very call (kernel instance, grid, block, LDS size)
    table = json.load(open(conv.GOLDEN))
    assert case in conv.CASES and (0, off["create"] + off["launches"]) == conv.decode(table, "default")[case]
    assert len(off["launches"]) == 37
    # ... and a handle that had the option on and off again is the default handle: plan hash and launches
    assert back["plan"] == off["plan"] and back["launches"] == off["launches"] and [y == 0 for y in back["y"]] == [y == 0 for y in off["y"]]
    # on: the same number of ops and launches, another hash
    assert on["plan"][0] == off["plan"][0] and on["plan"][1] != off["plan"][1] and len(on["launches"]) == 37
    diff = [i for i in range(37) if on["launches"][i] != off["launches"][i]]
    (i0,) = [i for i, l in enumerate(off["launches"]) if l[0] == PAIR0]
    (i1,) = [i for i, l in enumerate(off["launches"]) if l[0] == PAIR1]
    assert diff == [i1] and i1 == i0 + 2            # (block 1's conv2 between the two boundaries)
    # the layer1.1 boundary: the new kernel on the same grid and block, with its own LDS size
    assert on["launches"][i1] == (REBUILD,) + off["launches"][i1][1:7] + (LDS_REBUILD,)
    # the layer1.0 boundary: the same instance, y NULL (it was a buffer)
    assert on["launches"][i0] == off["launches"][i0] and off["y"][i0] != 0 and on["y"][i0] == 0
    assert all(y != 0 for i, y in enumerate(off["y"]) if off["launches"][i][0] in (PAIR0, PAIR1))


def test_small_launches_take_the_same_two_changes(conv, recorder):
    """3 frames: below every frame threshold of the executor"""
    case = conv.tower("clip", L50, 3)
    off, on = _run(conv, recorder, [case, case + "+l1"])
    assert off["rc"] == on["rc"] == 0 and len(on["launches"]) == len(off["launches"])
    diff = [i for i in range(len(off["launches"])) if on["launches"][i] != off["launches"][i]]
    assert [off["launches"][i][0] for i in diff] == [PAIR1] and [on["launches"][i][0] for i in diff] == [REBUILD]


def test_towers_without_the_two_boundaries_refuse_the_setter(conv, recorder):
    cases = [conv.tower("tvb", L50, 3) + "+l1",                                   # torchvision Bottleneck tower
             conv.tower("tvbasic", (2, 2, 2, 2), 3) + "+l1",                      # BasicBlock tower
             conv.tower("clip", (2, 4, 6, 3), 3) + "+l1",                         # layer1.1 is the pooled layer-1 -> layer-2 boundary
             conv.tower("clip", (6, 8, 18, 8), 2, width=96, res=384) + "+l1"]     # RN50x16: no fused boundaries at width 96
    plain = _run(conv, recorder, [c[:-3] for c in cases])
    for got, want in zip(_run(conv, recorder, cases), plain):
        assert got["set"] == [UNSUPPORTED] and got["rc"] == 0
        assert got["plan"] == want["plan"] and got["launches"] == want["launches"]      # the handle is unchanged

"""The RGB-D encoder of the pooled net on a box without a GPU: ``ec_spatial_mean_pair_bf16`` and ``ec_rn50_embed_rgbd`` declared,
bound and exported; their refusals in front of the first HIP call; and, through tools/launch_log.cpp standing in for the HIP
runtime, the launch list of the joint pass: the RGB tower's list at twice the frames with the stem launch split in two and one
pool launch appended; chunks counted in pairs; the composed route under EC_RGBD_JOINT=0.  The engine's new refusals need no GPU
either."""
import ctypes as C
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

NEW = ("ec_spatial_mean_pair_bf16", "ec_rn50_rgbd_workspace_bytes", "ec_rn50_embed_rgbd")
ARG, SHAPE, WORKSPACE, UNSUPPORTED = -1, -2, -4, -6
P = 0x1000          # a non-NULL, 16-byte aligned pointer that is never dereferenced: the recorder launches nothing for real
RGB_STEM, DEPTH_STEM, POOL = "stem_conv1_kernel<32, false>", "stem_conv1_depth_kernel<32>", "spatial_mean_pair_kernel"
L50 = (3, 4, 6, 3)
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
    # each cites what it replaces, as the header does throughout
    for n in ("ec_spatial_mean_pair_bf16", "ec_rn50_rgbd_workspace_bytes"):
        comment = text[:re.search(r"^(?:int|size_t) %s\(" % n, text, re.M).start()]
        comment = " ".join(comment[comment.rindex("/*"):].replace("*", " ").split())
        assert "[U]" in comment and "ResNetCLIPEncoder" in comment and "parity unpinned" in comment, n


def test_pair_kernel_refusals_need_no_hip(lib):
    f = lambda a=P, b=P, out=P, B=2, HW=49, Cc=64: lib.ec_spatial_mean_pair_bf16(a, b, out, B, HW, Cc, None)
    for k in ("a", "b", "out"):
        assert f(**{k: None}) == ARG, k
    for k in ("B", "HW", "Cc"):
        assert f(**{k: 0}) == SHAPE and f(**{k: -3}) == SHAPE, k
    assert f(a=None, B=0) == ARG            # pointers first


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
    return conv.build_recorder(str(tmp_path_factory.mktemp("launch_log_rgbd")), CXX)


def _name(name):
    """`k<1, 8>(args)` -> `k<1, 8>`"""
    depth = 0
    for i, ch in enumerate(name):
        depth += (ch == "<") - (ch == ">")
        if ch == "(" and depth == 0:
            return name[:i]
    return name


def _run(conv, recorder, cmds, env_extra=None):
    """-> [(rc, [(kernel, gx, gy, gz, bx, by, bz, lds)])] per command; the launches of the handle's creation (weight packing, in front
    of the `P` line) are dropped"""
    from embodied_clip_amd import _lib
    env = {k: v for k, v in os.environ.items() if not k.startswith("EC_")}
    env.update(env_extra or {})
    r = subprocess.run([recorder, _lib.LIB_PATH], input="".join(c + "\n" for c in cmds), capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr
    out = []
    for line in r.stdout.splitlines():
        tag, rest = line[0], line[2:]
        if tag == "C":
            out.append([None, []])
        elif tag == "P":
            out[-1][1].clear()
        elif tag == "L":
            f = rest.split("|")
            out[-1][1].append((_name(conv.short(f[0])), *map(int, f[1].split(",")), *map(int, f[2].split(",")), int(f[3])))
        elif tag == "R":
            out[-1][0] = int(rest)
    assert len(out) == len(cmds)
    return [(rc, ls) for rc, ls in out]


def _split_stem(f32_list, rgb_stem_at, depth_stem_at):
    """the f32 list with its ONE stem launch replaced by the RGB stem and the depth stem launches given"""
    stems = [i for i, l in enumerate(f32_list) if l[0] == RGB_STEM]
    assert stems == [0], stems
    return [rgb_stem_at, depth_stem_at] + f32_list[1:]


@pytest.mark.parametrize("pairs", [4, 128])
def test_joint_pass_is_the_rgb_list_at_twice_the_frames(conv, recorder, pairs):
    cmds = [conv.tower("clip", L50, pairs, inp="rgbd"), conv.tower("clip", L50, 2 * pairs), conv.tower("clip", L50, pairs),
            conv.tower("clip", L50, pairs, inp="depth")]
    (rc, got), (rc2, twice), (rc1, once), (rcd, dep) = _run(conv, recorder, cmds)
    assert rc == rc2 == rc1 == rcd == 0
    assert once[0][0] == RGB_STEM and dep[0][0] == DEPTH_STEM
    # kernel instance by kernel instance, with grid, block and LDS size: every op behind the stem runs ONCE, at 2 * pairs frames;
    # the stem is the RGB kernel, then the depth kernel, each at `pairs` frames
    assert got[:-1] == _split_stem(twice, once[0], dep[0])
    assert got[-1][0] == POOL and got[-1][1:] == (pairs * 8, 1, 1, 256, 1, 1, 0)      # 2048 channels: 8 slabs of 256 per pair
    assert [l[0] for l in got].count(POOL) == 1 and len(got) == len(twice) + 2


def test_chunks_count_pairs(conv, recorder):
    cmds = [conv.tower("clip", L50, 5, chunk=2, inp="rgbd"), conv.tower("clip", L50, 2, inp="rgbd"), conv.tower("clip", L50, 1, inp="rgbd")]
    (rc, got), (_, two), (_, one) = _run(conv, recorder, cmds)
    assert rc == 0 and got == two + two + one


def test_composed_route_under_the_switch(conv, recorder):
    for pairs in (4, 128):
        cmds = [conv.tower("clip", L50, pairs, inp="rgbd"), conv.tower("clip", L50, pairs), conv.tower("clip", L50, pairs, inp="depth")]
        (rc, got), (_, rgb), (_, dep) = _run(conv, recorder, cmds, env_extra={"EC_RGBD_JOINT": "0"})
        assert rc == 0 and got[:-1] == rgb + dep and got[-1][0] == POOL
    # ... chunked: per chunk RGB, depth, pool
    cmds = [conv.tower("clip", L50, 3, chunk=2, inp="rgbd"), conv.tower("clip", L50, 2), conv.tower("clip", L50, 2, inp="depth"),
            conv.tower("clip", L50, 1), conv.tower("clip", L50, 1, inp="depth")]
    (rc, got), (_, r2), (_, d2), (_, r1), (_, d1) = _run(conv, recorder, cmds, env_extra={"EC_RGBD_JOINT": "0"})
    pool = [l for l in got if l[0] == POOL]
    assert rc == 0 and len(pool) == 2 and got == r2 + d2 + pool[:1] + r1 + d1 + pool[1:]


def test_the_switch_is_not_part_of_the_plan_hash(conv, recorder):
    from embodied_clip_amd import _lib

    def plan(env_extra):
        env = {k: v for k, v in os.environ.items() if not k.startswith("EC_")}
        env.update(env_extra)
        r = subprocess.run([recorder, _lib.LIB_PATH], input=conv.tower("clip", L50, 2) + "\n", capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, r.stderr
        return [l for l in r.stdout.splitlines() if l.startswith("P ")]
    assert plan({}) == plan({"EC_RGBD_JOINT": "0"}) and len(plan({})) == 1


def test_a_torchvision_stem_handle_is_unsupported(conv, recorder):
    for kind in ("tvb", "tvbasic"):
        ((rc, got),) = _run(conv, recorder, [conv.tower(kind, (1, 1, 1, 1), 2, res=64, inp="rgbd")])
        assert rc == UNSUPPORTED and got == []


def test_embed_rgbd_null_arguments(lib):
    """NULL arguments are refused before the handle is read: no handle is needed"""
    m3 = (C.c_float * 3)(0.5, 0.5, 0.5)
    call = lambda h=P, rgb=P, u8=0, mean=None, std=None, depth=P, w9=P, pairs=2, ws=P, nws=1 << 40, embed=P: lib.ec_rn50_embed_rgbd(
        h, rgb, u8, mean, std, depth, 1.0, 0.0, w9, pairs, ws, nws, embed, 0, None)
    for k in ("h", "rgb", "depth", "w9", "ws", "embed"):
        assert call(**{k: None}) == ARG, k
    assert call(u8=1) == ARG and call(u8=1, mean=m3) == ARG and call(u8=1, std=m3) == ARG
    assert lib.ec_rn50_rgbd_workspace_bytes(None, 4) == 0


def test_embed_rgbd_shape_and_workspace_refusals(tmp_path):
    """pairs <= 0 and a short workspace, on a real handle: a small host program against the recorder's stand-in runtime"""
    if shutil.which(CXX) is None:
        pytest.skip("host C++ compiler not found")
    from embodied_clip_amd import _lib
    src = tmp_path / "refuse.cpp"
    # the recorder defines the HIP entry points; this program includes it for them and drives the library itself
    src.write_text(r'''
#define main launch_log_main
#include "%s"
#undef main
int main(int, char** argv) {
    g_lib = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
    if (!g_lib) return 2;
    typedef void* P;
    const int layers[4] = {1, 1, 1, 1};
    void* h = nullptr;
    const P w = fake(1u << 30), f = fake(1u << 28), stem = fake(1u << 20), rgb = fake(1u << 30), out = fake(1u << 30), w9 = fake(1u << 20);
    size_t nw = 0, nb = 0;
    resnet_counts(layers, false, nw, nb, 64);
    int rc = sym<int (*)(P*, int, const int*, int, P, P, size_t, P, size_t)>("ec_rn50_create")(&h, 64, layers, 64, stem, w, nw + 32 * 288 + 64 * 288, f, nb + 128);
    if (rc) return 3;
    printf("H\n");
    auto embed = sym<int (*)(P, P, int, const float*, const float*, P, float, float, P, int, P, size_t, P, int, P)>("ec_rn50_embed_rgbd");
    auto bytes = sym<size_t (*)(P, int)>("ec_rn50_rgbd_workspace_bytes");
    auto plain = sym<size_t (*)(P, int)>("ec_rn50_workspace_bytes");
    const size_t ws = bytes(h, 3);
    printf("S %%d %%d\n", embed(h, rgb, 0, nullptr, nullptr, rgb, 1.f, 0.f, w9, 0, out, ws, out, 0, nullptr),
           embed(h, rgb, 0, nullptr, nullptr, rgb, 1.f, 0.f, w9, -2, out, ws, out, 0, nullptr));
    printf("W %%d %%d\n", embed(h, rgb, 0, nullptr, nullptr, rgb, 1.f, 0.f, w9, 3, out, ws - 1, out, 0, nullptr),
           embed(h, rgb, 0, nullptr, nullptr, rgb, 1.f, 0.f, w9, 3, out, plain(h, 6), out, 0, nullptr));
    // the plan's buffers at 2 * pairs frames plus the [2 * pairs, S, S, C] bf16 maps; chunk 2 of 3 pairs needs the size at 2 pairs
    printf("B %%zu %%zu %%d\n", ws, plain(h, 6), sym<int (*)(P)>("ec_rn50_out_channels")(h) * 2 * 2 * 6 * 2);
    printf("C %%d\n", embed(h, rgb, 0, nullptr, nullptr, rgb, 1.f, 0.f, w9, 3, out, bytes(h, 2), out, 2, nullptr));
    return 0;
}
''' % os.path.join(ROOT, "tools", "launch_log.cpp"))
    exe = str(tmp_path / "refuse")
    subprocess.run([CXX, "-O1", "-std=c++17", "-rdynamic", "-o", exe, str(src), "-ldl"], check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("EC_")}
    r = subprocess.run([exe, _lib.LIB_PATH], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    tags = [l[0] for l in lines]
    # no launch in front of a refusal: behind the handle's creation, the first `L` line belongs to the chunked call that runs
    assert "L" not in tags[tags.index("H"):tags.index("B")] and "L" in tags[tags.index("B"):], lines[:8]
    rec = {l[0]: l[2:].split() for l in lines if l[0] in "SWBC"}
    assert rec["S"] == [str(SHAPE)] * 2 and rec["W"] == [str(WORKSPACE)] * 2 and rec["C"] == ["0"]
    ws, plain6, maps = map(int, rec["B"])
    assert ws == plain6 + maps          # (width 64 at 64 x 64: a 2 x 2 x 2048 map per frame, already a multiple of 256 bytes)


def test_engine_refusals_need_no_gpu():
    """``check_net`` is the constructors' first statement: what the pooled RGB-D agent refuses is raised before the library loads"""
    from embodied_clip_amd.engine import Worker, check_net
    from embodied_clip_amd.evaluate import Evaluator
    assert check_net("pooled", "avgpool", (2, 2), True, "rn50", True, False, 0) == (True, "avgpool", (2, 2))
    for cls in (Worker, Evaluator):
        for bad in (dict(pooling="attnpool"), dict(encoder="imagenet_rn18"), dict(encoder="imagenet_rn50"), dict(encoder="rn50x16"),
                    dict(zeroshot=True), dict(goal_in=2), dict(encoder="vit")):
            with pytest.raises(ValueError):
                cls(8, T=4, device="cuda:0", **{**dict(net="pooled", pooling="avgpool", depth=True), **bad})
    with pytest.raises(ValueError):
        Worker(8, T=4, device="cuda:0", net="pooled", pooling="avgpool", depth=True, frames_host=True)
    # the goal-encoder agent keeps its refusals: the helpers' behaviour is what it was
    for kw in (dict(prev_actions=32), dict(rnn_type="LSTM"), dict(rnn_layers=2)):
        for cls in (Worker, Evaluator):
            with pytest.raises(ValueError, match="depth=True"):
                cls(8, T=4, device="cuda:0", depth=True, **kw)

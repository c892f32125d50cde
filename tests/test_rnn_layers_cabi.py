"""Multi-layer recurrent cores on a box without a GPU: the new symbols declared, exported and bound; one layer through the new
constructor is today's handle (the golden layout); the layouts of L = 2, 3; every refusal in front of the first HIP call; and
the act step's launch count, 5 + (L - 1) with reused tables (tools/launch_log.cpp stands in for the HIP runtime)."""
import ctypes as C
import importlib.util
import json
import os
import re
import shutil
import subprocess

import pytest

NEW = ("ec_policy_create_rnn_layers", "ec_policy_rnn_layers", "ec_rnn_stack_step_fwd")
REFERENCE = dict(in_channels=2048, spatial=7, hidden=512, goal_dims=32, num_goals=12, num_actions=6, compress_hid=128, compress_out=32,
                 comb_hid=128, comb_out=32, fusion=0, dual=0, goal_in=0)
GRU, LSTM = 0, 1
P = 64        # a non-NULL "pointer": the checks under test return before anything is read
STACK_KERNELS = ("rnn_stack_step_kernel<false>", "rnn_stack_step_kernel<true>")


@pytest.fixture(scope="module")
def lib():
    from embodied_clip_amd import _lib
    return _lib.load()


def _create(lib, rnn, layers, **kw):
    from embodied_clip_amd import _lib
    h = C.c_void_p()
    return lib.ec_policy_create_rnn_layers(C.byref(h), C.byref(_lib.PolicyCfg(**dict(REFERENCE, **kw))), rnn, layers), h


def _layout(lib, h, shapes):
    offs = []
    for i in range(lib.ec_policy_num_param_tensors(h)):
        off, num = C.c_size_t(), C.c_size_t()
        assert lib.ec_policy_param_offset(h, i, C.byref(off), C.byref(num)) == 0
        offs.append([off.value, num.value])
    return dict(flat_size=lib.ec_policy_flat_size(h), param_offsets=offs,
                workspace_bytes=[[T, N, b, lib.ec_policy_workspace_bytes(h, T, N, b)] for T, N in shapes for b in (0, 1)])


def test_symbols_are_declared_exported_and_bound(lib, repo_root):
    from embodied_clip_amd import _lib
    text = open(os.path.join(repo_root, "include", "ec_amd.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, header) and n in _lib.SIGNATURES and hasattr(lib, n), n
    assert re.search(r"#define\s+EC_RNN_MAX_LAYERS\s+4\b", header)
    # no field was added to the configuration struct: the depth is an argument of the new constructor
    assert [f[0] for f in _lib.PolicyCfg._fields_][-2:] == ["prev_action_dims", "prev_action_null"]
    assert "[N, L*SW]" in text and "Non-overlap" in text and "Alignment" in text


def test_one_layer_is_todays_handle(lib, repo_root):
    """num_layers = 1 through the new constructor: the golden layout of tests/golden/policy_layout_golden.json, tensor for tensor
    and workspace for workspace; and ec_policy_create_rnn's LSTM handle."""
    golden = json.load(open(os.path.join(repo_root, "tests", "golden", "policy_layout_golden.json")))
    for name in ("reference", "small", "small7"):
        g = golden[name]
        order = [(T, N) for T, N, _, _ in g["workspace_bytes"]]
        shapes = sorted(set(order), key=order.index)
        rc, h = _create(lib, GRU, 1, **g["cfg"])
        assert rc == 0
        try:
            got = _layout(lib, h, shapes)
            assert got["flat_size"] == g["flat_size"] and got["param_offsets"] == g["param_offsets"], name
            assert got["workspace_bytes"] == g["workspace_bytes"], name
            assert lib.ec_policy_rnn_layers(h) == 1 and lib.ec_policy_state_width(h) == g["cfg"]["hidden"]
        finally:
            lib.ec_policy_destroy(h)
    from embodied_clip_amd import _lib
    shapes = [(1, 1), (1, 32), (8, 5), (128, 32)]
    for rnn in (GRU, LSTM):
        old = C.c_void_p()
        assert lib.ec_policy_create_rnn(C.byref(old), C.byref(_lib.PolicyCfg(**REFERENCE)), rnn) == 0
        rc, new = _create(lib, rnn, 1)
        assert rc == 0 and _layout(lib, old, shapes) == _layout(lib, new, shapes)
        assert lib.ec_policy_rnn_layers(old) == 1
        lib.ec_policy_destroy(old)
        lib.ec_policy_destroy(new)
    assert lib.ec_policy_rnn_layers(None) == 0


@pytest.mark.parametrize("L", [2, 3])
@pytest.mark.parametrize("rnn", ["GRU", "LSTM"])
@pytest.mark.parametrize("kw", [{}, dict(goal_in=3, num_actions=4), dict(hidden=64, in_channels=64, num_actions=84, prev_action_dims=32,
                                                                          prev_action_null=1)])
def test_layered_layout(kw, rnn, L):
    from embodied_clip_amd import synthetic as syn
    from embodied_clip_amd.policy import PolicyHandle
    one, h = PolicyHandle(rnn_type=rnn, **kw), PolicyHandle(rnn_type=rnn, rnn_layers=L, **kw)
    H = h.H
    G, SW = (4 * H, 2 * H) if rnn == "LSTM" else (3 * H, H)
    assert h.rnn_layers == L and h.state_width == L * SW and one.state_width == SW
    # every tensor of the single-layer handle keeps its index, offset and shape; the upper layers' END the order
    names = list(h.offsets)
    assert names[:len(one.offsets)] == list(one.offsets) and len(names) == len(one.offsets) + 4 * (L - 1)
    assert all(h.offsets[n] == one.offsets[n] and h.shapes[n] == one.shapes[n] for n in one.offsets)
    upper = [f"state_encoder.rnn.{k}_l{l}" for l in range(1, L) for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    assert names[len(one.offsets):] == upper == [k for l in range(1, L) for k in syn.policy_rnn_layer_tensors(l)]
    end = max(o + k for (o, k) in one.offsets.values())
    for n in upper:
        assert h.shapes[n] == ((G, H) if "weight" in n else (G,)) and h.offsets[n][0] >= end and h.offsets[n][0] % 4 == 0
        end = h.offsets[n][0] + h.offsets[n][1]
    assert end <= h.flat_size < end + 4
    assert h.recurrent_section() == one.recurrent_section()                 # it keeps its meaning
    for (T, N) in ((1, 1), (1, 32), (8, 5), (128, 32)):
        for mode in (False, True):
            assert h.workspace_bytes(T, N, mode) >= one.workspace_bytes(T, N, mode) + 4 * (L - 1) * T * N * (G + H), (T, N, mode)
    sd = syn.policy_state_dict(0, **h.cfg, rnn_type=rnn, rnn_layers=L)
    assert list(sd) == names and all(tuple(sd[n].shape) == tuple(h.shapes[n]) for n in names)
    assert float(sd[upper[0]].std()) > 0 and float(sd[upper[1]].std()) > 0


def test_refusals(lib):
    for L in (0, -1, 5):
        assert _create(lib, GRU, L)[0] == -1 and _create(lib, LSTM, L)[0] == -1          # EC_ERR_ARG outside 1..4
    assert _create(lib, 2, 2)[0] == -1
    assert _create(lib, GRU, 2, dual=1)[0] == -6 and _create(lib, GRU, 2, fusion=1, spatial=1)[0] == -6   # EC_ERR_UNSUPPORTED
    assert _create(lib, LSTM, 2, dual=1)[0] == -6
    rc, h = _create(lib, GRU, 1, dual=1)                                              # (one layer: the two-tower agent as before)
    assert rc == 0
    lib.ec_policy_destroy(h)
    assert _create(lib, LSTM, 2, hidden=40)[0] == -2 and _create(lib, LSTM, 2, hidden=640)[0] == -2
    rc, h = _create(lib, GRU, 4, hidden=40)                                           # a GRU stack takes it (the general route)
    assert rc == 0 and lib.ec_policy_state_width(h) == 160 and lib.ec_policy_rnn_layers(h) == 4
    off, num = C.c_size_t(), C.c_size_t()
    n = lib.ec_policy_num_param_tensors(h)
    assert n == 17 + 12 and lib.ec_policy_param_offset(h, n - 1, C.byref(off), C.byref(num)) == 0 and num.value == 120
    assert lib.ec_policy_param_offset(h, n, C.byref(off), C.byref(num)) == -1
    lib.ec_policy_destroy(h)
    from embodied_clip_amd.policy import PolicyHandle
    for bad in (0, 5, "2"):
        with pytest.raises(ValueError):
            PolicyHandle(rnn_layers=bad)
    with pytest.raises(ValueError):
        PolicyHandle(rnn_layers=2, dual=1)


def test_step_argument_checks(lib):
    def step(rnn=LSTM, x=P, ldx=64, wih=P, whh=P, bih=P, bhh=P, st=P, ld=128, mask=P, h=P, ldh=64, c=P, ldc=64, h2=None, ldh2=0, N=4, H=64):
        return lib.ec_rnn_stack_step_fwd(rnn, x, ldx, wih, whh, bih, bhh, st, ld, mask, h, ldh, c, ldc, h2, ldh2, N, H, None)
    for k in ("x", "wih", "whh", "bih", "bhh", "st", "mask", "h", "c"):
        assert step(**{k: None}) == -1, k
    assert step(rnn=GRU, c=None, ld=64, N=0) == -2                    # (a GRU step needs no c_out: the next check answers)
    assert step(rnn=2) == -1 and step(rnn=-1) == -1
    for kw in (dict(N=0), dict(H=40), dict(H=0), dict(H=640, ldx=640, ld=1280, ldh=640, ldc=640), dict(ldx=60), dict(ldx=66), dict(ld=64),
               dict(ld=130), dict(ldh=32), dict(ldc=60), dict(h2=P, ldh2=32), dict(rnn=GRU, ld=60)):
        assert step(**kw) == -2, kw
    for k in ("x", "wih", "whh", "st"):
        assert step(**{k: P + 4}) == -1, k                            # 16-byte alignment of the staged operands


# ---- launches ---------------------------------------------------------------------------------------------------------------------
CXX = os.environ.get("CXX", "c++")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def routes():
    spec = importlib.util.spec_from_file_location("make_policy_routes_golden", os.path.join(ROOT, "tests", "golden", "make_policy_routes_golden.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    return g


@pytest.fixture(scope="module")
def recorder(routes, tmp_path_factory):
    if shutil.which(CXX) is None:
        pytest.skip("host C++ compiler not found")
    return routes.build_recorder(str(tmp_path_factory.mktemp("launch_log_layers")), CXX)


def _act_launches(routes, recorder, cores, env_extra=None, N=32, T=1, reuse=1, hidden=512):
    """-> {core: [kernel names of the recorded call]} for the reference handle's act step with reused tables"""
    from embodied_clip_amd import _lib
    cfg = dict(REFERENCE, hidden=hidden)
    fields = " ".join(str(cfg.get(f[0], 0)) for f in _lib.PolicyCfg._fields_[:13])
    cmds = "".join("policy %s %d %d 0 1 %d 0%s\n" % (fields, T, N, reuse, (" %d" % core) if core else "") for core in cores)
    env = {k: v for k, v in os.environ.items() if not k.startswith("EC_")}
    env.update(env_extra or {})
    r = subprocess.run([recorder, _lib.LIB_PATH], input=cmds, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr
    out, cur, seen_b = {}, None, False
    it = iter(cores)
    for line in r.stdout.splitlines():
        tag, rest = line[0], line[2:]
        if tag == "C":
            cur = out.setdefault(next(it), [])
        elif tag == "B":
            assert int(rest) == 0
            cur.clear()                                       # what came before built the tables
        elif tag == "L":
            cur.append(routes.short(rest.split("|")[0]))
        elif tag == "D":
            cur.append("D")
        elif tag == "R":
            assert int(rest) == 0, line
    return out


def test_existing_recorder_forms_are_unchanged(routes, recorder):
    """the policy command without the trailing argument, and with it naming a one-layer GRU: the same launches"""
    got = _act_launches(routes, recorder, [0, 1])
    assert got[0] == got[1] and len(got[0]) == 5


@pytest.mark.parametrize("hidden", [512, 64])
def test_act_step_is_five_launches_plus_one_per_upper_layer(routes, recorder, hidden):
    cores = [0, 1, 2, 3, 4, 11, 12, 13, 14]
    got = _act_launches(routes, recorder, cores, hidden=hidden)
    for core in cores:
        L = max(core % 10, 1)
        ran = got[core]
        assert len(ran) == 5 + (L - 1), (core, ran)
        assert "D" not in ran                                              # no copy on the serial chain
        stack = [k for k in ran if k in STACK_KERNELS]
        lstm = core >= 10
        # a GRU stack: layer 0 too runs in the stacked kernel (the projection as given, both states at the row pitch)
        assert len(stack) == (0 if L == 1 else (L - 1 if lstm else L)), (core, ran)
        assert all(k == STACK_KERNELS[1 if lstm else 0] for k in stack)
        if L > 1:
            assert ran[:3] == got[core - (L - 1)][:3]                      # the stages in front of the recurrence: the single-layer handle's


def test_rnn_stack_0_is_the_general_route(routes, recorder):
    """EC_RNN_STACK=0: the new kernel is not launched; the layers run with the single-layer step kernels and one GEMM each"""
    got = _act_launches(routes, recorder, [2, 12, 3], env_extra={"EC_RNN_STACK": "0"})
    for core, ran in got.items():
        assert not [k for k in ran if k in STACK_KERNELS], (core, ran)
        L = core % 10
        step = "lstm_step_fwd_kernel" if core >= 10 else "gru_step_fwd_kernel"
        assert ran.count(step) == L and sum(k.startswith(("gemm_f32_kernel", "gemm_x3_kernel")) for k in ran) >= L - 1
    # ... and a T > 1 pass takes it whatever the switch says
    got = _act_launches(routes, recorder, [2, 12], T=3, reuse=0)
    for core, ran in got.items():
        assert not [k for k in ran if k in STACK_KERNELS], (core, ran)
        assert ran.count("lstm_step_fwd_kernel" if core >= 10 else "gru_step_fwd_kernel") == 6

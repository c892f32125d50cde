"""The pooled-embedding net on a box without a GPU: the new symbols declared, exported and bound; ``ec_policy_cfg`` unchanged; the
layout (tensor count, offsets in the documented order, state width, workspace sizes monotone in T and N); every refusal in front
of the first HIP call; and, through tools/launch_log.cpp standing in for the HIP runtime, the act step's launches: exactly 2 + L
with reused tables on the new route and the general route under EC_POOLED_ACT=0.  (The existing handles' launch lists are held
to their goldens by tests/test_policy_routes.py and tests/test_learn_routes.py, unchanged.)"""
import ctypes as C
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

NEW = ("ec_policy_create_pooled", "ec_policy_is_pooled", "ec_policy_forward_pooled", "ec_policy_act_pooled", "ec_pooled_fc_act",
       "ec_pooled_step0_fwd")
GRU, LSTM = 0, 1
P = 64        # a non-NULL, 16-byte aligned "pointer": the checks under test return before anything is read
FC_KERNELS = ("pooled_fc_act_kernel<7>", "pooled_fc_act_kernel<8>")
STEP0_KERNELS = ("pooled_step0_kernel<false>", "pooled_step0_kernel<true>")
STACK_KERNELS = ("rnn_stack_step_kernel<false>", "rnn_stack_step_kernel<true>")
BASE = dict(embed_in=1024, hidden=512, embed_dims=32, num_goals=12, num_sensors=2, sensor_in=(2, 2, 0), num_actions=6,
            prev_action_dims=32, prev_action_null=1, rnn_type=LSTM, num_layers=2)


@pytest.fixture(scope="module")
def lib():
    from embodied_clip_amd import _lib
    return _lib.load()


def _cfg(**kw):
    from embodied_clip_amd import _lib
    d = dict(BASE, **kw)
    d["sensor_in"] = (C.c_int * 3)(*d["sensor_in"])
    return _lib.PooledCfg(**d)


def _create(lib, **kw):
    h = C.c_void_p()
    return lib.ec_policy_create_pooled(C.byref(h), C.byref(_cfg(**kw))), h


def test_symbols_are_declared_exported_and_bound(lib, repo_root):
    from embodied_clip_amd import _lib
    text = open(os.path.join(repo_root, "include", "ec_amd.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, header) and n in _lib.SIGNATURES and hasattr(lib, n), n
    # ec_policy_cfg is what it was: the pooled net has a struct of its own
    assert [f[0] for f in _lib.PolicyCfg._fields_] == ["in_channels", "spatial", "hidden", "goal_dims", "num_goals", "num_actions",
                                                        "compress_hid", "compress_out", "comb_hid", "comb_out", "fusion", "dual",
                                                        "goal_in", "prev_action_dims", "prev_action_null"]
    body = header[:header.index("} ec_pooled_cfg;")]
    body = body[body.rindex("typedef struct {"):]
    fields = re.findall(r"\b([a-z_]+)(?:\[3\])?\s*[,;]", body)
    assert fields == [f[0] for f in _lib.PooledCfg._fields_]
    assert C.sizeof(_lib.PooledCfg) == 13 * 4
    assert "[U]" in text[text.index("The pooled-embedding net"):text.index("ec_pooled_cfg;")] and "parity unpinned" in text


@pytest.mark.parametrize("kw", [
    dict(embed_in=1024, hidden=512, num_goals=12, sensors=(2, 2), num_actions=6, prev_action_dims=32, rnn_type="LSTM", rnn_layers=2),
    dict(embed_in=2048, hidden=512, num_goals=0, sensors=(3,), num_actions=4, prev_action_dims=32, rnn_type="LSTM", rnn_layers=2),
    dict(embed_in=64, hidden=40, num_goals=5, sensors=(), num_actions=84, prev_action_dims=0, rnn_type="GRU", rnn_layers=1),
    dict(embed_in=72, hidden=64, num_goals=3, sensors=(1, 2, 5), num_actions=6, prev_action_dims=6, prev_action_null=0, rnn_type="GRU",
         rnn_layers=3),
])
def test_layout(lib, kw):
    from embodied_clip_amd import synthetic as syn
    from embodied_clip_amd.policy import PolicyHandle, pooled_param_shapes
    h = PolicyHandle.pooled(**kw)
    assert lib.ec_policy_is_pooled(h.h) == 1
    H, D, L = kw["hidden"], kw["embed_in"], kw["rnn_layers"]
    lstm = kw["rnn_type"] == "LSTM"
    G, SW = (4 * H, 2 * H) if lstm else (3 * H, H)
    ids, S, E = int(kw["num_goals"] > 0), len(kw["sensors"]), kw["prev_action_dims"]
    names = list(h.offsets)
    assert lib.ec_policy_num_param_tensors(h.h) == len(names) == 2 + ids + 2 * S + 8 + (1 if E else 0) + 4 * (L - 1)
    assert h.state_width == L * SW == lib.ec_policy_state_width(h.h)
    assert lib.ec_policy_rnn_type(h.h) == (1 if lstm else 0) and lib.ec_policy_rnn_layers(h.h) == L
    # the documented order, and offsets that follow each other (16-byte aligned, no overlap, nothing behind the last tensor)
    want = ["visual_fc.1.weight", "visual_fc.1.bias"] + (["obj_categories_embedding.weight"] if ids else [])
    assert names[:len(want)] == want
    i0 = names.index("state_encoder.rnn.weight_ih_l0")
    assert i0 == 2 + ids + 2 * S and all(n.endswith(("_embedding.weight", "_embedding.bias", "_embeding.weight", "_embeding.bias"))
                                         for n in names[2 + ids:i0])
    assert names[i0:i0 + 8] == ["state_encoder.rnn.weight_ih_l0", "state_encoder.rnn.weight_hh_l0", "state_encoder.rnn.bias_ih_l0",
                                "state_encoder.rnn.bias_hh_l0", "action_distribution.linear.weight", "action_distribution.linear.bias",
                                "critic.fc.weight", "critic.fc.bias"]
    tail = (["prev_action_embedding.weight"] if E else []) + [k for l in range(1, L) for k in syn.policy_rnn_layer_tensors(l)]
    assert names[i0 + 8:] == tail
    assert h.shapes["state_encoder.rnn.weight_ih_l0"] == (G, H + 32 * (ids + S) + E) and h.shapes["visual_fc.1.weight"] == (H, D)
    end = 0
    for n in names:
        off, num = h.offsets[n]
        assert off % 4 == 0 and end <= off < end + 4, n
        end = off + num
    assert end <= h.flat_size < end + 4
    off, num = C.c_size_t(), C.c_size_t()
    assert lib.ec_policy_param_offset(h.h, len(names), C.byref(off), C.byref(num)) == -1
    # the recurrent section: weight_ih_l0 .. critic.fc.bias, one contiguous range in front of the tensors that end the order
    sec = h.recurrent_section()
    assert sec.start == h.offsets["state_encoder.rnn.weight_ih_l0"][0]
    assert sec.stop == (h.offsets[tail[0]][0] if tail else h.flat_size)
    # workspace sizes: monotone in T and in N, a learn pass needs more than an act step
    sizes = {(T, N, b): h.workspace_bytes(T, N, b) for T in (1, 4, 16) for N in (1, 8, 33) for b in (False, True)}
    assert all(v > 0 for v in sizes.values())
    for b in (False, True):
        for N in (1, 8, 33):
            assert sizes[(1, N, b)] < sizes[(4, N, b)] < sizes[(16, N, b)]
        for T in (1, 4, 16):
            assert sizes[(T, 1, b)] < sizes[(T, 8, b)] < sizes[(T, 33, b)]
    assert all(sizes[(T, N, True)] > sizes[(T, N, False)] for T in (4, 16) for N in (8, 33))
    sd = syn.policy_state_dict(0, pooled=h.pooled_cfg)
    assert list(sd) == names and all(tuple(sd[n].shape) == tuple(h.shapes[n]) for n in names)
    assert syn.policy_param_shapes(pooled=h.pooled_cfg) == pooled_param_shapes(**h.pooled_cfg)
    assert float(sd["visual_fc.1.weight"].std()) > 0 and float(sd["state_encoder.rnn.weight_ih_l0"].std()) > 0


def test_constructor_refusals(lib):
    ARG, SHAPE = -1, -2
    assert lib.ec_policy_create_pooled(None, C.byref(_cfg())) == ARG
    h = C.c_void_p()
    assert lib.ec_policy_create_pooled(C.byref(h), None) == ARG
    assert _create(lib, num_goals=0, num_sensors=0)[0] == ARG                          # the net needs a goal
    assert _create(lib, sensor_in=(4, 5, 0))[0] == ARG                                 # K = 9 > 8
    assert _create(lib, num_sensors=3, sensor_in=(3, 3, 3))[0] == ARG
    assert _create(lib, sensor_in=(2, 0, 0))[0] == ARG and _create(lib, num_sensors=4)[0] == ARG and _create(lib, num_sensors=-1)[0] == ARG
    assert _create(lib, embed_dims=0)[0] == ARG and _create(lib, embed_dims=65)[0] == ARG
    assert _create(lib, num_actions=1)[0] == ARG and _create(lib, num_actions=257)[0] == ARG
    assert _create(lib, num_goals=-1)[0] == ARG and _create(lib, num_goals=257)[0] == ARG
    assert _create(lib, prev_action_dims=65)[0] == ARG and _create(lib, prev_action_dims=0, prev_action_null=1)[0] == ARG
    assert _create(lib, prev_action_null=2)[0] == ARG
    assert _create(lib, rnn_type=2)[0] == ARG and _create(lib, num_layers=0)[0] == ARG and _create(lib, num_layers=5)[0] == ARG
    assert _create(lib, embed_in=60)[0] == SHAPE and _create(lib, embed_in=4100)[0] == SHAPE and _create(lib, embed_in=66)[0] == SHAPE
    assert _create(lib, hidden=40)[0] == SHAPE and _create(lib, hidden=640)[0] == SHAPE          # the LSTM's widths
    assert _create(lib, hidden=42, rnn_type=GRU)[0] == SHAPE
    rc, h = _create(lib, hidden=40, rnn_type=GRU)                                       # a GRU takes it (the general route)
    assert rc == 0 and lib.ec_policy_state_width(h) == 80
    lib.ec_policy_destroy(h)
    assert lib.ec_policy_is_pooled(None) == 0
    from embodied_clip_amd.policy import PolicyHandle
    for bad in (dict(num_goals=0, sensors=()), dict(sensors=(4, 5)), dict(sensors=(1, 1, 1, 1)), dict(rnn_layers=5), dict(rnn_type="RNN")):
        with pytest.raises(ValueError):
            PolicyHandle.pooled(64, 64, **bad)


def test_entry_point_refusals(lib):
    """argument pairings, pooled against non-pooled entry points: all EC_ERR_ARG, all before any HIP call (the pointers are fake)"""
    from embodied_clip_amd import _lib
    ARG = -1
    rc, h = _create(lib)                                  # ids + sensors + previous action
    assert rc == 0
    rc, h_ids = _create(lib, num_sensors=0, sensor_in=(0, 0, 0), prev_action_dims=0, prev_action_null=0)
    assert rc == 0
    rc, h_sens = _create(lib, num_goals=0, num_sensors=1, sensor_in=(3, 0, 0), prev_action_dims=0, prev_action_null=0)
    assert rc == 0
    old = C.c_void_p()
    assert lib.ec_policy_create(C.byref(old), C.byref(_lib.PolicyCfg(in_channels=64, spatial=7, hidden=64, goal_dims=32, num_goals=12, num_actions=6,
                                                                    compress_hid=128, compress_out=32, comb_hid=128, comb_out=32))) == 0

    def fwd(hd, embed=P, goal=P, sens=P, prev=P, T=1, N=4):
        return lib.ec_policy_forward_pooled(hd, P, embed, goal, sens, prev, P, P, T, N, P, 1 << 40, 0, P, P + 4096, None)

    def act(hd, goal=P, sens=P, prev=P, greedy=0, expert=None, emask=None, p=0.0):
        return lib.ec_policy_act_pooled(hd, P, P, goal, sens, prev, P, P, 4, P, 1 << 40, 0, P, P + 4096, P, P, None, greedy, 1, 2, 0, expert, emask, p,
                                        None)
    for f in (fwd, act):
        # a NULL argument must match a part the handle does not have, and the reverse
        assert f(h, goal=None) == ARG and f(h, sens=None) == ARG and f(h, prev=None) == ARG
        assert f(h_ids, goal=P, sens=P, prev=None) == ARG and f(h_ids, goal=P, sens=None, prev=P) == ARG and f(h_ids, goal=None, sens=None, prev=None) == ARG
        assert f(h_sens, goal=P, sens=P, prev=None) == ARG and f(h_sens, goal=None, sens=None, prev=None) == ARG
        # ... and the pooled entry points refuse every other handle
        assert f(old, goal=P, sens=None, prev=None) == ARG and f(None) == ARG
    assert fwd(h, embed=P + 4) == ARG                      # the embedding rows are read as float4
    assert fwd(h, embed=None) == ARG
    assert fwd(h, T=0) == -2 and fwd(h, N=0) == -2         # (EC_ERR_SHAPE, still before any HIP call)
    assert act(h, expert=P) == ARG and act(h, expert=P, emask=P, p=1.5) == ARG and act(h, greedy=1, expert=P, emask=P, p=0.5) == ARG
    # the existing forward / act entry points refuse a pooled handle
    for hd in (h, h_ids, h_sens):
        assert lib.ec_policy_forward(hd, P, P, 0, P, P, P, 1, 4, P, 1 << 40, 0, P, P, None) == ARG
        assert lib.ec_policy_forward2(hd, P, P, None, 0, P, P, P, 1, 4, P, 1 << 40, 0, P, P, None) == ARG
        assert lib.ec_policy_forward_vec(hd, P, P, None, 0, P, P, P, 1, 4, P, 1 << 40, 0, P, P, None) == ARG
        assert lib.ec_policy_forward_pa(hd, P, P, None, 0, P, None, P, P, P, 1, 4, P, 1 << 40, 0, P, P, None) == ARG
        assert lib.ec_policy_act(hd, P, P, None, 0, P, P, P, 4, P, 1 << 40, 0, P, P, P, P, None, 1, 2, 0, None) == ARG
        assert lib.ec_policy_act_vec(hd, P, P, None, 0, P, P, P, 4, P, 1 << 40, 0, P, P, P, P, None, 1, 2, 0, None) == ARG
        assert lib.ec_policy_act_greedy(hd, P, P, None, 0, P, P, P, 4, P, 1 << 40, 0, P, P, P, P, None, None) == ARG
        assert lib.ec_policy_act_vec_greedy(hd, P, P, None, 0, P, P, P, 4, P, 1 << 40, 0, P, P, P, P, None, None) == ARG
        assert lib.ec_policy_act_ex(hd, P, P, None, 0, P, None, P, P, 4, P, 1 << 40, 0, P, P, P, P, None, 0, 1, 2, 0, None, None, 0.0, None) == ARG
        assert lib.ec_policy_act_pa(hd, P, P, None, 0, P, None, P, P, P, 4, P, 1 << 40, 0, P, P, P, P, None, 0, 1, 2, 0, None, None, 0.0, None) == ARG
        assert lib.ec_policy_set_goal_table(hd, P) == ARG
    # the backward refuses misaligned embedding rows with the other argument checks, before any launch
    assert lib.ec_policy_backward3(h, P, P + 4, None, 0, P, 1, 4, P, 1 << 40, P, None, P, None, None) == ARG
    # a workspace that is too small is noticed before any launch
    assert lib.ec_policy_forward_pooled(h, P, P, P, P, P, P, P, 1, 4, P, 16, 0, P, P + 4096, None) == -4
    for hd in (h, h_ids, h_sens, old):
        lib.ec_policy_destroy(hd)


def test_kernel_argument_checks(lib):
    ARG, SHAPE = -1, -2
    fc = lambda e=P, w=P, b=P, wf=P, v=P, N=4, D=64, H=32: lib.ec_pooled_fc_act(e, w, b, wf, v, N, D, H, None)
    for k in ("e", "w", "wf", "v"):
        assert fc(**{k: None}) == ARG, k
    for k in ("e", "w", "wf"):
        assert fc(**{k: P + 4}) == ARG, k
    for kw in (dict(D=72), dict(D=60), dict(H=40), dict(N=0), dict(D=0), dict(H=0)):
        assert fc(**kw) == SHAPE, kw

    def step(rnn=LSTM, x=P, ldx=64, wih=P, whh=P, bih=P, bhh=P, sb=None, gt=None, goal=None, ng=0, pt=None, prev=None, null=0, A=6, sv=None,
             sens=None, K=0, st=P, ld=128, mask=P, h=P + 4096, ldh=64, c=P + 8192, ldc=64, h2=None, ldh2=0, N=4, H=64):
        return lib.ec_pooled_step0_fwd(rnn, x, ldx, wih, whh, bih, bhh, sb, gt, goal, ng, pt, prev, null, A, sv, sens, K, st, ld, mask, h, ldh,
                                       c, ldc, h2, ldh2, N, H, None)
    for k in ("x", "wih", "whh", "bih", "bhh", "st", "mask", "h", "c"):
        assert step(**{k: None}) == ARG, k
    assert step(rnn=2) == ARG
    assert step(h=P) == ARG                                # in place: refused
    assert step(gt=P) == ARG and step(goal=P) == ARG and step(pt=P) == ARG and step(prev=P) == ARG and step(sv=P) == ARG and step(sens=P) == ARG
    assert step(gt=P, goal=P, ng=0) == ARG and step(gt=P, goal=P, ng=257) == ARG
    assert step(pt=P, prev=P, A=0) == ARG and step(pt=P, prev=P, null=2) == ARG
    assert step(sv=P, sens=P, K=0) == ARG and step(sv=P, sens=P, K=9) == ARG
    for kw in (dict(N=0), dict(H=40), dict(H=640, ldx=640, ld=1280, ldh=640, ldc=640), dict(ldx=60), dict(ldx=66), dict(ld=64), dict(ld=130),
               dict(ldh=32), dict(ldc=60), dict(h2=P, ldh2=32), dict(rnn=GRU, ld=60)):
        assert step(**kw) == SHAPE, kw
    for k in ("x", "wih", "whh", "st"):
        assert step(**{k: P + 4}) == ARG, k


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
    return routes.build_recorder(str(tmp_path_factory.mktemp("launch_log_pooled")), CXX)


def _cmd(D=1024, H=512, goals=12, sensors=(2, 2), A=6, E=32, null=1, rnn=LSTM, L=2, T=1, N=32, mode=0, reuse=1, inplace=0, act=1):
    k = tuple(sensors) + (0,) * (3 - len(sensors))
    return "pooled %d %d 32 %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d" % (D, H, goals, len(sensors), k[0], k[1], k[2], A, E, null, rnn, L, T, N,
                                                                                 mode, reuse, inplace, act)


def _run(routes, recorder, cmds, env_extra=None):
    """-> [[kernel names (and "D" for a copy) of the recorded call]] per command; what built the tables is dropped"""
    from embodied_clip_amd import _lib
    env = {k: v for k, v in os.environ.items() if not k.startswith("EC_")}
    env.update(env_extra or {})
    r = subprocess.run([recorder, _lib.LIB_PATH], input="".join(c + "\n" for c in cmds), capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr
    out, cur = [], None
    for line in r.stdout.splitlines():
        tag, rest = line[0], line[2:]
        if tag == "C":
            cur = []
            out.append(cur)
        elif tag in "BF":
            assert int(rest) == 0
            if tag == "B":
                cur.clear()
        elif tag == "L":
            cur.append(routes.short(rest.split("|")[0]))
        elif tag == "D":
            cur.append("D")
        elif tag == "R":
            assert int(rest) == 0, line
    assert len(out) == len(cmds)
    return out


@pytest.mark.parametrize("A", [6, 84])
@pytest.mark.parametrize("rnn", [GRU, LSTM])
@pytest.mark.parametrize("L", [1, 2])
def test_act_step_with_reused_tables_is_two_plus_L_launches(routes, recorder, L, rnn, A):
    (ran,) = _run(routes, recorder, [_cmd(A=A, rnn=rnn, L=L)])
    assert len(ran) == 2 + L and "D" not in ran, ran
    assert ran[0] == "pooled_fc_act_kernel<8>" and ran[1] == STEP0_KERNELS[rnn], ran
    assert ran[2:-1] == [STACK_KERNELS[rnn]] * (L - 1)
    assert ran[-1] == ("heads_fwd_kernel<8>" if A == 6 else "wa_heads_kernel"), ran
    # D % 56 == 0 and not % 64: seven waves; a plain forward call at T = 1 takes the same route in front of the heads
    (ran7, fwd) = _run(routes, recorder, [_cmd(D=112, A=A, rnn=rnn, L=L), _cmd(A=A, rnn=rnn, L=L, act=0)])
    assert ran7[0] == "pooled_fc_act_kernel<7>" and ran7[1:] == ran[1:]
    assert fwd[:1 + L] == ran[:1 + L]


def test_first_act_step_builds_the_tables(routes, recorder):
    (ran,) = _run(routes, recorder, [_cmd(reuse=0)])
    assert ran[-4:] == ["pooled_fc_act_kernel<8>", STEP0_KERNELS[LSTM], STACK_KERNELS[LSTM], "heads_fwd_kernel<8>"]
    built = ran[:-4]
    assert sorted(built) == sorted(["pa_rows_copy_kernel", "pa_table_kernel", "pa_table_kernel", "pooled_tables_kernel", "pooled_frag_pack_kernel"])


def test_general_route(routes, recorder):
    """EC_POOLED_ACT=0, a width the fc kernel does not take, and h_final == h0: neither new act kernel; GEMMs with the rows-add"""
    new = FC_KERNELS + STEP0_KERNELS
    gemm = lambda ran: sum(k.startswith(("gemm_f32_kernel", "gemm_x3_kernel")) for k in ran)
    for rnn, L in ((GRU, 1), (LSTM, 2)):
        off = _run(routes, recorder, [_cmd(rnn=rnn, L=L)], env_extra={"EC_POOLED_ACT": "0"})[0]
        assert not [k for k in off if k in new], off
        assert off.count("pooled_rows_add_kernel") == 1 and gemm(off) == 2, off
        step = "lstm_step_fwd_kernel" if rnn == LSTM else "gru_step_fwd_kernel"
        assert off.count(step) == 1 and off.count(STACK_KERNELS[rnn]) == L - 1
        d72, inplace = _run(routes, recorder, [_cmd(D=72, rnn=rnn, L=L), _cmd(rnn=rnn, L=L, inplace=1)])
        assert not [k for k in d72 if k in new] and d72.count("pooled_rows_add_kernel") == 1
        assert not [k for k in inplace if k in new] and inplace.count("pooled_rows_add_kernel") == 1
    # T > 1: the general route whatever the switch says, layer by layer
    (seq,) = _run(routes, recorder, [_cmd(T=3, N=5, reuse=0, act=0)])
    assert not [k for k in seq if k in new + STACK_KERNELS] and seq.count("lstm_step_fwd_kernel") == 6 and seq.count("pooled_rows_add_kernel") == 1


def test_learn_pass_launches_no_float_atomics_kernel(routes, recorder):
    """a learn pass and its backward run; the binned goal / previous-action sums and the sensor chain are in it, the atomic goal
    scatter of the goal-encoder handle is not"""
    (ran,) = _run(routes, recorder, [_cmd(T=3, N=5, mode=2, reuse=0, act=0)])
    assert ran.count("pa_bin_kernel") == 2 and ran.count("pooled_sensor_dwih_kernel") == 1 and ran.count("pooled_sensor_dw_kernel") == 1
    assert "group_sum_scatter_kernel" not in ran and ran.count("D") == 3          # previous actions, goal ids, sensors: kept for the backward


def test_engine_refusals_need_no_gpu():
    """``Worker`` / ``Evaluator`` ``(net="pooled", ...)``: ``engine.check_net`` is their first statement and raises before anything
    is allocated or the library is loaded"""
    from embodied_clip_amd.engine import Worker, check_net
    from embodied_clip_amd.evaluate import Evaluator
    assert check_net("goal_encoder", "attnpool", (), True, "rn50", False, False, 0) == (False, None, ())
    assert check_net("pooled", "attnpool", (2, 2), True, "rn50", False, False, 0) == (True, "attnpool", (2, 2))
    assert check_net("pooled", "avgpool", [3], False, "imagenet_rn50", False, False, 0) == (True, "avgpool", (3,))
    for cls in (Worker, Evaluator):
        for bad in (dict(depth=True), dict(zeroshot=True), dict(goal_in=2), dict(encoder="vit"), dict(encoder="imagenet_rn18", pooling="attnpool"),
                    dict(pooling="maxpool"), dict(goal_ids=False), dict(sensors=(4, 5)), dict(sensors=(1, 1, 1, 1)), dict(net="other")):
            with pytest.raises(ValueError):
                cls(8, T=4, device="cuda:0", **{**dict(net="pooled"), **bad})
        with pytest.raises(ValueError):
            cls(8, T=4, device="cuda:0", sensors=(2,))

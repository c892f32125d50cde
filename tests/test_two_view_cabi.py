"""The two-view rearrangement net on a box without a GPU: the new symbols declared, exported and bound; ``ec_policy_cfg`` and
``ec_pooled_cfg`` unchanged; the layout (tensor count, offsets in the documented order against the state dict, state width,
workspace sizes monotone in T and N); every refusal in front of the first HIP call -- the constructor's, the entry points'
pairings with the other handles, the stand-alone kernels' shapes; ``check_net`` before any allocation; and the layouts of the
existing handles, unchanged."""
import ctypes as C
import os
import re

import pytest

# recorded from the parent commit's library (flat sizes in floats, workspace sizes in bytes)
PARENT_WS = dict(default_flat=3480780, default_act32=28412160, default_learn=303513856, pooled_flat=4993836, pooled_act32=8388864,
                 pooled_learn=26866432, pa_flat=6756280, pa_learn=161010944)
NEW = ("ec_policy_create_two_view", "ec_policy_is_two_view", "ec_policy_forward_two_view", "ec_policy_act_two_view",
       "ec_two_view_workspace_bytes", "ec_two_view_fwd", "ec_two_view_bwd")
GRU, LSTM = 0, 1
ARG, SHAPE, WORKSPACE = -1, -2, -4
P = 64        # a non-NULL, 16-byte aligned "pointer": the checks under test return before anything is read
BASE = dict(in_channels=2048, spatial=7, hidden=512, attn_hidden=32, num_actions=84, prev_action_dims=512, prev_action_null=1,
            rnn_type=LSTM, num_layers=1)


@pytest.fixture(scope="module")
def lib():
    from embodied_clip_amd import _lib
    return _lib.load()


def _create(lib, **kw):
    from embodied_clip_amd import _lib
    h = C.c_void_p()
    return lib.ec_policy_create_two_view(C.byref(h), C.byref(_lib.TwoViewCfg(**dict(BASE, **kw)))), h


def test_symbols_are_declared_exported_and_bound(lib, repo_root):
    from embodied_clip_amd import _lib
    text = open(os.path.join(repo_root, "include", "ec_amd.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, header) and n in _lib.SIGNATURES and hasattr(lib, n), n
    body = header[:header.index("} ec_two_view_cfg;")]
    body = body[body.rindex("typedef struct {"):]
    fields = re.findall(r"\b([a-z_]+)\s*[,;]", body)
    assert fields == [f[0] for f in _lib.TwoViewCfg._fields_]
    assert C.sizeof(_lib.TwoViewCfg) == 9 * 4
    # the other handles' structs are what they were
    assert len(_lib.PolicyCfg._fields_) == 15 and C.sizeof(_lib.PooledCfg) == 13 * 4
    doc = text[text.index("The two-view rearrangement net"):text.index("ec_two_view_cfg;")]
    assert "[U]" in doc and "parity unpinned" in doc
    assert lib.ec_version() >= 630


@pytest.mark.parametrize("kw", [
    dict(in_channels=2048, hidden=512, num_actions=84, prev_action_dims=512, rnn_type="LSTM", rnn_layers=1),
    dict(in_channels=64, hidden=96, num_actions=6, prev_action_dims=96, rnn_type="GRU", rnn_layers=2),
    dict(in_channels=192, hidden=32, num_actions=84, prev_action_dims=6, prev_action_null=0, rnn_type="GRU", rnn_layers=3, spatial=3),
    dict(in_channels=64, hidden=64, num_actions=6, attn_hidden=64, prev_action_dims=0, rnn_type="LSTM", rnn_layers=2, spatial=8),
])
def test_layout(lib, kw):
    from embodied_clip_amd import synthetic as syn
    from embodied_clip_amd.policy import PolicyHandle, two_view_param_shapes
    h = PolicyHandle.two_view(**kw)
    assert lib.ec_policy_is_two_view(h.h) == 1 and lib.ec_policy_is_pooled(h.h) == 0
    H, Cc, L, A = kw["hidden"], kw["in_channels"], kw["rnn_layers"], kw["num_actions"]
    A1, E = kw.get("attn_hidden", 32), kw["prev_action_dims"]
    null = kw.get("prev_action_null", 1) if E else 0
    lstm = kw["rnn_type"] == "LSTM"
    G, SW = (4 * H, 2 * H) if lstm else (3 * H, H)
    names = list(h.offsets)
    assert lib.ec_policy_num_param_tensors(h.h) == len(names) == 6 + 8 + (1 if E else 0) + 4 * (L - 1)
    assert h.state_width == L * SW == lib.ec_policy_state_width(h.h)
    assert lib.ec_policy_rnn_type(h.h) == (1 if lstm else 0) and lib.ec_policy_rnn_layers(h.h) == L
    want = ["visual_encoder.0.weight", "visual_encoder.0.bias", "visual_attention.0.weight", "visual_attention.0.bias",
            "visual_attention.2.weight", "visual_attention.2.bias", "state_encoder.rnn.weight_ih_l0", "state_encoder.rnn.weight_hh_l0",
            "state_encoder.rnn.bias_ih_l0", "state_encoder.rnn.bias_hh_l0", "actor.linear.weight", "actor.linear.bias", "critic.fc.weight",
            "critic.fc.bias"]
    tail = (["prev_action_embedder.weight"] if E else []) + [k for l in range(1, L) for k in syn.policy_rnn_layer_tensors(l)]
    assert names == want + tail
    numel = lambda n: int(__import__("math").prod(h.shapes[n]))
    assert numel("visual_encoder.0.weight") == H * 3 * Cc and numel("visual_attention.0.weight") == A1 * 3 * Cc
    assert numel("visual_attention.2.weight") == A1 and numel("visual_attention.2.bias") == 1
    assert h.shapes["state_encoder.rnn.weight_ih_l0"] == (G, H + E) and h.shapes["actor.linear.weight"] == (A, H)
    if E:
        assert h.shapes["prev_action_embedder.weight"] == (A + null, E)
    end = 0
    for n in names:          # offsets follow each other: 16-byte aligned, no overlap, nothing behind the last tensor
        off, num = h.offsets[n]
        assert off % 4 == 0 and end <= off < end + 4 and num == numel(n), n
        end = off + num
    assert end <= h.flat_size < end + 4
    off, num = C.c_size_t(), C.c_size_t()
    assert lib.ec_policy_param_offset(h.h, len(names), C.byref(off), C.byref(num)) == ARG
    sec = h.recurrent_section()
    assert sec.start == h.offsets["state_encoder.rnn.weight_ih_l0"][0]
    assert sec.stop == (h.offsets[tail[0]][0] if tail else h.flat_size)
    # the state dict: the same names, shapes that flatten onto the offsets, upstream's 4-D conv weights
    sd = syn.policy_state_dict(0, two_view=h.two_view_cfg)
    assert list(sd) == names and all(tuple(sd[n].shape) == tuple(h.shapes[n]) for n in names)
    assert syn.policy_param_shapes(two_view=h.two_view_cfg) == two_view_param_shapes(**h.two_view_cfg)
    assert sd["visual_encoder.0.weight"].dim() == 4 and float(sd["visual_encoder.0.weight"].std()) > 0
    flat = h.flatten(sd, "cpu")
    for n in names:
        o, k = h.offsets[n]
        assert bool((flat[o:o + k] == sd[n].reshape(-1)).all()), n
    # workspace sizes: monotone in T and in N; a learn pass keeps the probabilities and both convs' activations
    sizes = {(T, N, b): h.workspace_bytes(T, N, b) for T in (1, 4, 16) for N in (1, 8, 33) for b in (False, True)}
    assert all(v > 0 for v in sizes.values())
    for b in (False, True):
        for N in (1, 8, 33):
            assert sizes[(1, N, b)] < sizes[(4, N, b)] < sizes[(16, N, b)]
        for T in (1, 4, 16):
            assert sizes[(T, 1, b)] < sizes[(T, 8, b)] < sizes[(T, 33, b)]
    S2 = kw.get("spatial", 7) ** 2
    for T, N in ((4, 8), (16, 33)):
        assert sizes[(T, N, True)] - sizes[(T, N, False)] >= T * N * S2 * (H + A1 + 1) * 4
    # the stand-alone kernels' workspace: the planes of the combined weight (three bf16 planes), and for a backward the activations
    wb = lib.ec_two_view_workspace_bytes(8, S2, Cc, H, A1, 0)
    assert wb >= (H + A1) * 3 * Cc * 3 * 2 + 8 * S2 * 4
    assert lib.ec_two_view_workspace_bytes(8, S2, Cc, H, A1, 1) - wb >= 8 * S2 * (H + A1) * 4


def test_constructor_refusals(lib):
    from embodied_clip_amd import _lib
    assert lib.ec_policy_create_two_view(None, C.byref(_lib.TwoViewCfg(**BASE))) == ARG
    h = C.c_void_p()
    assert lib.ec_policy_create_two_view(C.byref(h), None) == ARG
    assert _create(lib, num_actions=1)[0] == ARG and _create(lib, num_actions=257)[0] == ARG
    assert _create(lib, prev_action_dims=513)[0] == ARG and _create(lib, prev_action_dims=-1)[0] == ARG
    assert _create(lib, prev_action_dims=0, prev_action_null=1)[0] == ARG and _create(lib, prev_action_null=2)[0] == ARG
    assert _create(lib, rnn_type=2)[0] == ARG and _create(lib, num_layers=0)[0] == ARG and _create(lib, num_layers=5)[0] == ARG
    assert _create(lib, in_channels=32)[0] == SHAPE and _create(lib, in_channels=96)[0] == SHAPE and _create(lib, in_channels=4160)[0] == SHAPE
    assert _create(lib, spatial=0)[0] == SHAPE and _create(lib, spatial=9)[0] == SHAPE           # S2 in 1..64
    assert _create(lib, attn_hidden=0)[0] == SHAPE and _create(lib, attn_hidden=48)[0] == SHAPE and _create(lib, attn_hidden=160)[0] == SHAPE
    assert _create(lib, hidden=40)[0] == SHAPE and _create(lib, hidden=640)[0] == SHAPE            # the LSTM's widths ...
    assert _create(lib, hidden=40, rnn_type=GRU)[0] == SHAPE                                      # ... on both cells
    for ok in (dict(prev_action_dims=512), dict(prev_action_dims=0, prev_action_null=0), dict(spatial=8, attn_hidden=128, in_channels=4096),
               dict(spatial=1, in_channels=64, hidden=32, rnn_type=GRU, num_layers=4)):
        rc, hd = _create(lib, **ok)
        assert rc == 0 and lib.ec_policy_is_two_view(hd) == 1, ok
        lib.ec_policy_destroy(hd)
    assert lib.ec_policy_is_two_view(None) == 0
    from embodied_clip_amd.policy import PolicyHandle
    for bad in (dict(rnn_layers=5), dict(rnn_type="RNN")):
        with pytest.raises(ValueError):
            PolicyHandle.two_view(64, 64, **bad)


def test_entry_point_refusals(lib):
    """argument pairings, two-view against the other entry points and handles: all before any HIP call (the pointers are fake)"""
    from embodied_clip_amd import _lib
    rc, h = _create(lib)                                  # with a previous-action embedding
    assert rc == 0
    rc, h0 = _create(lib, prev_action_dims=0, prev_action_null=0)
    assert rc == 0
    old = C.c_void_p()
    assert lib.ec_policy_create(C.byref(old), C.byref(_lib.PolicyCfg(in_channels=64, spatial=7, hidden=64, goal_dims=32, num_goals=12, num_actions=6,
                                                                    compress_hid=128, compress_out=32, comb_hid=128, comb_out=32))) == 0
    pooled = C.c_void_p()
    assert lib.ec_policy_create_pooled(C.byref(pooled), C.byref(_lib.PooledCfg(
        embed_in=1024, hidden=512, embed_dims=32, num_goals=12, num_sensors=0, sensor_in=(C.c_int * 3)(0, 0, 0), num_actions=6,
        prev_action_dims=0, prev_action_null=0, rnn_type=LSTM, num_layers=1))) == 0

    def fwd(hd, u=P, w=P, prev=P, T=1, N=4, ws=1 << 40):
        return lib.ec_policy_forward_two_view(hd, P, u, w, prev, P, P, T, N, P, ws, 0, P, P + 4096, None)

    def act(hd, u=P, w=P, prev=P, greedy=0, expert=None, emask=None, p=0.0):
        return lib.ec_policy_act_two_view(hd, P, u, w, prev, P, P, 4, P, 1 << 40, 0, P, P + 4096, P, P, None, greedy, 1, 2, 0, expert, emask, p, None)
    for f in (fwd, act):
        assert f(h, prev=None) == ARG and f(h0, prev=P) == ARG          # NULL must match a handle without the embedding
        assert f(h, w=None) == ARG and f(h, u=None) == ARG              # both views
        assert f(h, u=P + 4) == ARG and f(h, w=P + 8) == ARG            # 16-byte aligned
        assert f(old, prev=None) == ARG and f(pooled, prev=None) == ARG and f(None) == ARG      # every other handle
    assert fwd(h, T=0) == SHAPE and fwd(h, N=0) == SHAPE
    assert fwd(h, ws=16) == WORKSPACE
    assert act(h, expert=P) == ARG and act(h, expert=P, emask=P, p=1.5) == ARG and act(h, greedy=1, expert=P, emask=P, p=0.5) == ARG
    # every other forward / act entry point refuses the handle
    for hd in (h, h0):
        assert lib.ec_policy_forward(hd, P, P, 1, P, P, P, 1, 4, P, 1 << 40, 0, P, P, None) == ARG
        assert lib.ec_policy_forward2(hd, P, P, P, 1, P, P, P, 1, 4, P, 1 << 40, 0, P, P, None) == ARG
        assert lib.ec_policy_forward_vec(hd, P, P, P, 1, P, P, P, 1, 4, P, 1 << 40, 0, P, P, None) == ARG
        assert lib.ec_policy_forward_pa(hd, P, P, P, 1, P, None, P, P, P, 1, 4, P, 1 << 40, 0, P, P, None) == ARG
        assert lib.ec_policy_forward_pooled(hd, P, P, None, None, P, P, P, 1, 4, P, 1 << 40, 0, P, P + 4096, None) == ARG
        assert lib.ec_policy_forward_pooled(hd, P, P, None, None, None, P, P, 1, 4, P, 1 << 40, 0, P, P + 4096, None) == ARG
        assert lib.ec_policy_act(hd, P, P, P, 1, P, P, P, 4, P, 1 << 40, 0, P, P, P, P, None, 1, 2, 0, None) == ARG
        assert lib.ec_policy_act_vec(hd, P, P, P, 1, P, P, P, 4, P, 1 << 40, 0, P, P, P, P, None, 1, 2, 0, None) == ARG
        assert lib.ec_policy_act_greedy(hd, P, P, P, 1, P, P, P, 4, P, 1 << 40, 0, P, P, P, P, None, None) == ARG
        assert lib.ec_policy_act_vec_greedy(hd, P, P, P, 1, P, P, P, 4, P, 1 << 40, 0, P, P, P, P, None, None) == ARG
        assert lib.ec_policy_act_ex(hd, P, P, P, 1, P, None, P, P, 4, P, 1 << 40, 0, P, P, P, P, None, 0, 1, 2, 0, None, None, 0.0, None) == ARG
        assert lib.ec_policy_act_pa(hd, P, P, P, 1, P, None, P, P, P, 4, P, 1 << 40, 0, P, P, P, P, None, 0, 1, 2, 0, None, None, 0.0, None) == ARG
        assert lib.ec_policy_act_pooled(hd, P, P, None, None, None, P, P, 4, P, 1 << 40, 0, P, P + 4096, P, P, None, 0, 1, 2, 0, None, None, 0.0,
                                        None) == ARG
        assert lib.ec_policy_set_goal_table(hd, P) == ARG
        # the backward: both views, both bf16, aligned
        assert lib.ec_policy_backward3(hd, P, P, P, 0, P, 1, 4, P, 1 << 40, P, None, P, None, None) == ARG       # feat_bf16 = 0
        assert lib.ec_policy_backward3(hd, P, P, None, 1, P, 1, 4, P, 1 << 40, P, None, P, None, None) == ARG    # no second view
        assert lib.ec_policy_backward3(hd, P, P, P + 4, 1, P, 1, 4, P, 1 << 40, P, None, P, None, None) == ARG
        assert lib.ec_policy_backward3(hd, P, P, P, 1, P, 1, 4, P, 16, P, None, P, None, None) == WORKSPACE
    for hd in (h, h0, old, pooled):
        lib.ec_policy_destroy(hd)


def test_kernel_refusals(lib):
    """the stand-alone kernels: shapes and arguments refused before any launch"""
    ok = (5, 49, 64, 32, 32)
    assert lib.ec_two_view_workspace_bytes(*ok, 1) > lib.ec_two_view_workspace_bytes(*ok, 0) > 0
    big = 1 << 40
    for bad in [(5, 49, 96, 32, 32), (5, 49, 32, 32, 32), (5, 49, 4160, 32, 32), (5, 0, 64, 32, 32), (5, 65, 64, 32, 32),
                (5, 49, 64, 40, 32), (5, 49, 64, 640, 32), (5, 49, 64, 32, 48), (5, 49, 64, 32, 160), (5, 49, 64, 32, 0), (0, 49, 64, 32, 32)]:
        assert lib.ec_two_view_workspace_bytes(*bad, 0) == 0, bad
        assert lib.ec_two_view_fwd(P, P, P, P, P, P, P, P, P, *bad, P, big, 0, None) == SHAPE, bad
        assert lib.ec_two_view_bwd(P, P, P, P, P, P, P, P, P, P, *bad, P, big, None) == SHAPE, bad
    assert lib.ec_two_view_fwd(None, P, P, P, P, P, P, P, P, *ok, P, big, 0, None) == ARG
    assert lib.ec_two_view_fwd(P, P, P, P, P, P, P, P, None, *ok, P, big, 0, None) == ARG
    assert lib.ec_two_view_fwd(P + 2, P, P, P, P, P, P, P, P, *ok, P, big, 0, None) == ARG           # misaligned view
    assert lib.ec_two_view_bwd(P, P, P, P, P + 4, P, P, P, P, P, *ok, P, big, None) == ARG           # misaligned gradient
    assert lib.ec_two_view_bwd(P, P, P, None, P, P, P, P, P, P, *ok, P, big, None) == ARG
    assert lib.ec_two_view_fwd(P, P, P, P, P, P, P, P, P, *ok, P, 16, 0, None) == WORKSPACE
    assert lib.ec_two_view_bwd(P, P, P, P, P, P, P, P, P, P, *ok, P, 16, None) == WORKSPACE


def test_existing_handles_layouts_are_unchanged(lib, repo_root):
    """flat sizes, offsets and workspace sizes of handles that existed before, against values recorded from the parent commit"""
    from embodied_clip_amd.policy import PolicyHandle
    h = PolicyHandle()
    assert h.flat_size == PARENT_WS["default_flat"] and h.state_width == 512
    assert h.workspace_bytes(1, 32, False) == PARENT_WS["default_act32"] and h.workspace_bytes(128, 8, True) == PARENT_WS["default_learn"]
    hp = PolicyHandle.pooled(1024, 512, 12, (2, 2), 6, 32, 1, "LSTM", 2)
    assert hp.flat_size == PARENT_WS["pooled_flat"]
    assert hp.workspace_bytes(1, 32, False) == PARENT_WS["pooled_act32"] and hp.workspace_bytes(16, 8, True) == PARENT_WS["pooled_learn"]
    hpa = PolicyHandle(prev_action_dims=32, prev_action_null=1, num_actions=84, rnn_type="LSTM", rnn_layers=2)
    assert hpa.flat_size == PARENT_WS["pa_flat"] and hpa.workspace_bytes(16, 8, True) == PARENT_WS["pa_learn"]




def test_check_net_refusals_before_any_allocation():
    """``check_net`` is the first statement of ``Worker`` / ``Evaluator``: it raises on the host, before a handle or a tensor exists"""
    from embodied_clip_amd.engine import check_net, check_prev_actions
    ok = dict(net="two_view", pooling="attnpool", sensors=(), goal_ids=True, encoder="rn50", depth=False, zeroshot=False, goal_in=0)
    assert check_net(**ok) == (True, None, ())
    assert check_net(**dict(ok, encoder="imagenet_rn50")) == (True, None, ())
    for bad in (dict(depth=True), dict(zeroshot=True), dict(goal_in=2), dict(sensors=(2, 2)), dict(goal_ids=False), dict(pooling="avgpool"),
                dict(encoder="vit")):
        with pytest.raises(ValueError, match="two_view"):
            check_net(**dict(ok, **bad))
    with pytest.raises(ValueError):
        check_net(**dict(ok, net="three_view"))
    # the other nets' answers are what they were
    assert check_net("goal_encoder", "attnpool", (), True, "rn50", False, False, 0) == (False, None, ())
    assert check_net("pooled", "avgpool", (2, 2), True, "rn50", True, False, 0) == (True, "avgpool", (2, 2))
    assert check_prev_actions(512, False, False, 512) == 512 and check_prev_actions(64, False, False) == 64
    for E, cap in ((65, 64), (513, 512)):
        with pytest.raises(ValueError):
            check_prev_actions(E, False, False, cap)

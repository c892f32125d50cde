"""The previous-action embedding kernels on a box without a GPU: declared, exported, bound, every argument check in front of the
first HIP call, and the scratch size's closed form with its bound."""
import os
import re

import pytest

NEW = ("ec_prev_action_table", "ec_prev_action_add", "ec_prev_action_grad_scratch_floats", "ec_prev_action_grad")
P = 64        # a non-NULL "pointer": the checks under test return before anything is read


@pytest.fixture(scope="module")
def lib():
    from embodied_clip_amd import _lib
    return _lib.load()


def test_symbols_are_declared_exported_and_bound(lib, repo_root):
    from embodied_clip_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(repo_root, "include", "ec_amd.h")).read(), flags=re.S)
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, header), n
        assert n in _lib.SIGNATURES and hasattr(lib, n), n


def test_table_argument_checks(lib):
    def call(emb=P, w=P, ld=1574, col0=1568, pt=P, A=6, null=1, G=1536, E=6):
        return lib.ec_prev_action_table(emb, w, ld, col0, pt, A, null, G, E, None)
    for k in ("emb", "w", "pt"):
        assert call(**{k: None}) == -1, k
    for kw in (dict(A=0), dict(A=257), dict(null=2), dict(null=-1), dict(E=0), dict(E=65), dict(G=0), dict(col0=-1),
               dict(ld=1573), dict(col0=1569)):
        assert call(**kw) == -2, kw


def test_add_argument_checks(lib):
    def call(gi=P, pt=P, prev=P, masks=P, null=1, A=6, B=33, G=96):
        return lib.ec_prev_action_add(gi, pt, prev, masks, null, A, B, G, None)
    for k in ("gi", "pt", "prev", "masks"):
        assert call(**{k: None}) == -1, k
    for kw in (dict(A=0), dict(A=257), dict(null=2), dict(B=0), dict(G=0)):
        assert call(**kw) == -2, kw


def test_grad_argument_checks(lib):
    def call(dgi=P, prev=P, masks=P, null=1, A=6, emb=P, w=P, ld=1574, col0=1568, demb=P, dw=P, scratch=P, B=33, G=1536, E=6):
        return lib.ec_prev_action_grad(dgi, prev, masks, null, A, emb, w, ld, col0, demb, dw, scratch, B, G, E, None)
    for k in ("dgi", "prev", "masks", "emb", "w", "demb", "dw", "scratch"):
        assert call(**{k: None}) == -1, k
    for kw in (dict(A=0), dict(A=257), dict(null=2), dict(E=0), dict(E=65), dict(G=0), dict(B=0), dict(col0=-1), dict(ld=1573)):
        assert call(**kw) == -2, kw


def test_scratch_size_and_its_bound(lib):
    f = lib.ec_prev_action_grad_scratch_floats
    assert f(0, 96, 6, 1) == 0 and f(8, 96, 257, 0) == 0 and f(8, 96, 6, 2) == 0 and f(8, 0, 6, 1) == 0
    for (B, G, A, null) in ((1, 96, 1, 0), (33, 96, 6, 1), (1000, 1536, 6, 1), (1000, 1536, 256, 1), (32768, 1536, 6, 1),
                            (32768, 1536, 256, 1), (1 << 20, 1536, 6, 1)):
        R = A + null
        chunk = max(R, 128, -(-B // 4096))
        parts = -(-B // chunk)
        assert f(B, G, A, null) == (parts + 1) * R * G, (B, G, A, null)
        assert parts <= 4096 and parts * R < B + R                   # the partitions' bins: less than (B + R) * G floats
    # the real workload (256 actors x 128 steps, Habitat's table): the bins of all partitions are 1 / 18 of dgi
    assert (f(32768, 1536, 6, 1) - 7 * 1536) * 18 < 32768 * 1536


# ---- the policy handle: configuration, flat layout, refusals (no HIP call is reached) ----------------------------------------------
import ctypes as C  # noqa: E402
import json  # noqa: E402

POLICY_NEW = ("ec_policy_forward_pa", "ec_policy_act_pa")
REFERENCE = dict(in_channels=2048, spatial=7, hidden=512, goal_dims=32, num_goals=12, num_actions=6, compress_hid=128, compress_out=32,
                 comb_hid=128, comb_out=32, fusion=0, dual=0, goal_in=0)
WIH = "state_encoder.rnn.weight_ih_l0"
EMB = "prev_action_embedder.fc.weight"


def _create(lib, **kw):
    from embodied_clip_amd import _lib
    h = C.c_void_p()
    return lib.ec_policy_create(C.byref(h), C.byref(_lib.PolicyCfg(**dict(REFERENCE, **kw)))), h


def _layout(lib, h, shapes):
    offs = []
    for i in range(lib.ec_policy_num_param_tensors(h)):
        off, num = C.c_size_t(), C.c_size_t()
        assert lib.ec_policy_param_offset(h, i, C.byref(off), C.byref(num)) == 0
        offs.append([off.value, num.value])
    return dict(flat_size=lib.ec_policy_flat_size(h), param_offsets=offs,
                workspace_bytes=[[T, N, b, lib.ec_policy_workspace_bytes(h, T, N, b)] for T, N in shapes for b in (0, 1)])


def test_policy_symbols(lib, repo_root):
    from embodied_clip_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(repo_root, "include", "ec_amd.h")).read(), flags=re.S)
    for n in POLICY_NEW:
        assert re.search(r"\b%s\s*\(" % n, header) and n in _lib.SIGNATURES and hasattr(lib, n), n
    names = [f[0] for f in _lib.PolicyCfg._fields_]
    assert names[-2:] == ["prev_action_dims", "prev_action_null"] and names[-3] == "goal_in"      # two TRAILING ints


def test_zero_filled_cfg_is_todays_handle(lib, repo_root):
    """prev_action_dims = 0 (what every existing caller's zero-filled cfg says): the golden layout of the commit before the launch
    plan, tensor for tensor and workspace for workspace."""
    golden = json.load(open(os.path.join(repo_root, "tests", "golden", "policy_layout_golden.json")))
    for name in ("reference", "small", "small7"):
        g = golden[name]
        shapes = sorted({(T, N) for T, N, _, _ in g["workspace_bytes"]}, key=[(T, N) for T, N, _, _ in g["workspace_bytes"]].index)
        rc, h = _create(lib, **{k: v for k, v in g["cfg"].items()})
        assert rc == 0
        try:
            got = _layout(lib, h, shapes)
            assert got["flat_size"] == g["flat_size"] and got["param_offsets"] == g["param_offsets"], name
            assert got["workspace_bytes"] == g["workspace_bytes"], name
        finally:
            lib.ec_policy_destroy(h)


def test_embedding_layout(lib):
    from embodied_clip_amd.policy import PolicyHandle
    h0 = PolicyHandle()
    for (E, null, kw) in ((6, 1, {}), (7, 1, {}), (32, 1, dict(goal_in=3, num_actions=4)), (64, 0, dict(num_actions=256))):
        base = PolicyHandle(**kw)
        h = PolicyHandle(prev_action_dims=E, prev_action_null=null, **kw)
        R, flat = h.A + null, 32 * 49
        assert len(h.offsets) == len(base.offsets) + 1 and list(h.offsets)[:-1] == list(base.offsets) and list(h.offsets)[-1] == EMB
        assert h.offsets[WIH][1] == 3 * 512 * (flat + E) and h.shapes[WIH] == (1536, flat + E)
        assert h.offsets[EMB][1] == R * E and h.shapes[EMB] == (R, E)
        sec = h.recurrent_section()
        assert sec.start == h.offsets[WIH][0] and sec.stop == h.offsets[EMB][0]          # the new tensor: outside, in the late section
        assert h.offsets[EMB][0] + R * E <= h.flat_size
        for (T, N, b) in ((1, 32, False), (4, 8, True)):
            assert h.workspace_bytes(T, N, b) > base.workspace_bytes(T, N, b)
    unpadded = lambda h: sum(k for _, k in h.offsets.values())
    a, b = PolicyHandle(prev_action_dims=6, prev_action_null=1), PolicyHandle(prev_action_dims=7, prev_action_null=1)
    assert unpadded(b) - unpadded(a) == 3 * 512 + 7                                      # exactly 3H + R floats before padding
    assert unpadded(a) - unpadded(h0) == 6 * (3 * 512 + 7)


def test_create_refusals(lib):
    for kw, want in ((dict(prev_action_dims=-1), -1), (dict(prev_action_dims=65), -1), (dict(prev_action_dims=6, prev_action_null=2), -1),
                     (dict(prev_action_dims=6, prev_action_null=-1), -1), (dict(prev_action_dims=0, prev_action_null=1), -1),
                     (dict(prev_action_dims=6, dual=1), -6), (dict(prev_action_dims=6, fusion=1, spatial=1), -6),
                     (dict(prev_action_dims=64, prev_action_null=1, num_actions=256), 0), (dict(prev_action_dims=1, goal_in=2), 0)):
        rc, h = _create(lib, **kw)
        assert rc == want, (kw, rc)
        if rc == 0:
            lib.ec_policy_destroy(h)


def test_entry_point_pairing(lib):
    """On a handle with the embedding every older forward / act entry point returns EC_ERR_ARG; the _pa entry points return it on a
    handle without, and for NULL prev_actions."""
    W = 1 << 30
    for goal_in in (0, 2):
        _, he = _create(lib, prev_action_dims=6, prev_action_null=1, goal_in=goal_in)
        _, h0 = _create(lib, goal_in=goal_in)
        g, gv = (None, P) if goal_in else (P, None)
        try:
            fwd_pa = lambda h, prev: lib.ec_policy_forward_pa(h, P, P, None, 1, g, gv, prev, P, P, 2, 4, P, W, 0, P, P, None)
            act_pa = lambda h, prev: lib.ec_policy_act_pa(h, P, P, None, 1, g, gv, prev, P, P, 4, P, W, 0, P, P, P, P, P, 0, 1, 2, 0, None, None,
                                                          0.0, None)
            assert fwd_pa(h0, P) == -1 and act_pa(h0, P) == -1 and fwd_pa(he, None) == -1 and act_pa(he, None) == -1
            assert lib.ec_policy_forward_pa(he, P, P, None, 1, P, P, P, P, P, 2, 4, P, W, 0, P, P, None) == -1       # both goals
            assert lib.ec_policy_forward_pa(he, P, P, None, 1, g, gv, P, P, P, 2, 4, P, 16, 0, P, P, None) == -4     # reaches the plan: workspace
            assert lib.ec_policy_act_pa(he, P, P, None, 1, g, gv, P, P, P, 4, P, 16, 0, P, P, P, P, P, 0, 1, 2, 0, None, None, 0.0, None) == -4
            assert lib.ec_policy_forward(he, P, P, 1, P, P, P, 2, 4, P, W, 0, P, P, None) == -1
            assert lib.ec_policy_forward2(he, P, P, None, 1, P, P, P, 2, 4, P, W, 0, P, P, None) == -1
            assert lib.ec_policy_forward_vec(he, P, P, None, 1, P, P, P, 2, 4, P, W, 0, P, P, None) == -1
            for name in ("ec_policy_act", "ec_policy_act_vec"):
                assert getattr(lib, name)(he, P, P, None, 1, P, P, P, 4, P, W, 0, P, P, P, P, P, 1, 2, 0, None) == -1, name
            for name in ("ec_policy_act_greedy", "ec_policy_act_vec_greedy"):
                assert getattr(lib, name)(he, P, P, None, 1, P, P, P, 4, P, W, 0, P, P, P, P, P, None) == -1, name
            assert lib.ec_policy_act_ex(he, P, P, None, 1, g, gv, P, P, 4, P, W, 0, P, P, P, P, P, 0, 1, 2, 0, None, None, 0.0, None) == -1
        finally:
            lib.ec_policy_destroy(he)
            lib.ec_policy_destroy(h0)


def test_synthetic_defaults_and_the_new_tensor():
    import torch
    from embodied_clip_amd import synthetic as syn
    from embodied_clip_amd.policy import PolicyHandle
    assert syn.policy_param_order() == syn.POLICY_PARAM_ORDER and len(syn.policy_param_order()) == 17
    assert syn.policy_param_order(goal_in=2) == syn.POLICY_PARAM_ORDER_POINTNAV
    assert list(syn.policy_param_shapes()) == list(syn.POLICY_PARAM_ORDER) and syn.policy_param_shapes()[WIH] == (1536, 1568)
    sd0 = syn.policy_state_dict(3, in_channels=64, hidden=32)
    sdz = syn.policy_state_dict(3, in_channels=64, hidden=32, prev_action_dims=0, prev_action_null=0)
    assert list(sd0) == list(sdz) and all(torch.equal(sd0[k], sdz[k]) for k in sd0)
    assert sum(v.numel() for v in syn.policy_state_dict(0).values()) == 3480775
    sd = syn.policy_state_dict(0, prev_action_dims=6, prev_action_null=1)
    assert list(sd)[-1] == EMB and tuple(sd[EMB].shape) == (7, 6) and tuple(sd[WIH].shape) == (1536, 1574)
    assert 0.6 < float(sd[EMB].std()) < 1.4                           # N(0, 1), as embed_class
    for k in sd0:                                                     # every other tensor: today's, bit for bit
        if k != WIH:
            assert torch.equal(syn.policy_state_dict(3, in_channels=64, hidden=32, prev_action_dims=6)[k], sd0[k]), k
    h = PolicyHandle(prev_action_dims=6, prev_action_null=1)
    flat = h.flatten(sd, "cpu")
    back = h.views(flat)
    assert list(back) == list(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
    with pytest.raises(AssertionError, match="prev_actions"):
        h._prev_ptr(None, 4)
    with pytest.raises(AssertionError, match="prev_action_dims=0"):
        PolicyHandle()._prev_ptr(torch.zeros(4, dtype=torch.int64), 4)
